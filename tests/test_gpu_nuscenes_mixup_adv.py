"""NuScenesMixUpAdvDataset on the device: the adversarial half against the numpy edit on the same draws, the MixUp item, two
steps of the stage-2 consistency trainer and the round trip through tools/generate_pseudo_labels --perturb, all on the mini
nuScenes tree of tests/nuscenes_dataset_cases.py."""
import os
import pickle

import numpy as np
import pytest
import torch
import yaml

from tests import nuscenes_dataset_cases as C
from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
from toda_amd.pcdet.datasets import NuScenesMixUpAdvDataset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT = [0.0, 0.0, 1.8]
VOXEL = np.array([0.1, 0.1, 0.2], np.float32)
DB_BOXES = np.array([[0.0, 14.0, -1.0, 4.0, 1.8, 1.6, 0.0, 0.0, 0.0], [-4.0, -9.0, -1.0, 4.0, 1.8, 1.6, 0.2, 0.0, 0.0]], np.float32)  # free space too
DB_ROWS = 30
DB_INFO = "tiny_dbinfos.pkl"
EXTRA = np.array([[0.0, -22.0, -1.0, 4.0, 1.8, 1.6, 0.3], [12.0, 21.0, -1.0, 4.0, 1.8, 1.6, -0.4]], np.float32)      # free space in every frame


def frame_voxels(points):
    """(z, y, x) cells of a frame's own voxels: the shifted rows inside the grid of C.RANGE at 0.1 x 0.1 x 0.2 m."""
    lo, hi = np.array(C.RANGE[:3], np.float32), np.array(C.RANGE[3:], np.float32)
    xyz = points[:, :3] + np.array(SHIFT, np.float32)
    cell = np.floor((xyz - lo) / VOXEL)
    grid = np.round((hi.astype(np.float64) - lo) / VOXEL).astype(np.int64)
    inside = ((cell >= 0) & (cell < grid)).all(1)
    return np.unique(cell[inside].astype(np.int32)[:, ::-1], axis=0)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The mini tree; its training frames 1 and 2 once more as pseudo-labelled infos: their objects' boxes, a little off, and two
    boxes in free space, scores on both sides of 0.3, the frames' own voxels with random gradients."""
    path = tmp_path_factory.mktemp("advmix_gpu")
    root = C.write_tree(path)
    with open(root / "nuscenes_infos_10sweeps_train.pkl", "rb") as f:
        infos = pickle.load(f)
    rng = np.random.default_rng(17)
    pseudo = []
    for info in infos[1:]:
        info = dict(info)
        boxes = np.concatenate([info["gt_boxes"][:, :7] + rng.normal(0, 0.05, (len(info["gt_boxes"]), 7)).astype(np.float32), EXTRA], 0)
        info["gt_boxes"], info["gt_names"] = boxes.astype(np.float32), np.array(["car"] * len(boxes))
        info["p_score"] = np.where(np.arange(len(boxes)) % 4 == 1, 0.2, 0.8).astype(np.float32)
        info["p_score"][-2:] = 0.9
        key = np.fromfile(str(root / info["lidar_path"]), np.float32).reshape(-1, 5)
        info["p_voxel_coords"] = frame_voxels(key)
        info["p_voxel_perturb"] = (rng.standard_normal((len(info["p_voxel_coords"]), 3)) * 50).astype(np.float32)
        pseudo.append(info)
    with open(path / "pseudo.pkl", "wb") as f:
        pickle.dump(pseudo, f)
    # the same frames with one pseudo box each: LIMIT_WHOLE_SCENE with 'car:2' then has one car left to paste
    sparse = []
    for info in pseudo:
        info = dict(info)
        info["gt_boxes"], info["gt_names"], info["p_score"] = info["gt_boxes"][4:5], info["gt_names"][4:5], np.array([0.8], np.float32)      # the car at (-12, -3): in range under every rotation
        sparse.append(info)
    with open(path / "pseudo_sparse.pkl", "wb") as f:
        pickle.dump(sparse, f)
    # a GT database of two cars in the frames' free space, stored as the database tools store it: rows relative to the box
    # centre, unshifted boxes with velocity
    (root / "tiny_db").mkdir()
    records = []
    for i, box in enumerate(DB_BOXES):
        rows = np.concatenate([rng.uniform(-0.4, 0.4, (DB_ROWS, 3)) * box[3:6] / 2, rng.uniform(0, 1, (DB_ROWS, 1)), np.zeros((DB_ROWS, 1))], 1)
        rows.astype(np.float32).tofile(str(root / "tiny_db" / f"{i}.bin"))
        records.append({"name": "car", "path": f"tiny_db/{i}.bin", "image_idx": 0, "gt_idx": i, "box3d_lidar": box.copy(), "num_points_in_gt": DB_ROWS,
                        "difficulty": 0})
    with open(root / DB_INFO, "wb") as f:
        pickle.dump({"car": records}, f)
    return path


def _dataset(tree, pseudo=None, **extra):
    cfg = C.dataset_cfg(tree, DATASET="NuScenesMixUpAdvDataset", MAX_SWEEPS=1, SHIFT_COOR=SHIFT, **extra)
    return NuScenesMixUpAdvDataset(cfg, C.CLASSES, training=True, pseudo_info_path=str(pseudo if pseudo is not None else tree / "pseudo.pkl"))


def _shifted_frame(ds, k):
    pts = ds.get_lidar_with_sweeps_host(k, 1)
    pts[:, :3] += np.array(SHIFT, np.float32)
    return pts


def test_the_adversarial_half_equals_the_numpy_edit_on_the_same_draws(tree):
    ds = _dataset(tree, MIXUP_PROB=0.0, GT_PROB=0.0)
    drawn = []
    draw = ds.draw_edits
    ds.draw_edits = lambda k: drawn.append(draw(k)) or drawn[-1]
    np.random.seed(21)
    item = ds.draw_item(1)
    assert item == ("same", 3 + 1)
    adv, org = ds.raw_pair(item)                                        # before the augmentor and the data processor
    assert len(drawn) == 1 and adv["points"].is_cuda and org["points"].is_cuda
    plain = _shifted_frame(ds, 4)
    n_boxes = int((ds.infos[4]["p_score"] > 0.3).sum())
    assert len(drawn[0]["op"]) == n_boxes == 15
    want = ds.adversarial_points_host(plain.copy(), ds.infos[4], drawn[0])
    got = adv["points"].cpu().numpy()
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    assert org["points"].cpu().numpy().tobytes() == plain.tobytes()
    assert want.shape != plain.shape or (want != plain).any()           # the edit did something
    kept = ds.infos[4]["gt_boxes"][ds.infos[4]["p_score"] >= 0.3].copy()
    kept[:, :3] += np.array(SHIFT, np.float32)
    for half in (adv, org):
        assert half["gt_boxes"].shape == (15, 8) and (half["gt_boxes"][:, :7] == kept).all() and (half["gt_boxes"][:, 7] == 1).all()
    assert ds.infos[4]["gt_boxes"].shape == (19, 7)                     # the infos themselves are left alone


def test_a_mixup_item_has_boxes_from_both_frames_and_lives_on_the_device(tree):
    ds = _dataset(tree, MIXUP_PROB=1.0)
    np.random.seed(5)
    adv, org = ds.raw_pair(("mixup", 0, 3))                             # labelled frame 0 with pseudo-labelled frame 1
    extra = EXTRA.copy()
    extra[:, :3] += np.array(SHIFT, np.float32)
    for half in (adv, org):
        boxes = half["gt_boxes"]
        assert half["points"].is_cuda and boxes.shape[1] == 8
        first = C.frame_boxes(0)[0][:, :7].copy()
        first[:, :3] += np.array(SHIFT, np.float32)
        assert (boxes[:17, :7] == first).all()                          # every box of the first frame
        assert len(boxes) == 19 and (boxes[17:, :7] == extra).all()     # of the second: the two that collide with none of them
    np.random.seed(6)
    adv, org = ds[0]
    for half in (adv, org):
        assert half["points"].is_cuda and half["points"].shape[1] == 5 and half["gt_boxes"].shape[1] == 8 and len(half["gt_boxes"]) > 0
        assert "augmentation_list" in half and "augmentation_params" in half
    batch = ds.collate_batch([ds[0], ds[1]])
    assert batch[0]["points"].is_cuda and batch[0]["batch_size"] == 2 and batch[1]["gt_boxes"].shape[0] == 2


def test_gt_sampling_of_the_shipped_augmentor_list_pastes_into_both_halves(tree):
    """The DATA_AUGMENTOR of toda_stage2_nus_advmix_real.yaml as shipped (gt_sampling 'car:2' with LIMIT_WHOLE_SCENE, flip,
    rotation, scaling) on a pseudo-labelled frame with one box: each half gains one car of the database with its class id, and box
    and rows sit SHIFT_COOR above where the database stores them."""
    from toda_amd import ops
    shipped = cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/models/toda_stage2_nus_advmix_real.yaml"), AttrDict()).DATA_CONFIG
    aug = shipped.DATA_AUGMENTOR
    assert [c.NAME for c in aug.AUG_CONFIG_LIST] == ["gt_sampling", "random_world_flip", "random_world_rotation", "random_world_scaling"]
    assert list(aug.DISABLE_AUG_LIST) == ["placeholder"] and list(aug.AUG_CONFIG_LIST[0].SAMPLE_GROUPS) == ["car:2"] and aug.AUG_CONFIG_LIST[0].LIMIT_WHOLE_SCENE
    aug.AUG_CONFIG_LIST[0].DB_INFO_PATH = [DB_INFO]
    ds = _dataset(tree, pseudo=tree / "pseudo_sparse.pkl", MIXUP_PROB=0.0, GT_PROB=0.0, DATA_AUGMENTOR=aug)
    stored = ds.data_augmentor.data_augmentor_queue[0].db_infos["car"]
    assert len(stored) == 2 and all(r["box3d_lidar"][2] == np.float32(-1.0) + np.float32(1.8) for r in stored)      # moved once, at construction
    np.random.seed(11)
    adv, org = ds[0]
    for half in (adv, org):
        boxes = half["gt_boxes"]
        assert half["points"].is_cuda and boxes.shape == (2, 8) and (boxes[:, 7] == 1).all()          # the frame's box and the pasted one
        assert half["augmentation_list"] == ["random_world_flip", "random_world_rotation", "random_world_scaling"]
        scale = half["augmentation_params"]["random_world_scaling"]
        assert abs(boxes[1, 2] / scale - 0.8) < 1e-5 and np.abs(boxes[1, 3:6] / scale - DB_BOXES[0, 3:6]).max() < 1e-5
        radius = np.hypot(boxes[1, 0], boxes[1, 1]) / scale
        assert min(abs(radius - np.hypot(*b[:2])) for b in DB_BOXES) < 1e-4                           # one of the two, rotated about z
        owner = ops.points_in_boxes(half["points"], torch.from_numpy(boxes[:, :7].copy()).cuda(), mode=2).cpu().numpy()
        assert int((owner == 1).sum()) == DB_ROWS                                                     # its rows came along, the scene's left the box


@pytest.fixture
def global_cfg_restored():
    """The tools merge their yaml into the process-wide cfg: put it back as it was, so nothing of this file's configs
    (SHIFT_COOR, PSEUDO_INFO_PATH, ...) is left for the tests that follow."""
    import copy

    from toda_amd.pcdet.config import cfg
    saved = copy.deepcopy(dict(cfg))
    yield
    cfg.clear()
    cfg.update(saved)


def _small_cfg_file(tree, tmp_path, dataset, info_test=None):
    """The stage-2 nuScenes config cut down to the mini tree: its range, 0.1 m voxels, the tree's tiny GT database, one layer per
    neck block."""
    cfg = cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/models/toda_stage2_nus_advmix_real.yaml"), AttrDict())
    data = cfg.DATA_CONFIG
    assert data.DATASET == "NuScenesMixUpAdvDataset" and data.MAX_SWEEPS == 1 and data.MIXUP_PROB == 0.6 and data.GT_PROB == 0.3
    assert data.MIXUP_TYPE == "gt+ps_gt+ps" and data.ALPHA == 2 and list(data.SHIFT_COOR) == SHIFT
    assert list(data.DATA_PROCESSOR[2].VOXEL_SIZE) == [0.075, 0.075, 0.2] and data.DATA_AUGMENTOR.AUG_CONFIG_LIST[0].NAME == "gt_sampling"
    data.pop("_BASE_CONFIG_", None)
    data.DATASET, data.DATA_PATH, data.VERSION, data.POINT_CLOUD_RANGE, data.REPEAT = dataset, str(tree), C.VERSION, C.RANGE, 1
    data.INFO_PATH = {"train": ["nuscenes_infos_10sweeps_train.pkl"], "test": [info_test or "nuscenes_infos_10sweeps_val.pkl"]}
    data.DATA_AUGMENTOR.AUG_CONFIG_LIST[0].DB_INFO_PATH = [DB_INFO]
    data.DATA_PROCESSOR[2].VOXEL_SIZE = [0.1, 0.1, 0.2]
    data.DATA_PROCESSOR[2].MAX_NUMBER_OF_VOXELS = {"train": 60000, "test": 60000}
    cfg.MODEL.BACKBONE_2D.LAYER_NUMS = [1, 1]
    cfg.MODEL.DENSE_HEAD.POST_PROCESSING.SCORE_THRESH = 0.0

    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        return v
    path = tmp_path / f"{dataset}.yaml"
    with open(path, "w") as f:
        yaml.safe_dump({k: plain(cfg[k]) for k in ("CLASS_NAMES", "DATA_CONFIG", "MODEL", "OPTIMIZATION")}, f)
    return str(path)


def test_two_steps_of_the_consistency_trainer(tree, tmp_path, global_cfg_restored):
    from toda_amd.tools import stage2_mixup_train_cl as stage2
    losses = []
    decorate = stage2.model_fn_decorator_cl

    def recording():
        fn = decorate()

        def wrapped(*args, **kwargs):
            out = fn(*args, **kwargs)
            losses.append(float(out[0].detach()))
            return out
        return wrapped
    stage2.model_fn_decorator_cl = recording
    try:
        np.random.seed(3)
        torch.manual_seed(3)
        steps = stage2.main(["--cfg_file", _small_cfg_file(tree, tmp_path, "NuScenesMixUpAdvDataset"), "--epochs", "1", "--batch_size", "2",
                             "--workers", "2", "--pseudo_info_path", str(tree / "pseudo.pkl")])
    finally:
        stage2.model_fn_decorator_cl = decorate
    assert steps == 2 and len(losses) == 2 and np.isfinite(losses).all()


def test_round_trip_through_the_pseudo_label_tool(tree, tmp_path, global_cfg_restored):
    from toda_amd.tools import generate_pseudo_labels as gen
    cfg_file = _small_cfg_file(tree, tmp_path, "NuScenesDataset", info_test="nuscenes_infos_10sweeps_train.pkl")
    unlabel = tree / C.VERSION / "nuscenes_infos_10sweeps_train.pkl"
    torch.manual_seed(1)
    pseudo = gen.main(["--cfg_file", cfg_file, "--pseudo_thresh", "0.05", "--batch_size", "2", "--perturb", "--unlabel_infos", str(unlabel),
                       "--output_dir", str(tmp_path / "out")])
    with open(pseudo, "rb") as f:
        infos = pickle.load(f)
    assert len(infos) == 3 and all({"gt_boxes", "gt_names", "p_score", "p_voxel_perturb", "p_voxel_coords", "lidar_path", "sweeps"} <= set(i) for i in infos)
    ds = _dataset(tree, pseudo=pseudo, MIXUP_PROB=0.5, PSEUDO_THRESH=0.05)
    assert len(ds.ps_infos) == 3 and len(ds.infos) == 6
    np.random.seed(4)
    for index in range(4):
        adv, org = ds[index]
        assert adv["points"].is_cuda and org["points"].is_cuda and torch.isfinite(adv["points"]).all()
        assert adv["gt_boxes"].shape[1] == 8 and len(adv["gt_boxes"]) > 0 and np.isfinite(adv["gt_boxes"]).all()
    frame = ds.frame(3, True)                                           # a pseudo-labelled frame of the tool's file through the edit
    assert frame["points"].is_cuda and frame["points"].shape[1] == 5 and frame["gt_boxes"].shape[1] == 7
