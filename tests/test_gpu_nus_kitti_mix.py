"""NusKittiMixDataset on the MI355X: KittiDataset.raw_frame, the two domains' prepared frames, a mixed sample against the mix
processors on the two prepared frames (bit for bit, the cloud never leaving the device), the unmixed branches against the
single datasets, the device field-of-view crop inside the mix, a target frame without an object, one SECOND-IoU stage-1 step
through the loader, and the evaluation through the DATA_CONFIG_TEST block of the stage-1 YAML.

Trees: the mini KITTI tree of tests/kitti_dataset_cases.py (its points keep clear of the field-of-view test's borderline bands, so
the device flags and numpy's agree on every row) and the mini nuScenes tree of tests/nuscenes_dataset_cases.py.  CutMix draws its
crop again until more than 10 000 target rows fall inside, so the mixed-sample tests read a second KITTI tree whose training
frames carry BIG_ROWS more rows spread over the range."""
import logging
import os

import numpy as np
import pytest
import torch

from tests import kitti_dataset_cases as kcases
from tests import nuscenes_dataset_cases as ncases
from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
from toda_amd.pcdet.datasets import build_dataloader
from toda_amd.pcdet.datasets.kitti.kitti_dataset import KittiDataset, create_kitti_infos
from toda_amd.pcdet.datasets.nuscenes.nuscenes_dataset import NuScenesDataset
from toda_amd.pcdet.datasets.two_dataset import NusKittiMixDataset
from toda_amd.pcdet.utils import calibration_kitti
from toda_amd.tools.test import test_data_config as choose_test_data

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE1 = os.path.join(ROOT, "toda_amd/tools/cfgs/models/toda_stage1_nus_kitti_polarmix_real.yaml")
KITTI_CLASSES = ["Car", "Pedestrian", "Cyclist"]
RANGE = [-25.6, -25.6, -5.0, 51.2, 25.6, 4.8]          # the nuScenes tree (+-25 m) and the KITTI boxes (x 9 to 35 m)
NUS_SHIFT, KITTI_SHIFT = [0.0, 0.0, 1.8], [0.0, 0.0, 1.6]
BIG_ROWS = 60_000
FRAME_IDS = ["000000", "000001", "000002"]
STEPS = [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
         {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}},
         {"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.1, 0.1, 0.2], "MAX_POINTS_PER_VOXEL": 10,
          "MAX_NUMBER_OF_VOXELS": {"train": 60000, "test": 60000}}]


@pytest.fixture(scope="module")
def gold():
    return kcases.load_golden()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def shifted(points, shift):
    out = points.copy()
    out[:, :3] += np.array(shift, np.float32)
    return out


def row_keys(rows):
    """The rows of an [n, 4] fp32 table as a set of their bytes."""
    rows = np.ascontiguousarray(rows, np.float32)
    return {rows[i].tobytes() for i in range(len(rows))}


def big_rows(frame):
    """BIG_ROWS rows spread over the x-y range, 1 m clear of the frame's boxes."""
    rng = np.random.default_rng(40 + int(frame))
    xyz = np.stack([rng.uniform(-25.0, 50.0, 2 * BIG_ROWS), rng.uniform(-25.0, 25.0, 2 * BIG_ROWS), rng.uniform(-2.5, 0.5, 2 * BIG_ROWS)], 1)
    clear = np.ones(len(xyz), bool)
    for _, box, _, _ in kcases.FRAMES[frame]:
        clear &= ~(np.abs(xyz - np.asarray(box[:3])) <= kcases.extents(box) / 2 + 1.0).all(1)
    xyz = xyz[clear][:BIG_ROWS]
    assert len(xyz) == BIG_ROWS
    return np.concatenate([xyz, rng.uniform(0, 1, (BIG_ROWS, 1))], 1).astype(np.float32)


@pytest.fixture(scope="module")
def trees(tmp_path_factory, gold):
    """(mini KITTI tree, the same with the big training frames, mini nuScenes tree), infos written."""
    kitti = kcases.write_tree(tmp_path_factory.mktemp("kitti"), gold)
    big = kcases.write_tree(tmp_path_factory.mktemp("kitti_big"), gold)
    for frame in kcases.SPLITS["train"]:
        rows = np.concatenate([kcases.frame_points(gold, frame)[0], big_rows(frame)], 0)
        rows.tofile(str(big / "training" / "velodyne" / f"{frame}.bin"))
    for root in (kitti, big):
        create_kitti_infos(kcases.dataset_cfg(root), KITTI_CLASSES, data_path=root, save_path=root)
    nus = tmp_path_factory.mktemp("nuscenes")
    ncases.write_tree(nus)
    return kitti, big, nus


def kitti_cfg(root, **extra):
    settings = {"SHIFT_COOR": KITTI_SHIFT, "FOV_POINTS_ONLY": False, "POINT_CLOUD_RANGE": RANGE, "DATA_PROCESSOR": STEPS}
    settings.update(extra)
    return kcases.dataset_cfg(root, **settings)


def nus_cfg(root, **extra):
    settings = {"MAX_SWEEPS": 1, "SHIFT_COOR": NUS_SHIFT, "BALANCED_RESAMPLING": False, "POINT_CLOUD_RANGE": RANGE, "DATA_PROCESSOR": STEPS}
    settings.update(extra)
    return ncases.dataset_cfg(root, **settings)


def mix_cfg(kitti_path, nus_path, mix_type="polarmix", kitti_classes=("Car",), nus_classes=("car",), joint=("car",), fov=False, **extra):
    cfg = {"DATASET": "NusKittiMixDataset", "CLASS_NAMES": list(joint), "MIX_TYPE": mix_type, "MIX_INC_METHOD": "center", "POLARMIX_PROB": 1.0, "CUTMIX_PROB": 1.0,
           "POLARMIX_RC_NUM": 1, "POLARMIX_DEGREE": 1.570796, "POLARMIX_DIS": "FULL", "POLARMIX_UPDATE_METHOD": ["FIX", "FIX", "FIX"],
           "LASERMIX_NUM_AREAS": 3, "LASERMIX_NUM_ANGLES": 2, "POINT_CLOUD_RANGE": RANGE,
           "POINT_FEATURE_ENCODING": {"encoding_type": "absolute_coordinates_encoding", "used_feature_list": ["x", "y", "z", "intensity"],
                                      "src_feature_list": ["x", "y", "z", "intensity", "timestamp"]},
           "DATA_PROCESSOR": STEPS, "NuScenesDataset": nus_cfg(nus_path, CLASS_NAMES=list(nus_classes)),
           "KittiDataset": kitti_cfg(kitti_path, CLASS_NAMES=list(kitti_classes), FOV_POINTS_ONLY=fov)}
    cfg.update(extra)
    return AttrDict(cfg)


# ---- 1. KittiDataset.raw_frame -----------------------------------------------------------------------------------------------
def all_frames(cfg):
    cfg["INFO_PATH"] = {"train": ["kitti_infos_trainval.pkl"], "test": ["kitti_infos_trainval.pkl"]}
    return cfg


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("fov", [True, False])
def test_getitem_is_prepare_data_on_the_raw_frame(trees, fov, training):
    steps = [STEPS[0], STEPS[2]]                                                          # no shuffle
    ds = KittiDataset(all_frames(kitti_cfg(trees[0], FOV_POINTS_ONLY=fov, DATA_PROCESSOR=steps, GET_ITEM_LIST=["points", "gt_boxes2d"])), KITTI_CLASSES, training=training)
    assert len(ds) == 3 and ds.on_device is fov
    for i, frame in enumerate(FRAME_IDS):
        got, raw = ds[i], ds.raw_frame(i)
        assert set(raw) == {"frame_id", "calib", "image_shape", "gt_names", "gt_boxes", "gt_boxes2d", "points"} | ({"road_plane"} if i == 0 else set())
        assert raw["gt_boxes"].shape == (17, 7) and "DontCare" not in raw["gt_names"] and len(raw["gt_names"]) == 17 and raw["gt_boxes2d"].shape == (17, 4)
        assert torch.is_tensor(raw["points"]) is fov
        want = ds.prepare_data(raw)
        assert set(got) == set(want) and got["frame_id"] == want["frame_id"] == frame and got["image_shape"].tolist() == [375, 1242]
        assert isinstance(got["calib"], calibration_kitti.Calibration)
        a, b = (p.cpu().numpy() if torch.is_tensor(p) else p for p in (got["points"], want["points"]))
        assert same_bits(a, b) and len(a) > 0 and same_bits(got["gt_boxes"], want["gt_boxes"]) and got["gt_boxes"].shape == (17, 8)
        assert same_bits(got["gt_boxes2d"], want["gt_boxes2d"])
        if i == 0:
            assert same_bits(got["road_plane"], want["road_plane"]) and got["road_plane"].shape == (4,)


def test_raw_frame_points_on_the_device(trees, gold):
    crop = KittiDataset(all_frames(kitti_cfg(trees[0], FOV_POINTS_ONLY=True)), KITTI_CLASSES, training=False)
    whole = KittiDataset(all_frames(kitti_cfg(trees[0])), KITTI_CLASSES, training=False)
    unshifted = KittiDataset(all_frames(kitti_cfg(trees[0], SHIFT_COOR=None)), KITTI_CLASSES, training=False)
    for i, frame in enumerate(FRAME_IDS):
        file_rows, in_fov = kcases.frame_points(gold, frame)
        assert 0 < in_fov.sum() < len(in_fov)
        got = crop.raw_frame(i, device=True)["points"]
        direct = crop.fov_points(crop.get_lidar(frame), crop.get_calib(frame), crop.kitti_infos[i]["image"]["image_shape"]).cpu().numpy()
        assert got.is_cuda and same_bits(got.cpu().numpy(), shifted(direct, KITTI_SHIFT)) and same_bits(direct, file_rows[in_fov])
        assert same_bits(crop.raw_frame(i)["points"].cpu().numpy(), got.cpu().numpy())    # with the crop the points are on the device either way
        got = whole.raw_frame(i, device=True)["points"]
        assert got.is_cuda and got.dtype == torch.float32 and same_bits(got.cpu().numpy(), shifted(file_rows, KITTI_SHIFT))
        host = whole.raw_frame(i)["points"]
        assert isinstance(host, np.ndarray) and same_bits(host, got.cpu().numpy())        # the fp32 addition gives the same bits on either side
        assert same_bits(unshifted.raw_frame(i, device=True)["points"].cpu().numpy(), file_rows)
        assert ("road_plane" in whole.raw_frame(i)) == (frame == "000000")
    no_points = KittiDataset(all_frames(kitti_cfg(trees[0], GET_ITEM_LIST=["gt_boxes2d"])), KITTI_CLASSES, training=False).raw_frame(0, device=True)
    assert "points" not in no_points and no_points["gt_boxes2d"].shape == (17, 4)


# ---- 2. the two domains' frames ----------------------------------------------------------------------------------------------
def test_domain_frames_rename_the_first_class_and_cut_the_boxes(trees, gold):
    ds = NusKittiMixDataset(mix_cfg(trees[0], trees[2], kitti_classes=("Car", "Pedestrian"), nus_classes=("car", "pedestrian"), joint=("car", "other")),
                            ["car", "other"], training=True)
    assert ds.on_device and len(ds) == 3 + 2 and ds.num_source == 3 and ds.num_target == 2
    assert ds.source.class_names == ["car", "pedestrian"] and ds.target.class_names == ["Car", "Pedestrian"] and ds.source.max_sweeps == 1
    tgt = ds.target_frame(1)                                                              # 000001: a Car, the Pedestrian, the lattice, DontCare
    assert list(tgt["gt_names"]) == ["car", "Pedestrian"] + ["car"] * 15 and tgt["gt_boxes"].shape == (17, 8) and tgt["gt_boxes"].dtype == np.float32
    assert tgt["gt_boxes"][:, 7].tolist() == [1.0, 2.0] + [1.0] * 15                      # the id of the domain's own list
    want = np.array([f[1] for f in kcases.FRAMES["000001"]], np.float32)
    want[:, 2] += np.float32(1.6)
    assert np.abs(tgt["gt_boxes"][:, :7] - want).max() < 0.012                            # labels carry two decimals
    plain = KittiDataset(kitti_cfg(trees[0], SHIFT_COOR=None), KITTI_CLASSES, training=True).raw_frame(1)["gt_boxes"]
    assert plain.shape == (17, 7) and np.abs(tgt["gt_boxes"][:, :7] - shifted(plain, KITTI_SHIFT)).max() < 1e-6      # SHIFT_COOR is added
    file_rows = kcases.frame_points(gold, "000001")[0]
    assert tgt["points"].is_cuda and tgt["points"].shape == (len(file_rows), 4) and same_bits(tgt["points"].cpu().numpy(), shifted(file_rows, KITTI_SHIFT))
    assert tgt["frame_id"] == "000001" and tgt["image_shape"].tolist() == [375, 1242]
    src = ds.source_frame(1)
    boxes, names = ncases.frame_boxes(1)
    keep = np.isin(names, ["car", "pedestrian"])
    assert list(src["gt_names"]) == ["car"] * 15 + ["pedestrian"] and src["gt_boxes"].shape == (16, 8) and src["gt_boxes"][:, 7].tolist() == [1.0] * 15 + [2.0]
    assert np.isnan(boxes[keep]).any() and np.isfinite(src["gt_boxes"]).all()            # the pedestrian's NaN velocity is gone with the columns
    want = boxes[keep][:, :7].copy()
    want[:, 2] += np.float32(1.8)
    assert np.abs(src["gt_boxes"][:, :7] - want).max() < 1e-6 and src["shift_coor"] == NUS_SHIFT
    assert src["points"].is_cuda and src["points"].shape == (ncases.N_KEY + 17 * ncases.N_IN_BOX, 4)
    assert same_bits(src["points"].cpu().numpy(), shifted(ncases.frame_files(1)[0][:, :4], NUS_SHIFT))


# ---- 3. a mixed sample ---------------------------------------------------------------------------------------------------------
def direct_mix(ds, source, target):
    from toda_amd.pcdet.datasets.processor.inter_domain_point_cutmix import inter_domain_point_cutmix
    from toda_amd.pcdet.datasets.processor.inter_domain_point_lasermix import inter_domain_point_lasermix
    from toda_amd.pcdet.datasets.processor.inter_domain_point_polarmix import inter_domain_point_polarmix
    r = ds.point_cloud_range
    if ds.mix_type == "cutmix":
        return inter_domain_point_cutmix(source, target, r, "center")
    if ds.mix_type == "polarmix":
        return inter_domain_point_polarmix(source, target, 1, 1.570796, 0.0, ["FIX", "FIX", "FIX"], r, "FULL", "center", False)
    return inter_domain_point_lasermix(source, target, [-20, 0], 3, 2, r, "center")


def test_an_admissible_cutmix_crop_exists(gold):
    """numpy alone: the smallest crop CutMix can draw (half the range on both sides), centred on the source point nearest the
    origin, holds more than 10 000 rows of the big target frame; every larger crop about that point holds at least those."""
    source = ncases.frame_files(1)[0]
    centre = source[np.argmin(np.abs(source[:, 0]) + np.abs(source[:, 1])), 0:2]
    half = (np.array(RANGE[3:5]) - np.array(RANGE[0:2])) * 0.5 / 2
    target = np.concatenate([kcases.frame_points(gold, "000000")[0], big_rows("000000")], 0)
    inside = ((target[:, 0:2] > centre - half) & (target[:, 0:2] < centre + half)).all(1)
    print(f"smallest crop about {centre.tolist()}: {int(inside.sum())} target rows")
    assert inside.sum() > 10000


@pytest.mark.parametrize("mix_type", ["polarmix", "cutmix", "lasermix"])
def test_mixed_sample_equals_the_processor_on_the_two_prepared_frames(trees, mix_type):
    ds = NusKittiMixDataset(mix_cfg(trees[1], trees[2], mix_type), ["car"], training=True)
    assert ds.mix_type == mix_type and ds.mix_prob == 1.0 and len(ds) == 5
    index = 4                                                                              # source frame 4 % 3 = 1, target frame 4 % 2 = 0
    np.random.seed(21)
    got = ds[index]
    np.random.seed(21)
    assert np.random.random(1) < 1.0                                                        # the draw against the probability
    source, target = ds.source_frame(1), ds.target_frame(0)
    assert source["metadata"]["token"] == "token1" and target["frame_id"] == "000000"
    want = ds.data_processor.forward(direct_mix(ds, source, target))
    assert got["points"].is_cuda and got["points"].shape[1] == 4 and same_bits(got["points"].cpu().numpy(), want["points"].cpu().numpy())
    assert got["gt_boxes"].ndim == 2 and got["gt_boxes"].shape[1] == 8 and same_bits(got["gt_boxes"], want["gt_boxes"]) and len(got["gt_boxes"]) > 0
    assert (got["gt_boxes"][:, 7] == 1).all() and "gt_names" not in got
    n_source, n_target = source["points"].shape[0], target["points"].shape[0]
    assert n_target > BIG_ROWS and min(n_source, n_target) < got["points"].shape[0] < n_source + n_target      # points of both domains


# ---- 4. the unmixed branches ---------------------------------------------------------------------------------------------------
def test_unmixed_branches_equal_the_single_datasets_frames(trees):
    ds = NusKittiMixDataset(mix_cfg(trees[0], trees[2], POLARMIX_PROB=0.0), ["car"], training=False)
    nus = NuScenesDataset(nus_cfg(trees[2]), ["car"], training=False)
    kitti = KittiDataset(kitti_cfg(trees[0]), ["Car"], training=False)
    assert len(ds) == len(nus) + len(kitti) == 1 + 1 and not kitti.on_device
    got, want = ds[0], nus[0]                                                               # source alone
    assert got["points"].is_cuda and same_bits(got["points"].cpu().numpy(), want["points"][:, :4]) and same_bits(got["gt_boxes"], want["gt_boxes"])
    assert got["metadata"] == want["metadata"] and got["gt_boxes"].shape == (15, 8) and got["shift_coor"] == NUS_SHIFT
    got, want = ds[1], kitti[0]                                                             # target alone: index - n_nus
    assert got["points"].is_cuda and isinstance(want["points"], np.ndarray) and same_bits(got["points"].cpu().numpy(), want["points"])
    assert same_bits(got["gt_boxes"], want["gt_boxes"]) and got["gt_boxes"].shape == (17, 8) and (got["gt_boxes"][:, 7] == 1).all()
    assert got["frame_id"] == want["frame_id"] == "000002" and got["image_shape"].tolist() == [375, 1242] and "gt_names" not in got
    assert isinstance(got["calib"], calibration_kitti.Calibration)


# ---- 5. FOV_POINTS_ONLY inside the mix -----------------------------------------------------------------------------------------
def test_the_target_half_of_a_mixed_sample_is_cropped_to_the_image(trees, gold):
    """The tree's rows lie outside the tau_px / tau_depth bands of the fixture, so the device flags are numpy's on every row."""
    ds = NusKittiMixDataset(mix_cfg(trees[0], trees[2], fov=True), ["car"], training=True)
    assert ds.target.fov_points_only and ds.target.on_device
    file_rows, in_fov = kcases.frame_points(gold, "000001")
    calib = ds.target.get_calib("000001")
    assert np.array_equal(KittiDataset.get_fov_flag(calib.lidar_to_rect(file_rows[:, :3]), gold["image_shape"], calib), in_fov)
    seen, unseen = row_keys(shifted(file_rows[in_fov], KITTI_SHIFT)), row_keys(shifted(file_rows[~in_fov], KITTI_SHIFT))
    source_rows = row_keys(shifted(ncases.frame_files(1)[0][:, :4], NUS_SHIFT))
    assert len(unseen) > 100 and not (seen & unseen) and not (source_rows & (seen | unseen))
    np.random.seed(8)
    got = row_keys(ds[1]["points"].cpu().numpy())                                           # source frame 1, target frame 1; PolarMix pastes at angle 0
    assert not (got & unseen) and len(got & seen) > 0 and len(got & source_rows) > 0 and got <= (seen | source_rows)
    alone = NusKittiMixDataset(mix_cfg(trees[0], trees[2], fov=True, POLARMIX_PROB=0.0), ["car"], training=True)
    np.random.seed(8)
    rows = row_keys(alone[3 + 1]["points"].cpu().numpy())                                   # the unmixed branch crops as well
    inside = shifted(file_rows[in_fov], KITTI_SHIFT)
    inside = inside[((inside[:, :2] >= np.array(RANGE[0:2], np.float32)) & (inside[:, :2] <= np.array(RANGE[3:5], np.float32))).all(1)]
    assert rows == row_keys(inside) and len(rows) > 0                                       # the crop, then the closed x-y range mask


# ---- 6. a target frame without an object -----------------------------------------------------------------------------------------
def test_a_target_frame_without_an_object(trees):
    ds = NusKittiMixDataset(mix_cfg(trees[0], trees[2], kitti_classes=("Cyclist",)), ["car"], training=True)
    target = ds.target_frame(0)
    assert target["gt_boxes"].shape == (0, 8) and target["gt_boxes"].dtype == np.float32 and target["gt_names"].shape == (0,) and target["gt_names"].dtype.kind == "U"
    np.random.seed(5)
    got = ds[3]                                                                             # source frame 0, target frame 1
    np.random.seed(5)
    np.random.random(1)
    source = ds.source_frame(0)
    want = ds.data_processor.forward(direct_mix(ds, source, ds.target_frame(1)))
    assert same_bits(got["points"].cpu().numpy(), want["points"].cpu().numpy()) and same_bits(got["gt_boxes"], want["gt_boxes"])
    assert 0 < len(got["gt_boxes"]) <= len(source["gt_boxes"]) == 15 and (got["gt_boxes"][:, 7] == 1).all()      # source boxes only
    alone = NusKittiMixDataset(mix_cfg(trees[0], trees[2], kitti_classes=("Cyclist",), POLARMIX_PROB=0.0), ["car"], training=True)
    np.random.seed(5)
    got = alone[3 + 1]                                                                      # a target index: redrawn until a source frame comes
    assert got["frame_id"].startswith("n008") and "metadata" in got and len(got["gt_boxes"]) == 15
    kept = NusKittiMixDataset(mix_cfg(trees[0], trees[2], kitti_classes=("Cyclist",), POLARMIX_PROB=0.0), ["car"], training=False)[1]
    assert kept["frame_id"] == "000002" and kept["gt_boxes"].shape == (0, 8)                # no redraw outside training


# ---- 7. and 8. the stage-1 YAML ------------------------------------------------------------------------------------------------
def shrunk_yaml(trees):
    cfg = cfg_from_yaml_file(STAGE1, AttrDict())
    for data in (cfg.DATA_CONFIG, cfg.DATA_CONFIG_TEST):
        data.POINT_CLOUD_RANGE = RANGE
        data.DATA_PROCESSOR[2].VOXEL_SIZE = [0.1, 0.1, 0.2]
    data = cfg.DATA_CONFIG
    data.NuScenesDataset.DATA_PATH, data.NuScenesDataset.VERSION = str(trees[2]), ncases.VERSION
    data.KittiDataset.DATA_PATH = str(trees[0])
    data.KittiDataset.INFO_PATH = AttrDict({"train": ["kitti_infos_train.pkl"], "test": ["kitti_infos_val.pkl"]})
    cfg.DATA_CONFIG_TEST.DATA_PATH = str(trees[0])
    cfg.DATA_CONFIG_TEST.INFO_PATH = AttrDict({"train": ["kitti_infos_train.pkl"], "test": ["kitti_infos_trainval.pkl"]})
    cfg.MODEL.BACKBONE_2D.LAYER_NUMS = [1, 1]
    cfg.LOCAL_RANK = 0
    return cfg


def test_one_stage1_step_through_the_loader(trees):
    from toda_amd.pcdet.models import build_network, prepare_batch_on_gpu
    cfg = shrunk_yaml(trees)
    data = cfg.DATA_CONFIG
    np.random.seed(3)
    torch.manual_seed(3)
    ds, loader, _ = build_dataloader(data, cfg.CLASS_NAMES, batch_size=4, dist=False, workers=2, training=True)
    assert isinstance(ds, NusKittiMixDataset) and ds.on_device and loader.num_workers == 0 and len(ds) == 3 + 2 and ds.mix_inc_method == "corner_del"
    assert ds.mix_prob == 0.3 and not ds.target.fov_points_only and ds.target.class_names == ["Car"] and ds.class_names == ["car"]
    assert len(ds.source.data_augmentor.data_augmentor_queue) == 3 and len(ds.target.data_augmentor.data_augmentor_queue) == 3     # gt_sampling is disabled
    batch = next(iter(loader))
    assert batch["batch_size"] == 4 and batch["points"].is_cuda and batch["points"].shape[1] == 5 and torch.isfinite(batch["points"]).all()
    assert batch["gt_boxes"].ndim == 3 and batch["gt_boxes"].shape[0] == 4 and batch["gt_boxes"].shape[2] == 8 and np.isfinite(batch["gt_boxes"]).all()
    assert set(np.unique(batch["gt_boxes"][..., 7])) <= {0.0, 1.0} and float(batch["points"][:, 4].max()) <= 1.0      # one class; intensity normalised
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    assert type(net).__name__ == "SECONDNetIoU"
    prepare_batch_on_gpu(batch, net)
    ret, tb, _ = net(batch)
    loss = ret["loss"]
    assert torch.isfinite(loss), tb
    loss.backward()
    grads = [p.grad for p in net.dense_head.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads) and float(sum(g.abs().sum() for g in grads)) > 0


def test_evaluation_through_the_test_block(trees, tmp_path):
    from toda_amd.pcdet.models import build_network
    from toda_amd.tools.eval_utils import eval_utils
    cfg = shrunk_yaml(trees)
    data_cfg, names = choose_test_data(cfg)
    assert data_cfg is cfg.DATA_CONFIG_TEST and names == ["Car"]
    ds, loader, _ = build_dataloader(data_cfg, names, batch_size=3, dist=False, workers=0, training=False)
    assert isinstance(ds, KittiDataset) and ds.class_names == ["Car"] and len(ds) == 3 and ds.fov_points_only and ds.on_device and loader.num_workers == 0
    torch.manual_seed(0)
    net = build_network(cfg.MODEL, len(names), ds).cuda().eval()                           # the anchors are configured under `car`
    assert net.dense_head.class_names == ["Car"] and cfg.MODEL.DENSE_HEAD.ANCHOR_GENERATOR_CONFIG[0].class_name == "car"
    batch = next(iter(loader))
    assert batch["gt_boxes"].shape == (3, 17, 8) or batch["gt_boxes"].shape == (3, 16, 8)
    preds = []
    for boxes in batch["gt_boxes"]:
        boxes = boxes[boxes[:, 7] == 1]
        preds.append({"pred_boxes": torch.from_numpy(boxes[:, :7].copy()).cuda(), "pred_scores": torch.linspace(0.5, 0.99, len(boxes), device="cuda"),
                      "pred_labels": torch.ones(len(boxes), dtype=torch.int64, device="cuda")})
    annos = ds.generate_prediction_dicts(batch, preds, ds.class_names)
    n_easy = 0
    for anno, info in zip(annos, ds.kitti_infos):
        cars = info["annos"]["name"][:len(info["annos"]["gt_boxes_lidar"])] == "Car"
        assert len(anno["name"]) == cars.sum() and (anno["name"] == "Car").all()
        assert np.abs(anno["boxes_lidar"] - info["annos"]["gt_boxes_lidar"][cars]).max() < 1e-4                    # the +1.6 m shift undone
        n_easy += int((info["annos"]["difficulty"][:len(cars)][cars] == 0).sum())
    assert n_easy >= 41
    text, res = ds.evaluation(annos, ds.class_names, eval_metric="kitti")
    assert res["Car_bev/easy_R40"] == 100.0 and res["Car_3d/easy_R40"] == 100.0, text
    with torch.no_grad():
        ret = eval_utils.eval_one_epoch(cfg, net, loader, "0", logging.getLogger("test_nus_kitti_eval"), dist_test=False, result_dir=tmp_path / "eval")
    assert {"Car_bev/easy_R40", "Car_3d/easy_R40", "Car_3d/moderate_R40", "recall/rcnn_0.7"} <= set(ret) and (tmp_path / "eval" / "result.pkl").exists()
