"""KittiMixUpAdvDataset, host side: the labelled / pseudo-labelled partition, its errors, the sampling policy, the boxes of both kinds
of frame and the numpy form of the adversarial edit on [n, 4] rows.  No GPU."""
import pickle

import numpy as np
import pytest

from tests import kitti_dataset_cases as K
from tests import kitti_mixup_adv_cases as C
from toda_amd.pcdet.config import AttrDict
from toda_amd.pcdet.datasets import __all__ as registry
from toda_amd.pcdet.datasets.kitti.kitti_mixup_adv_dataset import KittiMixUpAdvDataset
from toda_amd.pcdet.datasets.mixup_dataset import ADV_ADD, ADV_MODIFY, ADV_REMOVE, MixUpAdvPairPolicy, subset_keys
from toda_amd.pcdet.datasets.nuscenes.nuscenes_mixup_adv_dataset import NuScenesMixUpAdvDataset


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return C.write(tmp_path_factory.mktemp("kitti_advmix"), K.load_golden())


def dataset(tree, pseudo="pseudo.pkl", **extra):
    return KittiMixUpAdvDataset(C.cfg(tree, **extra), C.CLASSES, training=True, root_path=tree, pseudo_info_path=str(tree / pseudo))


def ids(infos):
    return [i["point_cloud"]["lidar_idx"] for i in infos]


def test_registry_flags_and_the_shared_policy(tree):
    assert registry["KittiMixUpAdvDataset"] is KittiMixUpAdvDataset
    ds = dataset(tree)
    assert ds.is_pair_dataset and ds.on_device and ds.pseudo_thresh == 0.2 and ds.mixup_prob == 0.6 and ds.gt_prob == 0.3
    assert dataset(tree, PSEUDO_THRESH=0.5).pseudo_thresh == 0.5
    for name in ("draw_item", "raw_pair", "__getitem__", "draw_edits", "adversarial_boxes", "voxel_table", "adversarial_points",
                 "adversarial_points_host", "voxel_gradients_host", "collate_batch"):
        assert name not in KittiMixUpAdvDataset.__dict__ or name == "raw_pair", name            # raw_pair only wraps the shared one
        assert name not in NuScenesMixUpAdvDataset.__dict__, name
        assert getattr(NuScenesMixUpAdvDataset, name) is getattr(MixUpAdvPairPolicy, name)
    with pytest.raises(ValueError, match="pseudo_info_path"):
        KittiMixUpAdvDataset(C.cfg(tree), C.CLASSES, training=True, root_path=tree)
    with pytest.raises(NotImplementedError, match="MIXUP_TYPE"):
        dataset(tree, MIXUP_TYPE="nope")


def test_partition_of_labelled_and_pseudo_infos(tree):
    ds = dataset(tree)
    assert ids(ds.gt_infos) == ["000001"] and ids(ds.ps_infos) == ["000000", "000002"] and ids(ds.infos) == ["000001", "000000", "000002"]
    assert "annos" in ds.gt_infos[0] and all("p_score" in i and "annos" not in i for i in ds.ps_infos)
    assert len(ds) == 3 and len(ds.kitti_infos) == 3 and ds.is_gt(0) and not ds.is_gt(1)
    assert len(dataset(tree, REPEAT=5)) == 5
    C.write_split(tree, [(2, "000002"), (0, "000000")], name="other.txt")
    ds = dataset(tree, LABELLED_SPLIT_FILE="ImageSets/other.txt")
    assert ids(ds.gt_infos) == ["000002", "000000"] and ids(ds.ps_infos) == ["000001"]                # the list's order, the rest


def test_a_list_that_covers_everything_takes_the_pseudo_infos_at_the_listed_indices(tree):
    C.write_split(tree, [(2, "000002"), (0, "000000"), (1, "000001")], name="all.txt")
    ds = dataset(tree, LABELLED_SPLIT_FILE="ImageSets/all.txt")
    assert ids(ds.gt_infos) == ["000002", "000000", "000001"] and ids(ds.ps_infos) == ["000002", "000000", "000001"]
    assert all("annos" in i for i in ds.gt_infos) and all("p_score" in i for i in ds.ps_infos) and len(ds.infos) == 6


def test_mismatches_are_value_errors(tree):
    C.write_split(tree, [(1, "000002")], name="wrong_id.txt")
    with pytest.raises(ValueError, match="000002"):
        dataset(tree, LABELLED_SPLIT_FILE="ImageSets/wrong_id.txt")
    C.write_split(tree, [(7, "000001")], name="wrong_index.txt")
    with pytest.raises(ValueError, match="index 7"):
        dataset(tree, LABELLED_SPLIT_FILE="ImageSets/wrong_index.txt")
    with open(tree / "pseudo.pkl", "rb") as f:
        pseudo = pickle.load(f)
    for name, bad in (("short.pkl", pseudo[:2]), ("order.pkl", [pseudo[1], pseudo[0], pseudo[2]])):
        with open(tree / name, "wb") as f:
            pickle.dump(bad, f)
        with pytest.raises(ValueError, match="pseudo-label infos"):
            dataset(tree, pseudo=name)
    with pytest.raises(FileNotFoundError):
        dataset(tree, pseudo="absent.pkl")
    with pytest.raises(FileNotFoundError, match="labelled split file"):
        dataset(tree, LABELLED_SPLIT_FILE="ImageSets/absent.txt")


def test_draw_item_under_a_seeded_rng(tree):
    ds = dataset(tree)                                                    # 1 labelled, 2 pseudo-labelled; MIXUP_PROB 0.6, GT_PROB 0.3
    n_gt, n = 1, 3
    for seed in range(12):
        rs = np.random.RandomState(seed)
        if rs.random_sample(1) > 0.6:
            want = ("same", 4 % n_gt) if rs.random_sample(1) < 0.3 else ("same", n_gt + 4 % 2)
        else:
            want = ("mixup", int(rs.randint(n)), int(rs.randint(n)))
        np.random.seed(seed)
        assert ds.draw_item(4) == want, seed
    kinds = set()
    for seed in range(12):
        np.random.seed(seed)
        kinds.add(ds.draw_item(4)[0])
    assert kinds == {"same", "mixup"}
    np.random.seed(0)
    assert dataset(tree, MIXUP_PROB=0.0, GT_PROB=0.0).draw_item(3) == ("same", 1 + 3 % 2)
    assert dataset(tree, MIXUP_PROB=0.0, GT_PROB=1.0).draw_item(3) == ("same", 0)
    assert dataset(tree, MIXUP_TYPE="no_mixup").draw_item(3) == ("same", 0)
    k1, k2 = dataset(tree, MIXUP_PROB=1.0, MIXUP_TYPE="ps_gt").draw_item(0)[1:]
    assert k1 >= 1 and k2 == 0


def test_boxes_of_labelled_and_pseudo_frames_carry_the_shift(tree):
    ds = dataset(tree)
    shift = np.array(C.SHIFT, np.float32)
    boxes, names = ds.frame_boxes(ds.infos[0])                            # labelled 000001: its annotations without DontCare
    want = np.array([f[1] for f in K.FRAMES["000001"]], np.float32)
    want[:, :3] += shift
    assert boxes.dtype == np.float32 and boxes.shape == want.shape and list(names) == [f[0] for f in K.FRAMES["000001"]]
    assert np.abs(boxes - want).max() < 0.02                              # the label file keeps two decimals
    stored = ds.infos[0]["annos"]["gt_boxes_lidar"].astype(np.float32)
    stored[:, :3] += shift
    assert np.abs(boxes - stored).max() < 1e-4
    info = ds.infos[1]                                                    # pseudo-labelled 000000: every box, whatever its score
    boxes, names = ds.frame_boxes(info)
    assert (info["p_score"] < 0.2).any() and len(boxes) == len(info["gt_boxes"]) == len(K.FRAMES["000000"]) + 1
    want = info["gt_boxes"].copy()
    want[:, :3] += shift
    assert np.array_equal(boxes, want) and set(names) == {"Car"}
    visited = ds.adversarial_boxes(info)                                  # the edit: p_score > 0.2
    assert len(visited) == int((info["p_score"] > 0.2).sum()) < len(boxes) and np.array_equal(visited, want[info["p_score"] > 0.2])
    assert np.array_equal(ds.infos[1]["gt_boxes"][:, 2] + shift[2], want[:, 2])                       # the infos are left alone


def test_adversarial_points_host_on_four_columns(tree):
    ds = dataset(tree)
    info = ds.infos[1]
    pts = ds.get_lidar("000000")
    pts[:, :3] += np.array(C.SHIFT, np.float32)
    assert pts.shape[1] == 4
    n, k = len(pts), len(ds.adversarial_boxes(info))
    known = np.arange(n - K.N_KNOWN, n)                                   # the rows inside pseudo box 0; the scene around it is cleared
    step = np.float32(ds.adv_eps) * C.GRAD
    assert np.array_equal(ds.voxel_gradients_host(pts[known, :3], info), np.tile(C.GRAD, (K.N_KNOWN, 1)))

    def draws(op, frac):
        d = {"op": np.full(k, 3, np.int64), "frac": np.zeros(k), "seed": np.full(k, 12345, np.uint32)}
        d["op"][0], d["frac"][0] = op, frac
        return d
    out = ds.adversarial_points_host(pts.copy(), info, draws(ADV_MODIFY, 0.0))
    assert out.shape == pts.shape and np.array_equal(out[:n - K.N_KNOWN], pts[:n - K.N_KNOWN])
    assert np.array_equal(out[known, :3], pts[known, :3] - step) and np.array_equal(out[known, 3], pts[known, 3])
    out = ds.adversarial_points_host(pts.copy(), info, draws(ADV_ADD, 0.0))
    assert out.shape == (n + K.N_KNOWN, 4) and np.array_equal(out[:n], pts)
    assert np.array_equal(out[n:, :3], pts[known, :3] - step) and np.array_equal(out[n:, 3], pts[known, 3])
    out = ds.adversarial_points_host(pts.copy(), info, draws(ADV_REMOVE, 0.0))
    assert np.array_equal(out, pts[:n - K.N_KNOWN])
    out = ds.adversarial_points_host(pts.copy(), info, draws(ADV_MODIFY, 0.5))                        # k = 5 stay: the 5 smallest keys move
    moved = np.flatnonzero((out[:, :3] != pts[:, :3]).any(1))
    want = np.sort(known[np.argsort(subset_keys(12345, known), kind="stable")[:5]])
    assert np.array_equal(moved, want) and np.array_equal(out[moved, :3], pts[moved, :3] - step)
    assert ds.adversarial_points_host(pts, ds.infos[0], draws(ADV_MODIFY, 0.0)) is pts                # a labelled info: nothing to do


def test_gt_sampling_is_refused_at_construction(tree):
    aug = {"DISABLE_AUG_LIST": ["placeholder"],
           "AUG_CONFIG_LIST": [{"NAME": "gt_sampling", "DB_INFO_PATH": ["kitti_dbinfos_train.pkl"], "SAMPLE_GROUPS": ["Car:2"], "NUM_POINT_FEATURES": 4,
                                "PREPARE": {"filter_by_min_points": ["Car:5"]}, "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": True},
                               {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x", "y"]}]}
    with pytest.raises(NotImplementedError, match="gt_sampling"):
        dataset(tree, DATA_AUGMENTOR=AttrDict(aug))
    aug["DISABLE_AUG_LIST"] = ["placeholder", "gt_sampling"]
    ds = dataset(tree, DATA_AUGMENTOR=AttrDict(aug))
    assert len(ds.data_augmentor.data_augmentor_queue) == 1


def test_the_shipped_config(tree):
    import os

    from toda_amd.pcdet.config import cfg_from_yaml_file
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = cfg_from_yaml_file(os.path.join(root, "toda_amd/tools/cfgs/models/toda_stage2_kitti_advmix_real.yaml"), AttrDict())
    data = cfg.DATA_CONFIG
    assert data.DATASET == "KittiMixUpAdvDataset" and list(data.POINT_CLOUD_RANGE) == [-76.2, -76.2, -3.0, 76.2, 76.2, 5.0]
    assert list(data.SHIFT_COOR) == [0.0, 0.0, 1.6] and data.FOV_POINTS_ONLY and "PSEUDO_THRESH" not in data
    assert (data.MIXUP_PROB, data.GT_PROB, data.MIXUP_TYPE, data.ALPHA, data.ADV_EPS) == (0.6, 0.3, "gt+ps_gt+ps", 2, 0.001)
    assert "gt_sampling" in data.DATA_AUGMENTOR.DISABLE_AUG_LIST
    assert cfg.MODEL.NAME == "SECONDNetIoU" and cfg.MODEL.ROI_HEAD.NAME == "SECONDHead" and cfg.OPTIMIZATION.LR == 0.003
    data.DATA_PATH, data.INFO_PATH = str(tree), {"train": [C.INFOS], "test": [C.INFOS]}
    ds = KittiMixUpAdvDataset(data, cfg.CLASS_NAMES, training=True, root_path=tree, pseudo_info_path=str(tree / "pseudo.pkl"))
    assert ds.pseudo_thresh == 0.2 and len(ds.gt_infos) == 1 and len(ds.ps_infos) == 2
    assert [type(s).__name__ for s in ds.data_augmentor.data_augmentor_queue] == ["partial"] * 3
