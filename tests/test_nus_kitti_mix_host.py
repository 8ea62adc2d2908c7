"""NusKittiMixDataset, the DATA_CONFIG_TEST choice of tools.test and tools.make_labelled_subset, host side: the registry and the
stage-1 YAML, the index policy of the two-domain dataset with its frame sources stubbed, the preparation of a target frame
without an object, and the labelled-subset files on a fake list of 250 KITTI infos.  No GPU."""
import os
import pickle
import re
import types

import numpy as np
import pytest
import torch

from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
from toda_amd.pcdet.datasets import __all__ as registry
from toda_amd.pcdet.datasets.kitti.kitti_mixup_adv_dataset import read_labelled_split
from toda_amd.pcdet.datasets.two_dataset import NusKittiMixDataset, TwoDomainMixDataset, WaymoNusMixDataset
from toda_amd.tools import make_labelled_subset as subset
from toda_amd.tools.test import test_data_config as choose_test_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE1 = os.path.join(ROOT, "toda_amd/tools/cfgs/models/toda_stage1_nus_kitti_polarmix_real.yaml")
KITTI_YAML = os.path.join(ROOT, "toda_amd/tools/cfgs/dataset_configs/kitti_dataset.yaml")


# ---- registry, YAML, the test block ------------------------------------------------------------------------------------------
def test_three_registry_names_are_one_class():
    assert all(registry[n] is NusKittiMixDataset for n in ("NusKittiMixDataset", "NusKittiPolarMixDataset", "NusKittiCutMixDataset"))
    assert issubclass(NusKittiMixDataset, TwoDomainMixDataset) and issubclass(WaymoNusMixDataset, TwoDomainMixDataset)
    assert NusKittiMixDataset.on_device is True
    for name in ("__getitem__", "__len__", "_prepare_domain", "num_source"):              # one definition, in the base
        assert name not in vars(NusKittiMixDataset) and name not in vars(WaymoNusMixDataset), name


def test_stage1_yaml_names_the_dataset_and_carries_a_test_block():
    cfg = cfg_from_yaml_file(STAGE1, AttrDict())
    mix = cfg.DATA_CONFIG
    assert registry[mix.DATASET] is NusKittiMixDataset and cfg.CLASS_NAMES == mix.CLASS_NAMES == ["car"]
    assert mix.MIX_TYPE == "polarmix" and mix.MIX_INC_METHOD == "corner_del" and mix.POLARMIX_PROB == 0.3 and mix.POLARMIX_DEGREE == 1.570796
    assert mix.POINT_CLOUD_RANGE == [-76.2, -76.2, -3.0, 76.2, 76.2, 5.0] and mix.DATA_PROCESSOR[2].VOXEL_SIZE == [0.075, 0.075, 0.2]
    assert mix.POINT_FEATURE_ENCODING.src_feature_list == ["x", "y", "z", "intensity", "timestamp"]
    nus, kitti = mix.NuScenesDataset, mix.KittiDataset
    assert nus.DATASET == "NuScenesDataset" and nus.MAX_SWEEPS == 1 and nus.SHIFT_COOR == [0.0, 0.0, 1.8] and nus.CLASS_NAMES == ["car"]
    assert kitti.DATASET == "KittiDataset" and kitti.CLASS_NAMES == ["Car"] and kitti.SHIFT_COOR == [0.0, 0.0, 1.6] and kitti.FOV_POINTS_ONLY is False
    assert kitti.INFO_PATH.train == ["top_1_percent_frames_kitti_infos_train.pkl"] and kitti.GET_ITEM_LIST == ["points"]
    assert "gt_sampling" in nus.DATA_AUGMENTOR.DISABLE_AUG_LIST and "gt_sampling" in kitti.DATA_AUGMENTOR.DISABLE_AUG_LIST
    assert cfg.MODEL.NAME == "SECONDNetIoU" and cfg.MODEL.POST_PROCESSING.EVAL_METRIC == "kitti"
    assert cfg.MODEL.DENSE_HEAD.ANCHOR_GENERATOR_CONFIG[0].class_name == "car"
    test = cfg.DATA_CONFIG_TEST
    assert test.DATASET == "KittiDataset" and test.CLASS_NAMES == ["Car"] and test.FOV_POINTS_ONLY is True and test.SHIFT_COOR == [0.0, 0.0, 1.6]
    assert test.INFO_PATH.test == ["kitti_infos_val.pkl"] and test.DATA_SPLIT.test == "val" and "DATA_PATH" in test
    assert test.POINT_CLOUD_RANGE == mix.POINT_CLOUD_RANGE and test.DATA_PROCESSOR[2].VOXEL_SIZE == mix.DATA_PROCESSOR[2].VOXEL_SIZE


def test_the_test_block_is_chosen_when_present():
    cfg = cfg_from_yaml_file(STAGE1, AttrDict())
    data, names = choose_test_data(cfg)
    assert data is cfg.DATA_CONFIG_TEST and names == ["Car"]
    cfg.pop("DATA_CONFIG_TEST")
    data, names = choose_test_data(cfg)
    assert data is cfg.DATA_CONFIG and names == ["car"]
    waymo_nus = cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/models/toda_stage1_waymo_nus_polarmix_real.yaml"), AttrDict())
    data, names = choose_test_data(waymo_nus)
    assert data.DATASET == "NuScenesDataset" and names == ["car"] and data.MAX_SWEEPS == 1 and data.SHIFT_COOR == [0.0, 0.0, 1.8]
    plain = cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/models/centerpoint_waymo_real.yaml"), AttrDict())
    data, names = choose_test_data(plain)
    assert data is plain.DATA_CONFIG and names == plain.CLASS_NAMES


# ---- the index policy, frame sources stubbed ---------------------------------------------------------------------------------
class _Nus:
    def __init__(self, n):
        self.infos = list(range(n))


class _Kitti:
    def __init__(self, n):
        self.kitti_infos = list(range(n))


class _Identity:
    def forward(self, data):
        return data


def stub_mix(n_nus, n_kitti, prob, training=True, boxes_after_mix=None):
    ds = NusKittiMixDataset.__new__(NusKittiMixDataset)
    ds.source, ds.target, ds.mix_prob, ds.training = _Nus(n_nus), _Kitti(n_kitti), prob, training
    ds._merge_all_iters_to_one_epoch, ds.total_epochs, ds.data_processor = False, 0, _Identity()
    ds.source_frame = lambda i: {"from": ("source", i), "gt_boxes": np.ones((2, 8), np.float32), "gt_names": np.array(["car", "car"])}
    ds.target_frame = lambda i: {"from": ("target", i), "gt_boxes": np.ones((3, 8), np.float32), "gt_names": np.array(["car"] * 3)}
    ds.mix = lambda s, t: {"from": ("mix", s["from"][1], t["from"][1]), "gt_boxes": np.ones((5, 8), np.float32) if boxes_after_mix is None else boxes_after_mix}
    return ds


def test_length_and_unmixed_branches():
    ds = stub_mix(5, 3, prob=0.0)
    assert len(ds) == 8 and ds.num_source == 5 and ds.num_target == 3
    assert [ds[i]["from"] for i in range(8)] == [("source", i) for i in range(5)] + [("target", i) for i in range(3)]      # index - n_nus
    assert all("gt_names" not in ds[i] for i in range(8))
    ds.merge_all_iters_to_one_epoch(merge=True, epochs=4)
    assert len(ds) == 32
    assert ds[8]["from"] == ("source", 0) and ds[8 + 6]["from"] == ("target", 1) and ds[31]["from"] == ("target", 2)      # the modulo of the length


def test_mixed_index_pairs_both_lists_by_modulo():
    ds = stub_mix(5, 3, prob=1.0)
    assert [ds[i]["from"] for i in range(8)] == [("mix", i % 5, i % 3) for i in range(8)]
    ds.merge_all_iters_to_one_epoch(merge=True, epochs=2)
    assert ds[13]["from"] == ("mix", 0, 2)                                               # 13 % 8 = 5


def test_one_draw_against_the_probability():
    ds = stub_mix(4, 4, prob=0.3)
    np.random.seed(5)
    draws = np.random.random(40)
    np.random.seed(5)
    got = [ds[i % 8]["from"][0] for i in range(40)]
    assert got == ["mix" if d < 0.3 else ("source" if i % 8 < 4 else "target") for i, d in enumerate(draws)]
    assert set(got) == {"mix", "source", "target"}


def test_both_redraws():
    calls = []
    ds = stub_mix(2, 2, prob=1.0, boxes_after_mix=np.ones((8,), np.float32))             # a mix whose boxes are not 2-D
    real = ds.mix

    def mix_once_bad(s, t):
        calls.append((s["from"][1], t["from"][1]))
        return real(s, t) if len(calls) == 1 else {"from": "second", "gt_boxes": np.ones((1, 8), np.float32)}
    ds.mix = mix_once_bad
    np.random.seed(0)
    np.random.random(1)                          # the draw against the probability (1.0: always mixed) ...
    want = int(np.random.randint(4))             # ... then the redraw's index, randint(len)
    np.random.seed(0)
    assert ds[1]["from"] == "second" and calls == [(1, 1), (want % 2, want % 2)]
    empty = stub_mix(2, 2, prob=0.0)                                                     # a target frame without a box, alone
    seen = []
    empty.target_frame = lambda i: seen.append(i) or {"from": ("target", i), "gt_boxes": np.zeros((0, 8), np.float32), "gt_names": np.zeros(0, dtype=str)}
    np.random.seed(0)
    assert empty[3]["from"][0] == "source" and seen[0] == 1                              # re-drawn until a source frame (2 boxes) came
    empty.training = False
    got = empty[3]
    assert got["from"] == ("target", 1) and got["gt_boxes"].shape == (0, 8)              # no re-draw outside training


def test_a_target_frame_without_an_object_leaves_with_empty_boxes(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)               # no device here: the upload is not what is checked
    ds = NusKittiMixDataset.__new__(NusKittiMixDataset)
    ds.training, ds.class_names, ds.point_feature_encoder = True, ["car"], _Identity()
    domain = types.SimpleNamespace(class_names=["Cyclist"], data_augmentor=None)
    frame = {"points": np.zeros((7, 4), np.float32), "gt_boxes": np.ones((3, 7), np.float32), "gt_names": np.array(["Car", "Pedestrian", "Car"]), "frame_id": "000003"}
    out = ds._prepare_domain(domain, dict(frame))
    assert out["gt_boxes"].shape == (0, 8) and out["gt_boxes"].dtype == np.float32
    assert out["gt_names"].shape == (0,) and out["gt_names"].dtype.kind == "U" and torch.is_tensor(out["points"])
    none = ds._prepare_domain(domain, {**frame, "gt_boxes": np.zeros((0, 7), np.float32), "gt_names": np.array([])})      # a label file of DontCare only
    assert none["gt_boxes"].shape == (0, 8) and none["gt_boxes"].dtype == np.float32 and none["gt_names"].dtype.kind == "U"
    source = {"gt_boxes": np.ones((2, 8), np.float32)}
    assert np.concatenate([source["gt_boxes"], out["gt_boxes"]], 0).shape == (2, 8)      # what the mixes do with the two box lists
    domain.class_names = ["Car", "Pedestrian"]
    kept = ds._prepare_domain(domain, dict(frame))
    assert list(kept["gt_names"]) == ["car", "Pedestrian", "car"] and kept["gt_boxes"][:, 7].tolist() == [1.0, 2.0, 1.0]


# ---- make_labelled_subset ----------------------------------------------------------------------------------------------------
N_FAKE = 250


@pytest.fixture()
def fake_kitti(tmp_path):
    """250 infos whose frame ids are not their indices (the train split of KITTI skips the val frames)."""
    infos = [{"point_cloud": {"num_features": 4, "lidar_idx": f"{3 * i + 1:06d}"}, "annos": {"name": np.array(["Car"] * (i % 3))}} for i in range(N_FAKE)]
    with open(tmp_path / "kitti_infos_train.pkl", "wb") as f:
        pickle.dump(infos, f)
    return tmp_path, infos


def run_kitti(root, *extra):
    return subset.main(["kitti", KITTI_YAML, "--data_path", str(root), *extra])


def read_pickle(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def test_one_percent_of_250_frames(fake_kitti):
    root, infos = fake_kitti
    split_file, pkl = run_kitti(root, "--percent", "1", "--seed", "1")
    assert split_file == root / "ImageSets" / "train_0.01_1.txt" and pkl == root / "top_1_percent_frames_kitti_infos_train.pkl"
    lines = split_file.read_text().splitlines()
    assert len(lines) == 2 == round(2.5)
    assert all(re.match(r"^\d{6} \d+$", line) for line in lines)
    indices = [int(line.split()[1]) for line in lines]
    assert indices == sorted(np.random.default_rng(1).choice(N_FAKE, 2, replace=False).tolist()) and indices[0] < indices[1]
    assert all(infos[i]["point_cloud"]["lidar_idx"] == line.split()[0] for i, line in zip(indices, lines))
    kept = read_pickle(pkl)
    assert [k["point_cloud"]["lidar_idx"] for k in kept] == [infos[i]["point_cloud"]["lidar_idx"] for i in indices]      # ascending index order
    assert all(np.array_equal(k["annos"]["name"], infos[i]["annos"]["name"]) for k, i in zip(kept, indices))
    assert read_labelled_split(split_file, infos) == indices                             # the check KittiMixUpAdvDataset.include_kitti_data makes


def test_the_seed_decides_the_draw(fake_kitti):
    root, _ = fake_kitti
    first = run_kitti(root, "--percent", "4", "--seed", "7")[0].read_text()
    kept = pickle.dumps(read_pickle(root / "top_4_percent_frames_kitti_infos_train.pkl"))
    again = run_kitti(root, "--percent", "4", "--seed", "7")
    assert again[0].name == "train_0.04_7.txt" and again[0].read_text() == first and pickle.dumps(read_pickle(again[1])) == kept
    other = run_kitti(root, "--percent", "4", "--seed", "8")[0]
    assert other.name == "train_0.04_8.txt" and len(first.splitlines()) == len(other.read_text().splitlines()) == 10
    assert [l.split()[1] for l in other.read_text().splitlines()] != [l.split()[1] for l in first.splitlines()]


def test_select_first_and_the_smallest_subset(fake_kitti):
    root, infos = fake_kitti
    split_file, pkl = run_kitti(root, "--percent", "1", "--select", "first")
    assert split_file.read_text() == "000001 0\n000004 1\n" and [k["point_cloud"]["lidar_idx"] for k in read_pickle(pkl)] == ["000001", "000004"]
    assert subset.draw_indices(250, 0.01, 1, "first") == [0] and len(subset.draw_indices(250, 0.01, 3)) == 1      # max(1, round(0.025))
    assert subset.draw_indices(3, 100, 1) == [0, 1, 2]


def test_listing_builds_the_pickle_and_refuses_a_wrong_index(fake_kitti, tmp_path):
    root, infos = fake_kitti
    listing = tmp_path / "authors.txt"
    listing.write_text("000022 7\n000004 1\n\n")
    split_file, pkl = run_kitti(root, "--percent", "1", "--listing", str(listing))
    assert split_file == listing and not (root / "ImageSets").exists()                   # no draw, no split file written
    assert [k["point_cloud"]["lidar_idx"] for k in read_pickle(pkl)] == ["000004", "000022"]
    listing.write_text("000022 7\n000004 2\n")
    with pytest.raises(ValueError, match="000004 2"):
        run_kitti(root, "--percent", "1", "--listing", str(listing))
    listing.write_text("000022 250\n")
    with pytest.raises(ValueError, match="no such info"):
        run_kitti(root, "--percent", "1", "--listing", str(listing))


def test_nuscenes_subset(tmp_path):
    version = tmp_path / "v1.0-mini"
    version.mkdir()
    infos = [{"token": f"t{i}", "lidar_path": f"samples/LIDAR_TOP/{i}.pcd.bin"} for i in range(N_FAKE)]
    with open(version / "nuscenes_infos_10sweeps_train.pkl", "wb") as f:
        pickle.dump(infos, f)
    yaml = os.path.join(ROOT, "toda_amd/tools/cfgs/dataset_configs/nuscenes_dataset.yaml")
    pkl = subset.main(["nuscenes", yaml, "--data_path", str(tmp_path), "--version", "v1.0-mini", "--percent", "1", "--seed", "1"])
    assert pkl == version / "top_1_percent_frames_nuscenes_infos_10sweeps_train.pkl"
    want = sorted(np.random.default_rng(1).choice(N_FAKE, 2, replace=False).tolist())
    assert [k["token"] for k in read_pickle(pkl)] == [f"t{i}" for i in want]
