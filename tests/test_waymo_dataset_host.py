"""WaymoDataset and WaymoNusMixDataset, host side: the numpy frame route, the info list, the sampled frames and the prediction
dicts against the reference's outputs in tests/golden/waymo_dataset.npz (capture_waymo_dataset.py), the file-level behaviour on
a mini Waymo tree, and the index policy of the two-domain dataset with its frame sources stubbed.  No GPU.

x, y, z, the elongation and the kept rows are compared with the fixture bit for bit.  The intensity of the numpy route is numpy's
fp32 tanh, an approximation that belongs to the numpy build: it is compared bit for bit with np.tanh taken here on the same
column, and with the fixture within `tanh_ulp_ref`, the distance the capture measured between that routine and the correctly
rounded value."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import waymo_dataset_cases as cases
from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
from toda_amd.pcdet.datasets import __all__ as registry
from toda_amd.pcdet.datasets.two_dataset import WaymoNusMixDataset
from toda_amd.pcdet.datasets.waymo import waymo_dataset
from toda_amd.pcdet.datasets.waymo.waymo_dataset import WaymoDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = [-200.0, -200.0, -10.0, 200.0, 200.0, 10.0]


@pytest.fixture(scope="module")
def gold():
    return cases.load_golden()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return cases.write_tree(tmp_path_factory.mktemp("waymo"))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def golden_dataset(tmp_path, gold, training=False, **extra):
    if not (tmp_path / "ImageSets").exists():
        cases.write_golden_tree(tmp_path, gold)
    return WaymoDataset(cases.dataset_cfg(tmp_path, POINT_CLOUD_RANGE=WIDE, **extra), cases.CLASSES, training=training)


# ---- the numpy route against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,disable", [("nlz", False), ("all", True)])
def test_numpy_route_equals_the_reference(tmp_path, gold, tag, disable):
    ds = golden_dataset(tmp_path, gold, DISABLE_NLZ_FLAG_ON_POINTS=disable)
    assert ds.use_nlz is (not disable) and ds.on_device
    ulp_ref = int(gold["tanh_ulp_ref"])
    for k in range(2):
        got, want, rows = ds.get_lidar_host(str(gold["sequence"]), k), gold[f"points_{tag}_{k}"], gold[f"frame{k}"]
        assert got.dtype == np.float32 and got.shape == want.shape
        assert same_bits(got[:, [0, 1, 2, 4]], want[:, [0, 1, 2, 4]])                       # the same rows in the same order (column 4 is a row id)
        kept = rows[:, 0:5] if disable else rows[:, 0:5][rows[:, 5] == -1]
        assert len(kept) == len(got) and (disable or 0 < len(got) < len(rows))
        assert same_bits(got[:, 3], np.tanh(kept[:, 3]))
        distance = cases.ulp_distance(got[:, 3], want[:, 3])
        print(f"{tag} frame {k}: intensity at most {int(distance.max())} ulp from the fixture, tanh_ulp_ref {ulp_ref}")
        assert distance.max() <= ulp_ref
    assert np.array_equal(np.load(tmp_path / cases.TAG / str(gold["sequence"]) / "0000.npy"), gold["frame0"])     # the file was not written to


def test_the_fixture_is_what_its_capture_says(gold):
    for k in range(2):
        rows = gold[f"frame{k}"]
        assert rows.dtype == np.float32 and rows.shape[1] == 6 and set(np.unique(rows[:, 5]).tolist()) == {-1.0, 0.0, 1.0}
        assert cases.tanh_tie_free(rows[:, 3]).all()
    worst = max(int(cases.ulp_distance(gold[f"points_all_{k}"][:, 3], cases.tanh_fp64(gold[f"frame{k}"][:, 3])).max()) for k in range(2))
    assert worst == int(gold["tanh_ulp_ref"]) <= 2
    edge = gold["frame1"][:10, 3]
    assert np.signbit(edge[1]) and not np.signbit(edge[0]) and 0 < edge[2] < np.finfo(np.float32).tiny
    out = gold["points_all_1"][:10, 3]
    assert np.signbit(out[1]) and out[1] == 0 and out[3] < 1 and out[5] == 1 and out[6] < 0
    exact = cases.tanh_fp64(edge)
    assert exact[3] == np.nextafter(np.float32(1), np.float32(0)) and exact[4] == 1 and exact[2] == edge[2]      # 9.0 and 9.1: either side of fp32 saturation


def test_tie_filter_passes_the_special_values_and_holds_for_the_random_inputs():
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 100.0, -100.0, 1e-40], np.float32)
    assert cases.tanh_tie_free(special).all()
    rng = np.random.default_rng(3)
    x = np.exp(rng.normal(-1.5, 1.5, 200_000)).astype(np.float32)
    ok = cases.tanh_tie_free(x)
    assert 0.999 < ok.mean() <= 1.0                                                      # 2^-40 against a spacing of 2^-24: next to nothing is refused
    assert cases.tanh_tie_free(cases.random_intensity(rng, 1000)).all() and cases.tanh_tie_free(cases.random_frame(rng, 500)[:, 3]).all()


# ---- the info list ---------------------------------------------------------------------------------------------------------
def test_sequence_name_fallbacks(tmp_path):
    check = WaymoDataset.check_sequence_name_with_all_version
    plain = tmp_path / "segment-77_with_camera_labels" / "segment-77_with_camera_labels.pkl"
    assert check(plain) == plain                                                         # a miss returns the argument
    for made in ("training_segment-77_with_camera_labels/training_segment-77_with_camera_labels.pkl",
                 "validation_segment-77_with_camera_labels/validation_segment-77_with_camera_labels.pkl",
                 "testing_segment-77_with_camera_labels/testing_segment-77_with_camera_labels.pkl", "segment-77/segment-77.pkl"):
        path = tmp_path / made
        path.parent.mkdir()
        path.write_bytes(b"")
        assert check(plain) == path, made
        path.unlink()
        path.parent.rmdir()
    plain.parent.mkdir()
    plain.write_bytes(b"")
    (tmp_path / "segment-77").mkdir()
    (tmp_path / "segment-77" / "segment-77.pkl").write_bytes(b"")
    assert check(plain) == plain                                                         # the listed name wins


def test_missing_sequences_are_skipped_and_counted(tree):
    ds = WaymoDataset(cases.dataset_cfg(tree), cases.CLASSES, training=True)
    assert ds.split == "train" and len(ds.sample_sequence_list) == 3 and ds.num_skipped_infos == 1
    assert [i["frame_id"] for i in ds.infos] == [f"{s}_{k:03d}" for s in cases.SEQUENCES for k in range(cases.FRAMES_PER_SEQUENCE)]
    val = WaymoDataset(cases.dataset_cfg(tree), cases.CLASSES, training=False)
    assert val.split == "val" and val.num_skipped_infos == 0 and len(val) == cases.FRAMES_PER_SEQUENCE
    assert all(i["point_cloud"]["lidar_sequence"] == cases.SEQUENCES[1] for i in val.infos)


def test_a_sequence_under_another_releases_name_is_found(tmp_path):
    cases.write_tree(tmp_path)
    old = tmp_path / cases.TAG / cases.SEQUENCES[0]
    new_name = cases.SEQUENCES[0].replace("segment", "training_segment")
    old.rename(tmp_path / cases.TAG / new_name)
    (tmp_path / cases.TAG / new_name / f"{cases.SEQUENCES[0]}.pkl").rename(tmp_path / cases.TAG / new_name / f"{new_name}.pkl")
    ds = WaymoDataset(cases.dataset_cfg(tmp_path), cases.CLASSES, training=True)
    assert ds.num_skipped_infos == 1 and len(ds) == 2 * cases.FRAMES_PER_SEQUENCE


@pytest.mark.parametrize("interval", [1, 2, 3])
def test_sampled_interval_equals_the_reference(tmp_path, gold, interval):
    ds = golden_dataset(tmp_path, gold, training=True, SAMPLED_INTERVAL={"train": interval, "test": 1})
    assert [i["frame_id"] for i in ds.infos] == [str(f) for f in gold[f"frame_ids_interval_{interval}"]]
    assert len(ds) == len(range(0, int(gold["n_infos"]), interval))
    ds.merge_all_iters_to_one_epoch(merge=True, epochs=5)
    assert len(ds) == 5 * len(ds.infos)


def test_set_split_reads_the_other_list(tree):
    ds = WaymoDataset(cases.dataset_cfg(tree), cases.CLASSES, training=True)
    assert len(ds) == 8
    ds.set_split("val")
    assert ds.split == "val" and len(ds) == 4 and ds.sample_sequence_list == [cases.SEQUENCES[1] + ".tfrecord"] and ds.num_skipped_infos == 0
    ds.set_split("train")
    assert len(ds) == 8 and ds.num_skipped_infos == 1


def test_other_channel_names_the_directory_of_the_frames(tmp_path):
    cases.write_tree(tmp_path, other_channel="modes/16^")
    assert not (tmp_path / cases.TAG / cases.SEQUENCES[0] / "0000.npy").exists()
    ds = WaymoDataset(cases.dataset_cfg(tmp_path, OTHER_CHANNEL="modes/16^"), cases.CLASSES, training=True)
    assert ds.frame_path == tmp_path / "modes/16^" and ds.data_path == tmp_path / cases.TAG and len(ds) == 8
    got = ds.get_lidar_host(cases.SEQUENCES[1], 2)
    assert same_bits(got, cases.host_route(cases.frame_rows(cases.FRAMES_PER_SEQUENCE + 2)))
    plain = WaymoDataset(cases.dataset_cfg(tmp_path), cases.CLASSES, training=True)
    with pytest.raises(FileNotFoundError):
        plain.get_lidar_host(cases.SEQUENCES[1], 2)


@pytest.mark.parametrize("bad", [np.zeros((7, 5), np.float32), np.zeros((7, 6), np.float64), np.zeros(42, np.float32), np.zeros((2, 3, 6), np.float32)])
def test_a_malformed_frame_file_raises_with_its_path(tmp_path, gold, bad):
    ds = golden_dataset(tmp_path, gold)
    path = tmp_path / cases.TAG / str(gold["sequence"]) / "0001.npy"
    np.save(str(path), bad)
    for read in (ds.get_lidar_host, ds.read_frame):
        with pytest.raises(ValueError) as err:
            read(str(gold["sequence"]), 1)
        assert str(path) in str(err.value)


# ---- samples and predictions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,training", [("train", True), ("test", False)])
def test_raw_frame_equals_the_references_getitem_input(tmp_path, gold, tag, training):
    ds = golden_dataset(tmp_path, gold, training=training)
    frame = ds.raw_frame(0, host=True)
    assert list(frame["gt_names"]) == [str(n) for n in gold[f"item_{tag}_names"]] and same_bits(frame["gt_boxes"], gold[f"item_{tag}_boxes"])
    assert "unknown" not in frame["gt_names"] and frame["metadata"] == frame["frame_id"] == f"{gold['sequence']}_000"
    assert (frame["num_points_in_gt"] > 0).all() == training and len(frame["num_points_in_gt"]) == len(frame["gt_names"])
    assert same_bits(frame["points"][:, [0, 1, 2, 4]], gold["points_nlz_0"][:, [0, 1, 2, 4]])
    assert "gt_boxes" not in ds.raw_frame(1, host=True)                                  # a frame without annotations
    assert len(ds.infos[0]["annos"]["name"]) == len(gold["anno_name"])                   # the info list keeps every object


def test_fakelidar_boxes_are_converted(tmp_path, gold):
    frame = golden_dataset(tmp_path, gold, INFO_WITH_FAKELIDAR=True).raw_frame(0, host=True)
    old = gold["anno_boxes"][gold["anno_name"] != "unknown"]
    want = np.concatenate([old[:, 0:2], old[:, 2:3] + old[:, 5:6] / 2, old[:, 4:5], old[:, 3:4], old[:, 5:6], -(old[:, 6:7] + np.pi / 2)], 1)
    assert frame["gt_boxes"].shape == (len(old), 7) and np.allclose(frame["gt_boxes"], want, rtol=0, atol=1e-6)


def test_prediction_dicts_equal_the_reference(gold):
    seq = str(gold["sequence"])
    batch = {"frame_id": [f"{seq}_000", f"{seq}_001"], "metadata": [{"context_name": seq, "timestamp_micros": 1}, f"{seq}_001"]}
    preds = [{"pred_boxes": torch.from_numpy(gold["pred_boxes"].copy()), "pred_scores": torch.from_numpy(gold["pred_scores"]),
              "pred_labels": torch.from_numpy(gold["pred_labels"])},
             {"pred_boxes": torch.zeros((0, 7)), "pred_scores": torch.zeros(0), "pred_labels": torch.zeros(0, dtype=torch.long)}]
    full, empty = WaymoDataset.generate_prediction_dicts(batch, preds, cases.CLASSES)
    assert set(full) == set(empty) == {"name", "score", "boxes_lidar", "frame_id", "metadata"}
    assert list(full["name"]) == [str(n) for n in gold["pred_name"]]
    assert same_bits(full["score"], gold["pred_score"]) and same_bits(full["boxes_lidar"], gold["pred_boxes_lidar"])
    assert full["frame_id"] == f"{seq}_000" and full["metadata"] == batch["metadata"][0] and empty["metadata"] == f"{seq}_001"
    assert empty["boxes_lidar"].shape == (0, 7) and empty["name"].shape == (0,) and empty["score"].shape == (0,) and empty["name"].dtype == np.float64


def test_evaluators_that_are_out_of_reach_say_so(tmp_path, gold, tree):
    ds = WaymoDataset(cases.dataset_cfg(tree), cases.CLASSES, training=False)
    with pytest.raises(ImportError, match="waymo_open_dataset") as err:
        ds.evaluation([], cases.CLASSES, eval_metric="waymo")
    assert "tensorflow" in str(err.value).lower() and "kitti" in str(err.value)
    with pytest.raises(NotImplementedError, match="eval_metric"):
        ds.evaluation([], cases.CLASSES, eval_metric="nuscenes")
    unlabelled = golden_dataset(tmp_path, gold)
    unlabelled.infos = unlabelled.infos[1:]
    assert unlabelled.evaluation([], cases.CLASSES, eval_metric="kitti") == ("No ground-truth boxes for evaluation", {})


def test_the_info_builder_command_says_it_is_out_of_scope():
    with pytest.raises(SystemExit) as err:
        waymo_dataset.main(["create_waymo_infos", "unused.yaml"])
    assert "out of scope" in str(err.value) and "TFRecords" in str(err.value) and "create_waymo_gt_database" in str(err.value)


def test_registry_configs_and_header():
    assert registry["WaymoDataset"] is WaymoDataset and registry["WaymoNusMixDataset"] is WaymoNusMixDataset
    assert all(registry[n] is WaymoNusMixDataset for n in ("WaymoNusPolarMixDataset", "WaymoNusCutMixDataset", "WaymoNusLaserMixDataset"))
    data = cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/dataset_configs/waymo_dataset.yaml"), AttrDict())
    assert data.DATASET == "WaymoDataset" and data.PROCESSED_DATA_TAG == "waymo_processed_data_v0_5_0" and data.SAMPLED_INTERVAL == {"train": 5, "test": 1}
    assert data.POINT_CLOUD_RANGE == [-75.2, -75.2, -2, 75.2, 75.2, 4] and data.DATA_PROCESSOR[2].VOXEL_SIZE == [0.1, 0.1, 0.15]
    assert data.FILTER_EMPTY_BOXES_FOR_TRAIN is True and data.DISABLE_NLZ_FLAG_ON_POINTS is True and data.DATA_SPLIT == {"train": "train", "test": "val"}
    assert data.POINT_FEATURE_ENCODING.used_feature_list == ["x", "y", "z", "intensity", "elongation"]
    sampler = data.DATA_AUGMENTOR.AUG_CONFIG_LIST[0]
    assert sampler.NAME == "gt_sampling" and sampler.NUM_POINT_FEATURES == 5 and sampler.SAMPLE_GROUPS == ["Vehicle:15", "Pedestrian:10", "Cyclist:10"]
    assert sampler.DB_INFO_PATH == ["waymo_processed_data_v0_5_0_waymo_dbinfos_train_sampled_1.pkl"]
    model = cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/models/centerpoint_waymo_real.yaml"), AttrDict())
    assert model.MODEL.NAME == "CenterPoint" and model.DATA_CONFIG.DATASET == "WaymoDataset" and model.CLASS_NAMES == cases.CLASSES
    assert model.MODEL.BACKBONE_3D.NAME == "VoxelResBackBone8x" and model.MODEL.POST_PROCESSING.EVAL_METRIC == "kitti"
    stage1 = cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/models/toda_stage1_waymo_nus_polarmix_real.yaml"), AttrDict())
    mix = stage1.DATA_CONFIG
    assert registry[mix.DATASET] is WaymoNusMixDataset and mix.MIX_TYPE == "polarmix" and mix.POLARMIX_PROB == 0.2 and mix.MIX_INC_METHOD == "corner_del"
    assert stage1.CLASS_NAMES == mix.CLASS_NAMES == ["car"] and mix.POINT_CLOUD_RANGE == [-54.0, -54.0, -5.0, 54.0, 54.0, 4.8]
    assert mix.WaymoDataset.CLASS_NAMES == ["Vehicle"] and mix.WaymoDataset.OTHER_CHANNEL == "modes/16^" and mix.WaymoDataset.DATASET == "WaymoDataset"
    assert mix.NuScenesDataset.CLASS_NAMES == ["car"] and mix.NuScenesDataset.MAX_SWEEPS == 1 and mix.NuScenesDataset.SHIFT_COOR == [0.0, 0.0, 1.8]
    assert not mix.NuScenesDataset.BALANCED_RESAMPLING and mix.NuScenesDataset.VERSION == "v1.0-trainval"
    assert [a.NAME for a in mix.WaymoDataset.DATA_AUGMENTOR.AUG_CONFIG_LIST] == [a.NAME for a in mix.NuScenesDataset.DATA_AUGMENTOR.AUG_CONFIG_LIST]
    assert "gt_sampling" in mix.WaymoDataset.DATA_AUGMENTOR.DISABLE_AUG_LIST and mix.POINT_FEATURE_ENCODING.normalize_intensity is True
    header = open(os.path.join(ROOT, "include", "toda.h")).read()
    assert "int toda_waymo_frame(const float* rows, int n, int c_in, int use_nlz, float* out, int32_t* flags, void* stream);" in header
    assert "waymo_frame.hip" in open(os.path.join(ROOT, "toda_amd", "csrc", "Makefile")).read()


def test_frame_entry_point_checks_sizes_before_pointers():
    from toda_amd import lib as L
    lib = L.load()
    fake = 4096                                                                          # never dereferenced: every call below returns before a launch

    def call(n, c_in, rows=fake, out=fake, flags=fake):
        return lib.toda_waymo_frame(rows, n, c_in, 1, out, flags, None)

    assert call(-1, 6) == -1 and lib.toda_last_error() == b"waymo_frame: need n >= 0"
    assert call(8, 5) == -1 and b"5 columns" in lib.toda_last_error() and b"NLZ" in lib.toda_last_error()
    assert call(0, 5, None, None, None) == -1                                            # sizes are checked before n == 0 is served
    assert call(0, 6, None, None, None) == 0 and call(0, 7) == 0
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert call(8, 6, *args) == -1 and lib.toda_last_error() == b"waymo_frame: null rows, out or flags"


# ---- the index policy of the two-domain dataset ----------------------------------------------------------------------------
class _Frames:
    def __init__(self, n):
        self.infos = list(range(n))


class _Identity:
    def forward(self, data):
        return data


def stub_mix(n_source, n_target, prob, training=True, boxes_after_mix=None):
    ds = WaymoNusMixDataset.__new__(WaymoNusMixDataset)
    ds.source, ds.target, ds.mix_prob, ds.training = _Frames(n_source), _Frames(n_target), prob, training
    ds._merge_all_iters_to_one_epoch, ds.total_epochs, ds.data_processor = False, 0, _Identity()
    ds.source_frame = lambda i: {"from": ("source", i), "gt_boxes": np.ones((2, 8), np.float32), "gt_names": np.array(["car", "car"])}
    ds.target_frame = lambda i: {"from": ("target", i), "gt_boxes": np.ones((3, 8), np.float32), "gt_names": np.array(["car"] * 3)}
    ds.mix = lambda s, t: {"from": ("mix", s["from"][1], t["from"][1]), "gt_boxes": np.ones((5, 8), np.float32) if boxes_after_mix is None else boxes_after_mix}
    return ds


def test_mix_dataset_length_and_unmixed_branches():
    ds = stub_mix(5, 3, prob=0.0)
    assert len(ds) == 8 and ds.num_source == 5 and ds.num_target == 3
    assert [ds[i]["from"] for i in range(8)] == [("source", i) for i in range(5)] + [("target", i) for i in range(3)]
    assert all("gt_names" not in ds[i] for i in range(8))
    ds.merge_all_iters_to_one_epoch(merge=True, epochs=4)
    assert len(ds) == 32
    assert ds[8]["from"] == ("source", 0) and ds[8 + 6]["from"] == ("target", 1) and ds[31]["from"] == ("target", 2)      # the modulo of the length


def test_mix_dataset_mixed_branch_takes_both_indices_modulo_their_lists():
    ds = stub_mix(5, 3, prob=1.0)
    assert [ds[i]["from"] for i in range(8)] == [("mix", i % 5, i % 3) for i in range(8)]
    ds.merge_all_iters_to_one_epoch(merge=True, epochs=2)
    assert ds[13]["from"] == ("mix", 0, 2)                                               # 13 % 8 = 5


def test_mix_dataset_draws_once_against_the_probability():
    ds = stub_mix(4, 4, prob=0.5)
    np.random.seed(11)
    draws = np.random.random(8)
    np.random.seed(11)
    got = [ds[i]["from"][0] for i in range(8)]
    assert got == ["mix" if d < 0.5 else ("source" if i < 4 else "target") for i, d in enumerate(draws)]
    assert "mix" in got and len(set(got)) > 1


def test_mix_dataset_draws_again_when_the_boxes_are_unusable():
    # a mix whose boxes are not 2-D, then frames without a box: both end in a re-draw (np.random.randint) until a usable sample comes
    calls = []
    ds = stub_mix(2, 2, prob=1.0, boxes_after_mix=np.ones((8,), np.float32))
    real = ds.mix

    def mix_once_bad(s, t):
        calls.append((s["from"][1], t["from"][1]))
        return real(s, t) if len(calls) == 1 else {"from": "second", "gt_boxes": np.ones((1, 8), np.float32)}
    ds.mix = mix_once_bad
    np.random.seed(0)
    assert ds[1]["from"] == "second" and len(calls) == 2
    empty = stub_mix(2, 2, prob=0.0)
    seen = []
    empty.source_frame = lambda i: seen.append(i) or {"from": ("source", i), "gt_boxes": np.zeros((0, 8), np.float32)}
    np.random.seed(0)
    assert empty[0]["from"][0] == "target" and seen[0] == 0                              # re-drawn until a target frame (3 boxes) came
    empty.training = False
    assert empty[0]["from"] == ("source", 0)                                             # no re-draw outside training
