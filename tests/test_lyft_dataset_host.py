"""LyftDataset without a GPU: the numpy route against the reference's own clouds (tests/golden/lyft_dataset.npz), truncated and
empty files, the ego rectangle, prediction dicts and get_ap against the reference's outputs, the registry, the two YAMLs, and
what is refused."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import lyft_dataset_cases as cases
from tests import lyft_eval_cases as E
from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
from toda_amd.pcdet.datasets.lyft import lyft_dataset as LD
from toda_amd.pcdet.datasets.lyft import lyft_eval
from toda_amd.pcdet.datasets.lyft.lyft_dataset import LyftDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return cases.load_golden()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    data_path = tmp_path_factory.mktemp("lyft")
    return data_path, cases.write_tree(data_path)


def bare(root, infos):
    ds = LyftDataset.__new__(LyftDataset)
    ds.root_path, ds.infos = root, infos
    return ds


# ---- the numpy route against the reference ------------------------------------------------------------------------------
def test_the_numpy_route_equals_the_reference_bit_for_bit(tmp_path, gold):
    ds = bare(tmp_path, cases.write_golden_files(tmp_path, gold))
    for sample, max_sweeps in gold["runs"]:
        np.random.seed(int(gold["seed"]))
        got = ds.get_lidar_with_sweeps_host(int(sample), int(max_sweeps))
        want = gold[f"points_{sample}_{max_sweeps}"]
        assert got.dtype == np.float32 and cases.same_bits_nan_aware(got, want), (sample, max_sweeps)
    assert np.isnan(gold["points_0_5"]).any() and len(gold["points_1_1"]) == 257          # NaN rows pass; the key frame of sample 1 lost 7 bytes


def test_files_lose_their_tail_and_an_empty_file_reads_as_no_rows(tmp_path, gold):
    cases.write_golden_files(tmp_path, gold)
    sizes = [os.path.getsize(tmp_path / f"f{k}.bin") for k in range(5)]
    assert [s % 20 for s in sizes] == [0, 0, 7, 19, 1] and sizes[1] == 0
    rows, offsets = LyftDataset.read_rows([tmp_path / f"f{k}.bin" for k in range(5)])
    assert offsets == [0, 256, 256, 513, 768, 808] and rows.shape == (808, 5) and rows.dtype == np.float32
    for k in range(5):
        assert rows[offsets[k]:offsets[k + 1]].tobytes() == cases.golden_rows(gold, k).tobytes()
        assert LyftDataset.read_points_host(tmp_path / f"f{k}.bin").tobytes() == np.ascontiguousarray(cases.golden_rows(gold, k)[:, :4]).tobytes()
    for tail in range(1, 20):                                                            # every trailing length
        path = tmp_path / f"tail{tail}.bin"
        with open(path, "wb") as f:
            f.write(cases.golden_rows(gold, 0)[:3].tobytes() + b"\xff" * tail)
        assert LyftDataset.read_rows([path])[1] == [0, 3] and LyftDataset.read_points_host(path).shape == (3, 4)


def test_the_ego_cut_is_an_open_rectangle_on_the_sweeps_only(tree):
    data_path, root = tree
    ds = LyftDataset(cases.dataset_cfg(data_path), cases.CLASSES, training=True)
    assert len(ds) == 2 and ds.on_device and ds.max_sweeps == 5
    info = ds.infos[0]
    pts, stamp = LyftDataset.get_sweep_host(root / info["sweeps"][1]["lidar_path"], None, 0.25)
    raw = LyftDataset.read_points_host(root / info["sweeps"][1]["lidar_path"])
    assert stamp.shape == (len(pts), 1) and stamp.dtype == np.float64 and (stamp == 0.25).all()
    first = cases.N_IN_FIRST
    for k, ((x, y), keep) in enumerate(cases.EGO_ROWS):
        row = raw[first + k]
        assert (np.isnan(row[0]) if np.isnan(x) else row[0] == np.float32(x)) and (np.isnan(row[1]) if np.isnan(y) else row[1] == np.float32(y))
        present = (pts[:, 3] == row[3]).any()                                            # the intensity draws are distinct
        assert present == bool(keep), (k, x, y)
    assert len(raw) - len(pts) == sum(1 - keep for _, keep in cases.EGO_ROWS) == 7
    np.random.seed(3)
    cloud = ds.get_lidar_with_sweeps_host(0, 5)
    np.random.seed(3)
    paths, mats, lags, ego = ds._sweep_table(info, 5)
    counts = np.diff(LyftDataset.read_rows(paths)[1])
    assert ego == [False, True, True, True, True] and mats[0] is None and sum(m is None for m in mats[1:]) == 2        # the repeated sweep
    assert len(cloud) == counts[0] + sum(c - 7 for c in counts[1:])                      # the key frame keeps its rows inside the rectangle
    key = LyftDataset.read_points_host(paths[0])
    assert cases.same_bits_nan_aware(cloud[:len(key), :4], np.ascontiguousarray(key)) and (cloud[:len(key), 4] == 0).all()
    with pytest.raises(ValueError, match="Cannot take a larger sample"):
        ds._sweep_table(info, 6)                                                         # np.random.choice without replacement, as in the reference


def test_raw_frame_and_len(tree):
    data_path, root = tree
    ds = LyftDataset(cases.dataset_cfg(data_path, MAX_SWEEPS=1), cases.CLASSES, training=False)
    assert len(ds) == 1 and not ds.on_device
    frame = ds.raw_frame(0)
    assert isinstance(frame["points"], np.ndarray) and frame["points"].shape[1] == 5 and (frame["points"][:, 4] == 0).all()
    assert frame["gt_boxes"].shape == (17, 7) and frame["gt_names"].tolist() == cases.frame_boxes(2)[1].tolist()
    assert frame["metadata"] == {"token": "token2"} and frame["frame_id"] == "host-a101_lidar1_1200000002"
    ds.merge_all_iters_to_one_epoch(merge=True, epochs=7)
    assert len(ds) == 7


# ---- predictions and the curve against the reference ----------------------------------------------------------------------
def test_prediction_dicts_equal_the_reference(gold):
    ds = LyftDataset.__new__(LyftDataset)
    batch = {"frame_id": ["a", "b"], "metadata": [{"token": "t0"}, {"token": "t1"}]}
    preds = [{"pred_boxes": torch.from_numpy(gold["pred_boxes"].copy()), "pred_scores": torch.from_numpy(gold["pred_scores"]), "pred_labels": torch.from_numpy(gold["pred_labels"])},
             {"pred_boxes": torch.zeros((0, 7)), "pred_scores": torch.zeros(0), "pred_labels": torch.zeros(0, dtype=torch.long)}]
    full, empty = ds.generate_prediction_dicts(batch, preds, cases.CLASSES)
    assert sorted(full) == sorted(empty) == ["boxes_lidar", "frame_id", "metadata", "name", "pred_labels", "score"]
    assert full["name"].tolist() == gold["pred_name"].tolist() and np.array_equal(full["score"], gold["pred_score"])
    assert np.array_equal(full["boxes_lidar"], gold["pred_boxes_lidar"]) and np.array_equal(full["pred_labels"], gold["pred_out_labels"])
    assert full["metadata"] == {"token": "t0"} and empty["frame_id"] == "b"
    assert empty["boxes_lidar"].shape == (0, 7) and empty["name"].shape == (0,) and empty["pred_labels"].dtype == np.float64


def test_get_ap_equals_the_reference(gold):
    """The reference's get_ap on curves of made-up flag sequences: the restatement's get_ap and the evaluator's curves against it."""
    for k in range(int(gold["ap_cases"])):
        flags, n_gt, want = gold[f"ap{k}_flags"], int(gold[f"ap{k}_n_gt"]), float(gold[f"ap{k}"])
        tp, fp = np.cumsum(flags.astype(np.float64)), np.cumsum(1.0 - flags)
        assert E.get_ap(tp / float(n_gt), tp / np.maximum(tp + fp, np.finfo(np.float64).eps)) == want
        scores = np.linspace(1.0, 0.5, len(flags))                                      # already in score order
        got = lyft_eval.average_precisions(flags[None, :], scores, np.zeros(len(flags), np.int64), np.array([n_gt]), 1)
        assert got.shape == (1, 1) and abs(got[0, 0] - want) < 1e-9, (k, got, want)
    assert float(gold["ap0"]) == pytest.approx(0.5 + 0.5 * 2 / 3) and float(gold["ap1"]) == 0.0 and float(gold["ap2"]) == 1.0


# ---- registry, YAMLs, refusals ----------------------------------------------------------------------------------------------
def test_registry_and_yamls():
    from toda_amd.pcdet import datasets
    assert datasets.__all__["LyftDataset"] is LyftDataset
    data = cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/dataset_configs/lyft_dataset.yaml"), AttrDict())
    assert data.DATASET == "LyftDataset" and data.MAX_SWEEPS == 5 and data.VERSION == "trainval"
    assert list(data.POINT_CLOUD_RANGE) == [-80.0, -80.0, -5.0, 80.0, 80.0, 3.0]
    assert list(data.EVAL_LYFT_IOU_LIST) == [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]
    voxels = [p for p in data.DATA_PROCESSOR if p.NAME == "transform_points_to_voxels"][0]
    assert list(voxels.VOXEL_SIZE) == [0.1, 0.1, 0.2] and voxels.MAX_NUMBER_OF_VOXELS["train"] == 80000
    assert dict(data.INFO_PATH) == {"train": ["lyft_infos_train.pkl"], "test": ["lyft_infos_val.pkl"]}
    path = os.path.join(ROOT, "toda_amd/tools/cfgs/models/centerpoint_lyft_real.yaml")
    header = open(path).read().split("CLASS_NAMES")[0]
    assert "reference ships no Lyft model" in header and "project's own" in header
    cwd = os.getcwd()
    os.chdir(os.path.join(ROOT, "toda_amd", "tools"))
    try:
        cfg = cfg_from_yaml_file(path, AttrDict())
    finally:
        os.chdir(cwd)
    assert cfg.DATA_CONFIG.DATASET == "LyftDataset" and cfg.MODEL.NAME == "CenterPoint" and cfg.MODEL.BACKBONE_3D.NAME == "VoxelResBackBone8x"
    assert list(cfg.CLASS_NAMES) == ["car", "truck", "bus", "emergency_vehicle", "other_vehicle", "motorcycle", "bicycle", "pedestrian", "animal"]
    assert [list(g) for g in cfg.MODEL.DENSE_HEAD.CLASS_NAMES_EACH_HEAD] == [["car"], ["truck", "bus", "emergency_vehicle", "other_vehicle"],
                                                                             ["motorcycle", "bicycle"], ["pedestrian", "animal"]]
    assert cfg.MODEL.POST_PROCESSING.EVAL_METRIC == "lyft" and "vel" not in cfg.MODEL.DENSE_HEAD.SEPARATE_HEAD_CFG.HEAD_ORDER


def test_what_is_refused(tree, tmp_path):
    data_path, root = tree
    ds = LyftDataset(cases.dataset_cfg(data_path), cases.CLASSES, training=False)
    annos = [{"name": np.array(["car"]), "score": np.array([0.5], np.float32), "boxes_lidar": np.zeros((1, 7), np.float32) + 1, "pred_labels": np.array([1]),
              "frame_id": "x", "metadata": {"token": "token2"}}]
    with pytest.raises(KeyError, match="emergency_vehicle"):
        ds.evaluation(annos, ["car", "emergency_vehicle"], eval_metric="kitti")
    with pytest.raises(NotImplementedError, match="nds"):
        ds.evaluation(annos, ["car"], eval_metric="nds")
    bare_path = tmp_path / "no_tables"
    cases.write_tree(bare_path, tables=False)
    no_tables = LyftDataset(cases.dataset_cfg(bare_path), cases.CLASSES, training=False)
    with pytest.raises(FileNotFoundError, match=r"data/sample_annotation\.json.*eval_metric 'kitti'"):
        no_tables.evaluation(annos, ["car"], eval_metric="lyft")
    with pytest.raises(SystemExit, match="out of scope"):
        LD.create_lyft_info("trainval", data_path, data_path, None)
    with pytest.raises(SystemExit, match="out of scope"):
        LD.main(["create_lyft_infos", os.path.join(ROOT, "toda_amd/tools/cfgs/dataset_configs/lyft_dataset.yaml")])
    before = pickle.dumps(ds.infos)
    assert ds.infos[0]["gt_boxes"].shape == (17, 7) and pickle.dumps(ds.infos) == before
