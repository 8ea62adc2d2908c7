"""Host side of the KITTI evaluator: the numpy restatement (tests/kitti_eval_cases.py) reproduces the fixtures captured from
the reference, the committed fixtures satisfy their screening, the LiDAR-frame conversion equals the capture, the new entry
points reject bad arguments without a device, and the synthetic dataset's default report is unchanged."""
import copy
import os

import numpy as np
import pytest

from tests import kitti_eval_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def E():
    from toda_amd.pcdet.datasets.kitti.kitti_object_eval_python import eval as ev
    return ev


def load(name):
    z = np.load(os.path.join(GOLDEN, f"kitti_eval_{name}.npz"))
    return z, C.unpack(z, "gt"), C.unpack(z, "dt")


def test_restated_overlaps_reproduce_the_capture():
    z = np.load(os.path.join(GOLDEN, "kitti_eval_overlaps.npz"))
    # fp32 only, at the project's parity bound: the capture's rotated part is fp32, and on its degenerate pairs (identical,
    # touching, shared corners) the outcome of the inside and crossing tests hangs on fp32 rounding - the same rules in fp64
    # differ there by up to 0.33.  The fp64 restatement is held to the screened evaluator fixtures below instead.
    for dtype, tol in ((np.float32, 1e-4),):
        for metric in (0, 1, 2):
            for crit in (-1, 0, 1, 2):
                got = []
                for f in range(len(z["box_off"]) - 1):
                    b, q = slice(z["box_off"][f], z["box_off"][f + 1]), slice(z["query_off"][f], z["query_off"][f + 1])
                    got.append(C.overlaps(z["box3d"][b], z["bbox"][b], z["query3d"][q], z["query_bbox"][q], metric, crit, dtype).reshape(-1))
                want = z[f"expect_m{metric}_c{crit}"]
                # criterion 2 of the image metric is an area in px^2 (up to 1e4), not a ratio in [0, 1], and fp32 carries it to
                # about 1e-7 of its size: relative there, a stated departure from the issue's absolute bound
                scale = np.maximum(np.abs(want), 1.0) if (metric == 0 and crit == 2) else 1.0
                assert np.max(np.abs(np.concatenate(got) - want) / scale) <= tol, (dtype, metric, crit)


@pytest.mark.parametrize("name", ["match", "ties", "lidar"])
def test_fixtures_satisfy_their_screening(name):
    z, gts, dts = load(name)
    gap, shared = C.screen([z[f"overlaps_{m}"] for m in (0, 1, 2)], dts)
    assert gap >= 1e-3
    assert shared == (1 if name == "ties" else 0)                     # the ties fixture shares one score on purpose
    if name == "match":
        assert len(gts) == 40 and any(len(g["name"]) == 0 for g in gts) and any(len(d["name"]) == 0 for d in dts)
        names = set(np.concatenate([g["name"] for g in gts]))
        assert {"DontCare", "Van", "Car", "Person_sitting", "Pedestrian"} <= names
        occ = np.concatenate([g["occluded"] for g in gts])
        assert {0.0, 1.0, 2.0, 3.0} <= set(occ)


@pytest.mark.parametrize("name", ["match", "ties", "lidar"])
@pytest.mark.parametrize("backend", [C.HostBackend, C.HostBackend64])
def test_restated_evaluator_reproduces_the_reference_result(name, backend):
    ev = E()
    z, gts, dts = load(name)
    classes = [str(c) for c in z["classes"]]
    ids = [C.KITTI_CLASSES.index(c) for c in classes]
    for metric in (0, 1, 2):
        ret = ev.eval_class(gts, dts, ids, [0, 1, 2], metric, ev.MIN_OVERLAPS[:, :, ids], compute_aos=(metric == 0), backend=backend)
        got_pr = np.concatenate([pr for _, pr in ret["counts"].values()], 0)           # against the reference's own tables
        assert [len(th) for th, _ in ret["counts"].values()] == list(z[f"counts_len_{metric}"])
        assert np.array_equal(got_pr[:, :3], z[f"counts_{metric}"][:, :3])
        assert np.allclose(got_pr[:, 3], z[f"counts_{metric}"][:, 3], rtol=1e-6, atol=0)
        assert np.array_equal(ret["precision"], z[f"precision_{metric}"], equal_nan=True)
        assert np.array_equal(ret["recall"], z[f"recall_{metric}"], equal_nan=True)
        assert np.allclose(ret["orientation"], z[f"orientation_{metric}"], rtol=1e-6, atol=0, equal_nan=True)
    text, res = ev.get_official_eval_result(gts, dts, classes, backend=backend)
    assert text == str(z["result_str"])
    assert sorted(res) == [str(k) for k in z["ret_keys"]]
    assert np.allclose([res[str(k)] for k in z["ret_keys"]], z["ret_vals"], rtol=1e-6, atol=0)


def test_transform_annotations_to_kitti_format_equals_the_capture():
    from toda_amd.pcdet.datasets.kitti.kitti_utils import transform_annotations_to_kitti_format
    z, gts, dts = load("lidar")
    mapping = {str(k): str(v) for k, v in zip(z["map_keys"], z["map_vals"])}
    infos, dets = C.lidar_frames(int(z["seed"]))
    g, d = copy.deepcopy(infos), copy.deepcopy(dets)
    assert transform_annotations_to_kitti_format(d, map_name_to_kitti=mapping) is d
    transform_annotations_to_kitti_format(g, map_name_to_kitti=mapping)
    for got, want in ((g, gts), (d, dts)):
        for a, b in zip(got, want):
            assert list(a["name"]) == list(b["name"]) and "gt_names" not in a
            for k in ("bbox", "location", "dimensions", "rotation_y", "alpha", "truncated", "occluded"):
                assert np.array_equal(np.asarray(a[k], np.float64).reshape(np.shape(b[k])), b[k]), k
    fake = [{"name": np.array(["car"]), "boxes_lidar": np.array([[1.0, 2.0, -1.0, 1.6, 3.9, 1.5, 0.3]])}]
    transform_annotations_to_kitti_format(fake, map_name_to_kitti=mapping, info_with_fakelidar=True)
    assert np.allclose(fake[0]["dimensions"], [[3.9, 1.5, 1.6]]) and np.allclose(fake[0]["location"], [[-2.0, 1.0, 1.0]])
    assert np.allclose(fake[0]["rotation_y"], [0.3])


def test_get_thresholds_and_means():
    ev = E()
    th = ev.get_thresholds(np.array([0.9, 0.1, 0.5, 0.7]), 4)
    assert th == [0.9, 0.7, 0.5, 0.1]
    assert len(ev.get_thresholds(np.linspace(0.01, 1, 100), 100)) == 41
    assert ev.get_thresholds(np.zeros(0), 0) == []
    prec = np.ones((2, 3, 2, 41))
    assert np.all(ev.get_mAP(prec) == 100.0) and np.all(ev.get_mAP_R40(prec) == 100.0)
    n, ign_gt, ign_det, dc = ev.clean_data({"name": np.array(["Car", "Van", "DontCare", "Car"]), "occluded": np.array([0, 0, -1, 2]),
                                            "truncated": np.zeros(4), "bbox": np.array([[0, 0, 10, 50.0]] * 4)},
                                           {"name": np.array(["Car", "Pedestrian", "Car"]), "bbox": np.array([[0, 0, 9, 45.0], [0, 0, 9, 45.0], [0, 0, 9, 30.0]])},
                                           0, 0)
    assert (n, ign_gt, ign_det, len(dc)) == (1, [0, 1, -1, 1], [0, -1, 1], 1)


def test_entry_points_reject_bad_arguments_without_a_device():
    import torch

    from toda_amd import lib as L
    from toda_amd import ops
    lib = L.load()
    assert lib.toda_eval_overlaps(None, None, None, None, None, None, None, 4, 10, 3, -1, None, None) == -1 and b"metric" in lib.toda_last_error()
    assert lib.toda_eval_overlaps(None, None, None, None, None, None, None, 4, 10, 1, 5, None, None) == -1 and b"criterion" in lib.toda_last_error()
    assert lib.toda_eval_overlaps(None, None, None, None, None, None, None, 4, 10, 1, -1, None, None) == -1 and b"null" in lib.toda_last_error()
    assert lib.toda_eval_overlaps(None, None, None, None, None, None, None, 0, 0, 1, -1, None, None) == 0      # nothing to do
    assert lib.toda_eval_overlaps(None, None, None, None, None, None, None, 4, 0, 2, 0, None, None) == 0
    need = lib.toda_eval_match_workspace_bytes(100, 41, 2000)
    assert need >= 100 * 41 * 4 * 8 + 41 * 2000 and lib.toda_eval_match_workspace_bytes(0, 41, 10) == 0
    one = L.hptr(L.host_f64([0.0]))
    args = [one] * 12
    assert lib.toda_eval_match(*args, 100, 2000, one, 41, 0.7, 1, 0, one, one, need - 1, None) == -1 and b"workspace" in lib.toda_last_error()
    assert lib.toda_eval_match(*args, 100, 2000, one, 41, 1.5, 1, 0, one, one, need, None) == -1 and b"min_overlap" in lib.toda_last_error()
    assert lib.toda_eval_match(*args, 100, 2000, one, 41, 0.7, 4, 0, one, one, need, None) == -1 and b"metric" in lib.toda_last_error()
    assert lib.toda_eval_match(*args, 100, 2000, one, 0, 0.7, 1, 0, one, one, need, None) == 0                 # no thresholds
    assert lib.toda_eval_match_scores(*([one] * 7), 100, 2000, 0.7, one, one, one, 8, None) == -1 and b"workspace" in lib.toda_last_error()
    assert lib.toda_eval_match_scores(*([None] * 7), 0, 0, 0.7, None, None, None, 0, None) == 0
    with pytest.raises(RuntimeError, match="GPU"):
        ops.eval_overlaps(None, None, torch.zeros(2, dtype=torch.int32), None, None, torch.zeros(2, dtype=torch.int32),
                          torch.zeros(2, dtype=torch.int64), 0, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.eval_match_scores(torch.zeros(1), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
                              torch.zeros(2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32),
                              torch.zeros(0, dtype=torch.float64), 0.7)


def test_synthetic_evaluation_without_the_kitti_metric_is_unchanged():
    """The case of tests/test_eval_host.py::test_centre_distance_evaluation_counts: same text, same numbers, for no
    eval_metric and for the `synthetic` every shipped YAML sets."""
    from tests.test_eval_host import toda_cfg
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    cfg = toda_cfg(samples=2)
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=False)
    assert dict(cfg.DATA_CONFIG.MAP_CLASS_TO_KITTI)["car"] == "Car"
    annos = []
    for k, info in enumerate(ds.infos):
        boxes = info["gt_boxes"].copy()
        boxes[:, 0] += 0.5
        boxes = np.concatenate([boxes[: len(boxes) // 2], boxes[:1] + 30.0], 0)
        annos.append({"frame_id": f"syn_{k:06d}", "name": np.array(["car"] * len(boxes)), "score": np.linspace(1, 0.5, len(boxes)),
                      "boxes_lidar": boxes})
    n_gt = sum(len(i["gt_boxes"]) for i in ds.infos)
    n_hit = sum(len(i["gt_boxes"]) // 2 for i in ds.infos)
    n_det = sum(len(a["name"]) for a in annos)
    want = {"car/recall_2m": n_hit / n_gt, "car/precision_2m": n_hit / n_det}
    want_text = f"car: recall@2m {n_hit / n_gt:.4f} precision@2m {n_hit / n_det:.4f} ({n_hit} TP / {n_gt} gt / {n_det} det)"
    for kwargs in ({}, {"eval_metric": "synthetic"}, {"eval_metric": None, "output_path": None}):
        text, res = ds.evaluation(annos, ["car"], **kwargs)
        assert text == want_text and res == want
