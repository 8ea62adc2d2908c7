"""The KITTI evaluator on the GPU: the overlap and matching kernels against the fixtures captured from the reference
(tests/golden/capture_kitti_eval.py) and against the numpy restatement (tests/kitti_eval_cases.py) at the edge shapes.

Observed on one MI355X (printed by the tests): largest overlap difference to the capture over all metrics and criteria
9.5e-7 for the ratios (1.1e-5 relative for the criterion-2 areas); counts, precision, recall, every AP and the text equal to the reference's."""
import os

import numpy as np
import pytest
import torch

from tests import kitti_eval_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def E():
    from toda_amd.pcdet.datasets.kitti.kitti_object_eval_python import eval as ev
    return ev


def load(name):
    z = np.load(os.path.join(GOLDEN, f"kitti_eval_{name}.npz"))
    return z, C.unpack(z, "gt"), C.unpack(z, "dt")


def cuda(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def test_overlaps_match_the_capture_for_every_metric_and_criterion():
    from toda_amd import ops
    z = np.load(os.path.join(GOLDEN, "kitti_eval_overlaps.npz"))
    nb, nq = np.diff(z["box_off"]), np.diff(z["query_off"])
    out_off = np.concatenate([[0], np.cumsum(nb * nq)])
    worst = 0.0
    for metric in (0, 1, 2):
        for crit in (-1, 0, 1, 2):
            got = ops.eval_overlaps(cuda(z["box3d"], torch.float32), cuda(z["bbox"], torch.float32), cuda(z["box_off"], torch.int32),
                                    cuda(z["query3d"], torch.float32), cuda(z["query_bbox"], torch.float32),
                                    cuda(z["query_off"], torch.int32), cuda(out_off, torch.int64), int(out_off[-1]), metric, crit)
            want = z[f"expect_m{metric}_c{crit}"]
            # criterion 2 of the image metric is an area in px^2 (up to 1e4), not a ratio in [0, 1], and fp32 carries it to
            # about 1e-7 of its size: relative there, a stated departure from the issue's absolute bound
            scale = np.maximum(np.abs(want), 1.0) if (metric == 0 and crit == 2) else 1.0
            diff = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - want) / scale))
            print(f"metric {metric} criterion {crit}: max |diff| {diff:.3e} over {len(want)} pairs")
            worst = max(worst, diff)
            assert diff <= 1e-4
    print(f"largest overlap difference to the capture: {worst:.3e}")


def test_rotate_iou_gpu_eval_numpy_in_numpy_out():
    from toda_amd.pcdet.datasets.kitti.kitti_object_eval_python.rotate_iou import rotate_iou_gpu_eval
    z = np.load(os.path.join(GOLDEN, "kitti_eval_overlaps.npz"))
    f = 12
    b = z["box3d"][z["box_off"][f]:z["box_off"][f + 1]][:, [0, 2, 3, 5, 6]]
    q = z["query3d"][z["query_off"][f]:z["query_off"][f + 1]][:, [0, 2, 3, 5, 6]]
    start = int((np.diff(z["box_off"]) * np.diff(z["query_off"]))[:f].sum())
    for crit in (-1, 0, 1):
        got = rotate_iou_gpu_eval(b, q, crit)
        assert got.shape == (len(b), len(q)) and got.dtype == b.dtype
        assert np.abs(got.reshape(-1) - z[f"expect_m1_c{crit}"][start:start + got.size]).max() <= 1e-4
    assert rotate_iou_gpu_eval(b[:0], q).shape == (0, len(q))


def test_a_rotated_box_against_itself_has_iou_one():
    """Bit-identical rotated rectangles: every corner lies exactly on the other boundary.  The reference leaves that to the
    signs of rounded dot products that are zero in exact arithmetic and returns 0, 1/3 or 1 (0.0 for the first box below);
    the kernel takes a corner that equals a corner of the other rectangle as inside.  The bound is the parity tolerance."""
    from toda_amd import ops
    rng = np.random.default_rng(5)
    n = 300
    b3 = np.stack([rng.uniform(-40, 40, n), rng.uniform(1.2, 2.2, n), rng.uniform(5, 70, n), rng.uniform(0.5, 10, n),
                   rng.uniform(1, 3, n), rng.uniform(0.5, 3, n), rng.uniform(-np.pi, np.pi, n)], 1)
    b3[0] = [2.0, 1.6, 20.0, 4.0, 1.5, 1.8, 0.3]
    off = cuda(np.arange(n + 1), torch.int32)                                  # one box per frame, against itself
    box = cuda(b3, torch.float32)
    for metric in (1, 2):
        got = ops.eval_overlaps(box, None, off, box, None, off, cuda(np.arange(n + 1), torch.int64), n, metric, -1).cpu().numpy()
        print(f"metric {metric}: IoU of {n} boxes with themselves in [{got.min():.7f}, {got.max():.7f}]")
        assert np.abs(got - 1.0).max() <= 1e-4
    b32 = b3.astype(np.float32)
    assert abs(C.rect_inter(b32[0, [0, 2, 3, 5, 6]], b32[0, [0, 2, 3, 5, 6]], np.float32) / (b32[0, 3] * b32[0, 5]) - 1.0) <= 1e-4


@pytest.mark.parametrize("name", ["match", "ties", "lidar"])
def test_counts_curves_and_result_equal_the_reference(name):
    ev = E()
    z, gts, dts = load(name)
    classes = [str(c) for c in z["classes"]]
    ids = [C.KITTI_CLASSES.index(c) for c in classes]
    min_overlaps = ev.MIN_OVERLAPS[:, :, ids]
    for metric in (0, 1, 2):
        dev = ev.eval_class(gts, dts, ids, [0, 1, 2], metric, min_overlaps, compute_aos=(metric == 0))
        host = ev.eval_class(gts, dts, ids, [0, 1, 2], metric, min_overlaps, compute_aos=(metric == 0), backend=C.HostBackend)
        n_thresh = 0
        for key, (th, pr) in dev["counts"].items():
            th_h, pr_h = host["counts"][key]
            assert np.array_equal(th, th_h)
            assert np.array_equal(pr[:, :3], pr_h[:, :3]), (metric, key)                    # tp, fp, fn: integers, exactly
            assert np.allclose(pr[:, 3], pr_h[:, 3], rtol=1e-6, atol=0)
            n_thresh += len(th)
        assert n_thresh > 0
        # and against the reference's own tables, captured from its fused_compute_statistics: nothing of the restatement
        ref_pr = z[f"counts_{metric}"]
        assert [len(th) for th, _ in dev["counts"].values()] == list(z[f"counts_len_{metric}"])
        dev_pr = np.concatenate([pr for _, pr in dev["counts"].values()], 0)
        assert np.array_equal(dev_pr[:, :3], ref_pr[:, :3])
        assert np.allclose(dev_pr[:, 3], ref_pr[:, 3], rtol=1e-6, atol=0)
        assert np.array_equal(dev["precision"], z[f"precision_{metric}"], equal_nan=True)
        assert np.array_equal(dev["recall"], z[f"recall_{metric}"], equal_nan=True)
        assert np.allclose(dev["orientation"], z[f"orientation_{metric}"], rtol=1e-6, atol=0, equal_nan=True)
    text, res = ev.get_official_eval_result(gts, dts, classes)
    assert text == str(z["result_str"])
    assert sorted(res) == [str(k) for k in z["ret_keys"]]
    for k, v in zip(z["ret_keys"], z["ret_vals"]):
        if "_aos/" in str(k):
            assert np.isclose(res[str(k)], v, rtol=1e-6, atol=0)
        else:
            assert res[str(k)] == v, k


def test_two_runs_agree_bit_for_bit():
    ev = E()
    z, gts, dts = load("match")
    runs = []
    for _ in range(2):
        ret = ev.eval_class(gts, dts, [0, 1, 2], [0, 1, 2], 0, ev.MIN_OVERLAPS[:, :, [0, 1, 2]], compute_aos=True)
        runs.append(np.concatenate([pr.reshape(-1) for _, pr in ret["counts"].values()] + [ret["orientation"].reshape(-1)]))
    assert runs[0].tobytes() == runs[1].tobytes()


class DeviceOverlapHost(C.HostBackend):
    """The numpy matching on the DEVICE's overlaps: isolates the matching kernel from the last bit of the overlaps."""
    source = None

    def overlaps(self, metric):
        flat = self.source.ov[metric].cpu().numpy()
        off, p = self.p["ov_off"], self.p
        self.ov[metric] = [flat[off[f]:off[f + 1]].reshape(p["dt_off"][f + 1] - p["dt_off"][f], p["gt_off"][f + 1] - p["gt_off"][f])
                           for f in range(p["n_frames"])]


def both(gts, dts, ids, metrics=(0, 1, 2)):
    ev = E()
    prep = ev.prepare(gts, dts)
    out = []
    for metric in metrics:
        dev_be = ev.DeviceBackend(prep)
        dev = ev._eval_prepared(dev_be, prep, ids, [0, 1, 2], metric, ev.MIN_OVERLAPS[:, :, ids], metric == 0)
        host_be = DeviceOverlapHost(prep)
        host_be.source = dev_be
        host = ev._eval_prepared(host_be, prep, ids, [0, 1, 2], metric, ev.MIN_OVERLAPS[:, :, ids], metric == 0)
        for key, (th, pr) in dev["counts"].items():
            assert np.array_equal(th, host["counts"][key][0])
            assert np.array_equal(pr[:, :3], host["counts"][key][1][:, :3]), (metric, key)
            assert np.allclose(pr[:, 3], host["counts"][key][1][:, 3], rtol=1e-6, atol=0)
        assert np.array_equal(dev["precision"], host["precision"], equal_nan=True)
        out.append(dev)
    return out


def test_edge_one_frame_one_pair_one_threshold():
    gts, dts = C.kitti_frames(11, 1, classes=("Car",), mean_gt=1, extra_det=1, dontcare=False)
    gts[0]["occluded"][:], gts[0]["truncated"][:], gts[0]["bbox"][:] = 0, 0, [100.0, 100.0, 200.0, 200.0]
    det = {k: np.array(v[:1], copy=True) for k, v in gts[0].items()}
    det["score"] = np.array([0.9])
    det["location"] = det["location"] + 0.02
    ret = both(gts[:1], [det], [0])
    for r in ret:
        assert [len(th) for th, _ in r["counts"].values()] == [1] * 6                    # T = 1
    assert ret[1]["precision"][0, 0, 0, 0] == 1.0


def test_edge_frames_with_more_than_64_and_256_detections_and_41_thresholds():
    gts, dts = C.kitti_frames(28, 3, classes=("Car", "Van"), mean_gt=45, extra_det=260)
    sizes = sorted(len(d["name"]) for d in dts)
    assert sizes[-1] > 256 and 64 < sizes[0] <= 256
    both(gts, dts, [0, 3], metrics=(0, 2))
    # 41 thresholds straight at the kernel: the flags of Car / hard, every 41st-quantile of the scores as a threshold
    ev = E()
    prep = ev.prepare(gts, dts)
    dev_be, host_be = ev.DeviceBackend(prep), DeviceOverlapHost(prep)
    host_be.source = dev_be
    gt_h = prep["gt_bbox"][:, 3] - prep["gt_bbox"][:, 1]
    dt_h = np.abs(prep["dt_bbox"][:, 3] - prep["dt_bbox"][:, 1])
    ign_gt, ign_det = ev._flags(prep["gt_name"], gt_h, prep["occluded"], prep["truncated"], prep["dt_name"], dt_h, 0, 2)
    thresholds = np.quantile(prep["score"], np.linspace(1.0, 0.0, 41))
    for metric, level in ((0, 0.7), (1, 0.5)):
        dev_be.overlaps(metric)
        host_be.overlaps(metric)
        assert np.array_equal(np.sort(dev_be.match_scores(metric, ign_gt, ign_det, level)),
                              np.sort(host_be.match_scores(metric, ign_gt, ign_det, level)))
        pr = dev_be.match(metric, ign_gt, ign_det, thresholds, level, metric == 0)
        pr_h = host_be.match(metric, ign_gt, ign_det, thresholds, level, metric == 0)
        assert pr.shape == (41, 4) and np.array_equal(pr[:, :3], pr_h[:, :3]) and pr[:, 0].max() > 0
        assert np.allclose(pr[:, 3], pr_h[:, 3], rtol=1e-6, atol=0)


def test_edge_all_ground_truths_ignored_and_a_class_absent_everywhere():
    ev = E()
    z, gts, dts = load("match")
    for g in gts:
        g["occluded"][:] = 3                                                   # above every difficulty's limit
    ret = both(gts, dts, [0, 5], metrics=(1,))[0]
    assert all(len(th) == 0 for th, _ in ret["counts"].values()) and not ret["precision"].any()
    z, gts, dts = load("lidar")                                                # no Cyclist anywhere: the reference's zeros
    text, res = ev.get_official_eval_result(gts, dts, ["Cyclist"])
    host_text, host_res = ev.get_official_eval_result(gts, dts, ["Cyclist"], backend=C.HostBackend)
    assert text == host_text and res == host_res and res["Cyclist_3d/moderate_R40"] == 0.0


def test_edge_empty_inputs_return_without_a_launch():
    from toda_amd import ops
    i32 = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = ops.eval_overlaps(None, None, i32, None, None, i32, torch.zeros(1, dtype=torch.int64, device="cuda"), 0, 1, -1)
    assert out.numel() == 0
    ev = E()
    text, res = ev.get_official_eval_result([], [], ["Car"])
    assert res["Car_3d/easy_R40"] == 0.0


def _own_ground_truth(shift):
    from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    cfg = AttrDict()
    cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/models/second_backbone_nuscenes.yaml"), cfg)
    cfg.DATA_CONFIG.SYNTHETIC.NUM_POINTS, cfg.DATA_CONFIG.SYNTHETIC.NUM_SAMPLES = 3000, 8    # >= 41 boxes per class: fewer cannot fill the 41 recall points
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=False)
    annos = []
    for k, i in enumerate(ds.infos):
        boxes = np.asarray(i["gt_boxes"]).copy()
        boxes[:, :2] += shift
        annos.append({"frame_id": ds.frame_id(k), "name": np.array(i["gt_names"]), "score": np.ones(len(boxes)), "boxes_lidar": boxes})
    text, res = ds.evaluation(annos, cfg.CLASS_NAMES, eval_metric="kitti")
    assert "Car AP_R40@0.70, 0.70, 0.70:" in text and "Cyclist AP@" in text
    return res


def test_ground_truth_moved_by_one_centimetre_as_detections_scores_100():
    res = _own_ground_truth(0.01)
    for cls in ("Car", "Pedestrian", "Cyclist"):
        for kind in ("3d", "bev", "image"):
            assert res[f"{cls}_{kind}/moderate_R40"] == 100.0, (cls, kind)


def test_own_ground_truth_as_detections_scores_100():
    """The frames' own boxes as detections, bit for bit: every pair that matters is a box against itself."""
    res = _own_ground_truth(0.0)
    for cls in ("Car", "Pedestrian", "Cyclist"):
        for kind in ("3d", "bev", "image"):
            assert res[f"{cls}_{kind}/moderate_R40"] == 100.0, (cls, kind)


def test_eval_one_epoch_reports_finite_r40_keys(tmp_path):
    from toda_amd.tools import test as tester
    from toda_amd.tools import train as trainer
    cfg_file = os.path.join(ROOT, "toda_amd/tools/cfgs/models/toda_stage1_centerpoint_res.yaml")
    small = ["DATA_CONFIG.SYNTHETIC.NUM_SAMPLES", "4", "DATA_CONFIG.SYNTHETIC.NUM_POINTS", "20000",
             "DATA_CONFIG.POINT_CLOUD_RANGE", "[-21.6,-21.6,-5.0,21.6,21.6,4.8]",
             "MODEL.DENSE_HEAD.POST_PROCESSING.SCORE_THRESH", "0.0"]
    out = str(tmp_path / "out")
    trainer.main(["--cfg_file", cfg_file, "--epochs", "1", "--batch_size", "2", "--output_dir", out, "--fix_random_seed", "--set"] + small)
    ckpt = sorted((tmp_path / "out").rglob("checkpoint_epoch_1.pth"))[0]
    ret = tester.main(["--cfg_file", cfg_file, "--ckpt", str(ckpt), "--batch_size", "2", "--output_dir", out, "--set"] + small
                      + ["MODEL.POST_PROCESSING.EVAL_METRIC", "kitti"])
    keys = [k for k in ret if k.endswith("_R40")]
    assert "Car_3d/moderate_R40" in keys and "Car_bev/easy_R40" in keys and "car/recall_2m" not in ret
    assert all(np.isfinite(ret[k]) for k in keys)
