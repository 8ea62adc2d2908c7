"""Host side of the nuScenes mAP / NDS evaluator (eval_metric 'nds'): the curve stage against closed forms, the NaN rules, NDS
from its parts, the tables, the quaternion helpers, the JSON layouts, the entry points' argument checks without a device, and
the devkit route (eval_metric 'nuscenes') still raising ImportError."""
import json
import math

import numpy as np
import pytest

from tests import nusc_eval_cases as C


def E():
    from toda_amd.pcdet.datasets.nuscenes import nuscenes_eval
    return nuscenes_eval


def errs_of(n, **vals):
    return {m: np.asarray(vals.get(m, np.zeros(n)), np.float64) for m in E().TP_METRICS}


# ---- the curve stage against closed forms: one class, 10 ground truths
def test_ten_perfect_predictions():
    ev = E()
    c = ev.accumulate(np.ones(10, bool), np.linspace(0.95, 0.05, 10), errs_of(10), 10)
    assert abs(ev.calc_ap(c) - 1.0) <= 1e-12
    assert all(ev.calc_tp(c, m) == 0.0 for m in ev.TP_METRICS)


def test_alternating_tp_fp():
    """TP, FP, TP, FP, ...: the k-th TP lifts the precision to k / (2k - 1) at recall k / 10 and the FP after it drops it to 1 / 2 at
    the same recall; the issue's AP for this curve was computed independently on the CPU."""
    ev = E()
    c = ev.accumulate(np.arange(20) % 2 == 0, np.linspace(0.975, 0.025, 20), errs_of(20, trans_err=np.full(20, 0.25)), 10)
    assert abs(ev.calc_ap(c) - 0.47592376472665426) <= 1e-12
    assert abs(ev.calc_tp(c, "trans_err") - 0.25) <= 1e-12


def test_single_tp_reaches_recall_one_tenth_only():
    """Recall stops at exactly 0.1 = grid index 10: the precision beyond is 0, so AP is 0, and the last non-zero confidence index
    (10) lies below 11, so every error is 1."""
    ev = E()
    c = ev.accumulate(np.array([True]), np.array([0.9]), errs_of(1, trans_err=[0.3]), 10)
    assert ev.calc_ap(c) == 0.0
    assert np.count_nonzero(c["confidence"]) == 11 and ev.calc_tp(c, "trans_err") == 1.0


def test_two_tps():
    """Precision is 1 up to recall 0.2: 9 of the 90 entries from index 11 on are 0.9 after the subtraction: AP = 9 * 0.9 / 90 / 0.9
    = 1 / 9.  The cumulative mean goes 0.5 -> 1.0 over the confidences 0.9 -> 0.8; at grid index 10 + j the confidence is
    0.9 - 0.01 j, so the error is 0.5 + 0.05 j and its mean over j = 1 .. 10 is 0.775."""
    ev = E()
    c = ev.accumulate(np.array([True, True]), np.array([0.9, 0.8]), errs_of(2, trans_err=[0.5, 1.5]), 10)
    assert abs(ev.calc_ap(c) - 1 / 9) <= 1e-12
    assert abs(ev.calc_tp(c, "trans_err") - 0.775) <= 1e-12


def test_no_ground_truth_or_no_tp_gives_zeros_and_ones():
    ev = E()
    for c in (ev.accumulate(np.array([False, False]), np.array([0.9, 0.8]), errs_of(2), 10),
              ev.accumulate(np.array([True]), np.array([0.9]), errs_of(1), 0), ev.accumulate(np.zeros(0, bool), np.zeros(0), errs_of(0), 3)):
        assert not c["precision"].any() and not c["confidence"].any() and all((c[m] == 1).all() for m in ev.TP_METRICS)
        assert ev.calc_ap(c) == 0.0 and ev.calc_tp(c, "vel_err") == 1.0


def test_nan_aware_cumulative_mean():
    ev = E()
    nan = math.nan
    assert np.array_equal(ev.cummean([nan, nan, nan]), [1.0, 1.0, 1.0])
    assert np.array_equal(ev.cummean([nan, 2.0, nan, 4.0]), [0.0, 2.0, 2.0, 3.0])
    assert np.array_equal(ev.cummean([1.0, 2.0, 6.0]), [1.0, 1.5, 3.0])
    assert np.array_equal(ev.cummean([nan, 2.0, nan, 4.0]), C.cummean([nan, 2.0, nan, 4.0]))
    # a class whose TPs all lack the attribute: the attr curve is ones, so the error is 1
    c = ev.accumulate(np.ones(10, bool), np.linspace(0.95, 0.05, 10), errs_of(10, attr_err=np.full(10, nan)), 10)
    assert ev.calc_tp(c, "attr_err") == 1.0 and ev.calc_tp(c, "vel_err") == 0.0


def curves_with(ev, good):
    perfect = ev.accumulate(np.ones(10, bool), np.linspace(0.95, 0.05, 10), errs_of(10, trans_err=np.full(10, 0.5)), 10)
    return {(c, t): (perfect if c in good else ev.empty_curve()) for c in ev.CLASSES for t in ev.DIST_THS}


def test_nan_entries_and_nds_from_its_parts():
    ev = E()
    m = ev.summarise(curves_with(ev, ("car", "traffic_cone", "barrier")))
    for name, metric in (("traffic_cone", "attr_err"), ("traffic_cone", "vel_err"), ("traffic_cone", "orient_err"), ("barrier", "attr_err"), ("barrier", "vel_err")):
        assert math.isnan(m["label_tp_errors"][name][metric])
    assert sum(math.isnan(v) for per in m["label_tp_errors"].values() for v in per.values()) == 5
    assert m["label_tp_errors"]["barrier"]["orient_err"] == 0.0 and m["label_tp_errors"]["traffic_cone"]["trans_err"] == 0.5
    assert abs(m["mean_ap"] - 0.3) <= 1e-12 and abs(m["mean_dist_aps"]["car"] - 1.0) <= 1e-12
    # trans: three classes at 0.5, seven at 1; scale: 3 x 0 + 7 x 1; orient: cone out, car and barrier 0, seven 1; vel and attr: car 0, seven 1
    want = {"trans_err": (3 * 0.5 + 7) / 10, "scale_err": 0.7, "orient_err": 7 / 9, "vel_err": 7 / 8, "attr_err": 7 / 8}
    for k, v in want.items():
        assert abs(m["tp_errors"][k] - v) <= 1e-12 and abs(m["tp_scores"][k] - (1 - v)) <= 1e-12
    assert abs(m["nd_score"] - (5 * 0.3 + sum(1 - v for v in want.values())) / 10) <= 1e-12
    assert ev.nd_score(1.0, {k: 1.0 for k in ev.TP_METRICS}) == 1.0
    assert ev.nd_score(0.0, {"a": 0.0}) == 0.0
    # an error above 1 scores 0, not a negative number
    worse = curves_with(ev, ev.CLASSES)
    for key in worse:
        worse[key] = dict(worse[key], trans_err=np.full(101, 1.5))
    assert ev.summarise(worse)["tp_scores"]["trans_err"] == 0.0


def test_restatement_and_evaluator_agree_on_the_curve_stage():
    ev = E()
    rng = np.random.default_rng(3)
    for npos in (1, 7, 40):
        n = 60
        tp = rng.random(n) < 0.5
        conf = np.sort(np.round(rng.uniform(0.05, 1, n) * 32) / 32)[::-1]
        errs = rng.uniform(0, 2, (5, n))
        errs[1, rng.random(n) < 0.3] = math.nan
        tp[np.cumsum(tp) > npos] = False
        got = ev.accumulate(tp, conf, {m: errs[ev.ERR_ROW[m]] for m in ev.TP_METRICS}, npos)
        precision, confidence, curves = C.curve(list(tp), list(conf), [list(errs[:, k]) for k in range(n)], npos)
        assert abs(ev.calc_ap(got) - C.ap_of(precision)) <= 1e-12
        for m in ev.TP_METRICS:
            assert abs(ev.calc_tp(got, m) - C.tp_of(confidence, curves[m])) <= 1e-12


# ---- tables, rotations, JSON
def test_tables_load_and_a_missing_one_is_named(tmp_path):
    ev = E()
    root, infos = C.write_tree(tmp_path)
    attr_of, racks = ev.annotation_index(ev.load_tables(root, C.VERSION))
    assert attr_of["ann0_0"] == "vehicle.moving" and attr_of["ann0_2"] == "" and attr_of["ann1_1"] == "vehicle.stopped"
    assert list(racks) == ["sample0"] and len(racks["sample0"]) == 1
    trans, wlh, R = racks["sample0"][0]
    assert np.allclose(wlh, [2.0, 6.0, 1.5]) and np.allclose(R @ R.T, np.eye(3), atol=1e-12)
    # the bicycle of sample 0 stands in the rack, the closed test takes a point on the rack's face, and a point beyond is out
    G = np.linalg.inv(infos[0]["car_from_global"]) @ np.linalg.inv(infos[0]["ref_from_car"])
    to_global = lambda p: G[:3, :3] @ np.asarray(p, np.float64) + G[:3, 3]      # noqa: E731
    h = C.RACK_OF_SAMPLE_0[6]
    along = np.array([math.cos(h), math.sin(h), 0.0])
    centre = np.array(C.RACK_OF_SAMPLE_0[:3])
    pts = [to_global([12.0, 14.0, -1.2]), to_global(centre + 2.5 * along), to_global(centre + 3.5 * along), to_global(centre + [0, 0, 0.8])]
    assert list(ev.in_racks(pts, racks["sample0"])) == [True, True, False, False]
    assert list(ev.in_racks(np.array([[0.0, 0.0, 0.75], [0.0, 1.0, 0.0], [0.0, 1.0 + 1e-9, 0.0]]), [(np.zeros(3), np.array([2.0, 6.0, 1.5]), np.eye(3))])) == [True, True, False]
    (root / C.VERSION / "instance.json").unlink()
    with pytest.raises(FileNotFoundError, match="instance.json"):
        ev.load_tables(root, C.VERSION)


def test_quaternion_helpers_round_trip():
    ev = E()
    rng = np.random.default_rng(0)
    qs = [q / np.linalg.norm(q) for q in rng.standard_normal((50, 4))]
    qs += [np.array(q, np.float64) for q in ([1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0.5, 0.5, -0.5, 0.5], [1e-9, 0, 0, 1])]
    for q in qs:
        q = q / np.linalg.norm(q)
        R = ev.quat_to_matrix(q)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1) <= 1e-14
        back = ev.matrix_to_quat(R)
        assert back[0] >= 0 and min(np.abs(back - q).max(), np.abs(back + q).max()) <= 1e-12
        assert np.allclose(R, C.quat_matrix(list(q)), atol=1e-15)
    assert np.allclose(ev.matrix_to_quat(ev.rot_z(0.7)), [math.cos(0.35), 0, 0, math.sin(0.35)], atol=1e-15)


def test_prediction_attributes():
    ev = E()
    assert ev.prediction_attribute("car", 0.21) == "vehicle.moving" and ev.prediction_attribute("car", 0.2) == "vehicle.parked"
    assert ev.prediction_attribute("bus", 0.0) == "vehicle.stopped" and ev.prediction_attribute("bus", 3.0) == "vehicle.moving"
    assert ev.prediction_attribute("bicycle", 1.0) == "cycle.with_rider" and ev.prediction_attribute("motorcycle", 0.0) == "cycle.without_rider"
    assert ev.prediction_attribute("pedestrian", 0.1) == "pedestrian.standing" and ev.prediction_attribute("pedestrian", 1.0) == "pedestrian.moving"
    assert ev.prediction_attribute("barrier", 5.0) == "" and ev.prediction_attribute("traffic_cone", 0.0) == ""
    assert ev.prediction_attribute("pedestrian", math.nan) == "pedestrian.standing"
    for name in ev.CLASSES:
        for speed in (0.0, 1.0):
            assert ev.prediction_attribute(name, speed) == C.stated_attribute(name, speed)


def test_json_layouts(tmp_path):
    ev = E()
    m = ev.summarise(curves_with(ev, ("car",)), eval_time=1.5)
    assert list(m) == ["label_aps", "label_tp_errors", "mean_dist_aps", "mean_ap", "tp_errors", "tp_scores", "nd_score", "eval_time"]
    assert list(m["label_aps"]) == list(ev.CLASSES) and list(m["label_aps"]["car"]) == ["0.5", "1.0", "2.0", "4.0"]
    assert list(m["label_tp_errors"]["bus"]) == list(ev.TP_METRICS) == list(m["tp_errors"]) == list(m["tp_scores"])
    back = json.loads(json.dumps(m))
    assert back["nd_score"] == m["nd_score"] and math.isnan(back["label_tp_errors"]["barrier"]["vel_err"])
    text, details = ev.format_results(m, ["car", "barrier"])
    assert list(details) == list(ev.TP_METRICS) + ["mAP", "NDS"] and details["NDS"] == m["nd_score"]
    lines = text.splitlines()
    assert lines[0] == "----------------Nuscene detection_cvpr_2019 results-----------------"
    assert lines[1] == "***car error@trans, scale, orient, vel, attr | AP@0.5, 1.0, 2.0, 4.0"
    assert lines[2].startswith("0.50, 0.00, 0.00, 0.00, 0.00 | 100.00, 100.00, 100.00, 100.00 | mean AP: ")
    assert lines[4].startswith("1.00, 1.00, 1.00, nan, nan | 0.00, 0.00, 0.00, 0.00 | mean AP: 0.0")
    assert lines[5] == "--------------average performance-------------" and lines[-2].startswith("mAP:\t 0.1000") and lines[-1].startswith("NDS:\t ")
    # the submission block: w, l, h sizes, the w x y z quaternion of R . Rz(heading), two velocity components
    R = ev.quat_to_matrix([math.cos(0.1), 0, 0, math.sin(0.1)])
    glob = np.array([[1.0, 2.0, 3.0, 0.5, 0.3, -0.4], [4.0, 5.0, 6.0, 0.0, 0.0, 0.0]])
    rows = np.array([[0, 0, 0, 4.0, 2.0, 1.5, 0.3], [0, 0, 0, 1.0, 0.5, 1.8, -0.2]])
    res = ev.submission_results(["a", "b"], [2, 0], glob, rows, np.stack([R, R]), ["car", "pedestrian"], [0.75, 0.5], ["vehicle.moving", "pedestrian.standing"])
    assert list(res) == ["a", "b"] and res["b"] == [] and len(res["a"]) == 2
    box = json.loads(json.dumps(res))["a"][0]
    assert sorted(box) == sorted(["sample_token", "translation", "size", "rotation", "velocity", "detection_name", "detection_score", "attribute_name"])
    assert box["sample_token"] == "a" and box["translation"] == [1.0, 2.0, 3.0] and box["size"] == [2.0, 4.0, 1.5] and box["velocity"] == [0.3, -0.4]
    assert np.allclose(box["rotation"], [math.cos(0.25), 0, 0, math.sin(0.25)], atol=1e-15)       # 0.2 rad of R and the heading 0.3
    assert box["detection_name"] == "car" and box["detection_score"] == 0.75 and box["attribute_name"] == "vehicle.moving"


def test_constants_agree_between_the_layers():
    from toda_amd import ops
    ev = E()
    assert tuple(ops.NUSC_CLASSES) == tuple(ev.CLASSES) == tuple(C.CLASSES) and tuple(ops.NUSC_DIST_THS) == tuple(ev.DIST_THS)
    assert ops.NUSC_MAX_PRED == ev.MAX_BOXES_PER_SAMPLE == 500 and ops.NUSC_MAX_GT >= 2048
    assert ev.DIST_THS.index(ev.DIST_TH_TP) == 2


# ---- the C ABI without a device
def test_entry_points_reject_bad_arguments_without_a_device():
    import torch

    from toda_amd import lib as L
    from toda_amd import ops
    lib = L.load()
    assert lib.toda_abi_version() == 3
    one = L.hptr(L.host_f64([0.0] * 16))
    assert lib.toda_nusc_eval_prepare(None, None, None, 0, None, None, 0, None, None, None) == 0            # nothing to do, no pointer read
    assert lib.toda_nusc_eval_prepare(None, None, None, -1, None, None, 0, None, None, None) == -1 and b"negative" in lib.toda_last_error()
    assert lib.toda_nusc_eval_prepare(None, one, one, 4, one, one, 1, one, one, None) == -1 and b"null" in lib.toda_last_error()
    assert lib.toda_nusc_eval_prepare(one, one, one, 4, None, one, 1, one, one, None) == -1 and b"null transforms" in lib.toda_last_error()
    assert lib.toda_nusc_eval_match_workspace_bytes(0) == 0 and lib.toda_nusc_eval_match_workspace_bytes(10) >= (11 + 11 + 10) * 4
    ths = L.hptr(L.host_f64([0.5, 1.0, 2.0, 4.0]))

    def match(n_pred, n_gt, pred_off, gt_off, cls, tp=2, ws_bytes=1 << 20, pred=one, out=one):
        return lib.toda_nusc_eval_match(pred, one, one, n_pred, one, one, n_gt, L.hptr(L.host_i32(pred_off)), L.hptr(L.host_i32(gt_off)),
                                        L.hptr(L.host_i32(cls)), len(cls), ths, tp, out, one, one, ws_bytes, None)
    assert lib.toda_nusc_eval_match(*([None] * 3), 0, None, None, 0, None, None, None, 0, None, 2, None, None, None, 0, None) == 0
    assert lib.toda_nusc_eval_match(*([None] * 3), 0, None, None, 7, None, None, None, 3, None, 2, None, None, None, 0, None) == 0     # no predictions
    assert match(-1, 0, [0, 0], [0, 0], [0]) == -1 and b"negative" in lib.toda_last_error()
    assert match(5, 0, [0, 5], [0, 0], [0], pred=None) == -1 and b"null" in lib.toda_last_error()
    assert match(5, 0, [0, 5], [0, 0], [0], out=None) == -1 and b"null" in lib.toda_last_error()
    assert match(501, 3, [0, 501], [0, 3], [0]) == -1 and b"501 predictions" in lib.toda_last_error()
    assert match(5, 2049, [0, 5], [0, 2049], [0]) == -1 and b"2049 ground truths" in lib.toda_last_error()
    assert match(5, 3, [0, 6, 5], [0, 1, 3], [0, 1]) == -1 and b"descend" in lib.toda_last_error()
    assert match(5, 3, [0, 4], [0, 3], [0]) == -1 and b"offsets" in lib.toda_last_error()
    assert match(5, 3, [0, 5], [0, 3], [10]) == -1 and b"class" in lib.toda_last_error()
    assert match(5, 3, [0, 5], [0, 3], [0], tp=4) == -1 and b"tp_threshold" in lib.toda_last_error()
    assert match(5, 3, [0, 5], [0, 3], [0], ws_bytes=8) == -1 and b"workspace" in lib.toda_last_error()
    with pytest.raises(RuntimeError, match="GPU"):
        ops.nusc_eval_prepare(torch.zeros((1, 10), dtype=torch.float64), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                              torch.zeros((1, 3, 4), dtype=torch.float64), torch.zeros((1, 3), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.nusc_eval_match(torch.zeros((1, 8), dtype=torch.float64), torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int32),
                            torch.zeros((0, 8), dtype=torch.float64), torch.zeros(0, dtype=torch.int32), [0, 1], [0, 0], [0])


# ---- wiring
def test_the_devkit_route_still_raises_and_nds_checks_its_inputs_first(tmp_path):
    from toda_amd.pcdet.datasets.nuscenes.nuscenes_dataset import NuScenesDataset
    C.write_tree(tmp_path)
    ds = NuScenesDataset(C.dataset_cfg(tmp_path), C.CLASSES, training=False)
    dets = C.perfect_detections(ds.infos)
    with pytest.raises(ImportError, match="nuscenes-devkit"):
        ds.evaluation(dets, C.CLASSES, eval_metric="nuscenes", output_path=str(tmp_path / "out"))
    with pytest.raises(NotImplementedError, match="nds"):
        ds.evaluation(dets, C.CLASSES, eval_metric="waymo")
    # refused before anything reaches the device
    with pytest.raises(ValueError, match="output_path"):
        ds.evaluation(dets, C.CLASSES, eval_metric="nds")
    with pytest.raises(ValueError, match="exactly"):
        ds.evaluation(dets[:2], C.CLASSES, eval_metric="nds", output_path=str(tmp_path / "out"))
    renamed = [dict(d, metadata={"token": "other"}) if k == 1 else d for k, d in enumerate(dets)]
    with pytest.raises(ValueError, match="other"):
        ds.evaluation(renamed, C.CLASSES, eval_metric="nds", output_path=str(tmp_path / "out"))
    with pytest.raises(ValueError, match="exactly"):
        ds.evaluation(dets + dets[:1], C.CLASSES, eval_metric="nds", output_path=str(tmp_path / "out"))
    many = dict(dets[2], name=np.array(["car"] * 501), score=np.full(501, 0.5), boxes_lidar=np.zeros((501, 9)))
    with pytest.raises(ValueError, match="sample2.*501"):
        ds.evaluation(dets[:2] + [many], C.CLASSES, eval_metric="nds", output_path=str(tmp_path / "out"))
    assert not (tmp_path / "out" / "results_nusc.json").exists()


def test_infos_without_the_two_poses_are_refused(tmp_path):
    from toda_amd.pcdet.datasets.nuscenes.nuscenes_dataset import NuScenesDataset
    C.write_tree(tmp_path, with_poses=False)
    ds = NuScenesDataset(C.dataset_cfg(tmp_path), C.CLASSES, training=False)
    with pytest.raises(KeyError, match="ref_from_car.*car_from_global"):
        ds.evaluation(C.perfect_detections(ds.infos), C.CLASSES, eval_metric="nds", output_path=str(tmp_path / "out"))
