"""The Lyft mAP on the MI355X: ops.lyft_eval_best, ops.lyft_eval_flags (csrc/lyft_eval.hip) and lyft_eval.evaluate against the
numpy / Python restatement of the reference (tests/lyft_eval_cases.py).

Pass criteria: the argmax and every TP flag exactly, the largest IoU within 1e-12 absolute (both sides clip the same fp64
corners; only the order of the operations differs), AP per class and cut-off within 1e-9 (the summation order over equal integer
ratios).  The exact checks are valid away from rounding edges, so they rest on a condition taken on the restatement's own numbers
(lyft_eval_cases.away_from_edges): every |largest IoU - cut-off| and every gap to a different runner-up exceeds 1e-9.  The worlds'
seeds are chosen so that the condition holds for every prediction; nothing is left out."""
import json

import numpy as np
import pytest
import torch

from tests import lyft_eval_cases as C
from toda_amd import lib as L
from toda_amd import ops
from toda_amd.pcdet.datasets.lyft import lyft_eval as E

pytestmark = pytest.mark.gpu


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


@pytest.fixture(scope="module")
def edge():
    """The edge world, its restatement (computed once, read by every test) and its segments."""
    built = C.build(C.edge_world())
    built["avg"], built["per_cut"], built["seen"] = C.get_average_precisions(built["gt"], built["pred"], C.CLASSES, C.THRESHOLDS)
    built["seg"] = E.segment(built["infos"], built["det_annos"], C.CLASSES, E.ground_truth_rows(built["tables"]))
    built["uids"] = C.segment_uids(built["det_annos"], C.CLASSES)
    return built


def run_kernels(seg, thresholds=C.THRESHOLDS):
    best_iou, best_gt = ops.lyft_eval_best(dev(seg["pred"], np.float64), dev(seg["gt"], np.float64), seg["pred_off"], seg["gt_off"])
    tp = ops.lyft_eval_flags(dev(seg["pred_score"], np.float64), best_iou, best_gt, seg["pred_off"], thresholds)
    return best_iou.cpu().numpy(), best_gt.cpu().numpy(), tp.cpu().numpy()


def test_the_edge_world_holds_the_shapes_it_promises(edge):
    seg = edge["seg"]
    n_pred, n_gt = np.diff(seg["pred_off"]).tolist(), np.diff(seg["gt_off"]).tolist()
    chunk = L.load().toda_lyft_eval_flags_chunk()
    assert {0, 1, 63, 64, 65} <= set(n_gt) and {1, 65, chunk + 1} <= set(n_pred)
    assert (3, 0) in set(zip(n_pred, n_gt))                                       # truck in s0: predictions, no ground truth there
    assert seg["n_gt"][C.CLASSES.index("animal")] == 0 and seg["n_gt"][C.CLASSES.index("truck")] > 0
    assert C.CLASSES.index("bicycle") not in seg["pred_cls"] and seg["n_gt"][C.CLASSES.index("bicycle")] == 3
    assert len(edge["det_annos"][3]["name"]) == 0 and len(edge["det_annos"][4]["name"]) == 0          # 0 predictions
    assert C.away_from_edges(edge["seen"])
    scores = seg["pred_score"]
    assert len(np.unique(scores[:seg["pred_off"][1]])) < seg["pred_off"][1]       # equal scores within a segment
    norms = seg["pred"][:, 3] ** 2 + seg["pred"][:, 4] ** 2
    assert (norms < 0.95).any() and (np.abs(norms - 1) < 1e-12).any()             # tilted and level poses


def test_best_iou_argmax_and_flags_equal_the_restatement(edge):
    seg, seen = edge["seg"], edge["seen"]
    best_iou, best_gt, tp = run_kernels(seg)
    assert best_iou.dtype == np.float64 and best_gt.dtype == np.int32 and tp.dtype == np.uint8 and tp.shape == (10, len(edge["uids"]))
    worst, walked, twins, both_sides = 0.0, 0, 0, 0
    for k, uid in enumerate(edge["uids"]):
        cls = seg["pred_cls"][k]
        if uid not in seen:                      # a class with no ground truth anywhere: the reference does not walk it
            assert seg["n_gt"][cls] == 0 and best_gt[k] == -1 and best_iou[k] == -np.inf and not tp[:, k].any()
            continue
        overlaps, best, jmax, flags = seen[uid]
        walked += 1
        assert best_gt[k] == jmax, (uid, best_gt[k], jmax)
        if jmax < 0:                             # this sample has no ground truth of the class
            assert best_iou[k] == -np.inf and not tp[:, k].any()
            continue
        worst = max(worst, abs(best_iou[k] - best))
        assert tp[:, k].tolist() == flags.tolist(), uid
        twins += overlaps.count(best) > 1 and best > 0
        both_sides += 0 < flags.sum() < len(flags)
    print(f"max |best_iou - restatement| = {worst:.3e} over {walked} predictions; {twins} argmax ties, {both_sides} predictions TP at some cut-offs only")
    assert worst < 1e-12
    assert twins >= 3 and both_sides >= 10


def test_several_predictions_on_one_ground_truth_straddle_the_cutoffs(edge):
    """s1 / car: 257 predictions on 10 ground truths.  For every ground truth the TPs at cut-off t are exactly the first prediction in
    (score descending, position) order among those with that argmax and IoU > t."""
    seg = edge["seg"]
    best_iou, best_gt, tp = run_kernels(seg)
    s = np.diff(seg["pred_off"]).tolist().index(257)
    p0, p1 = seg["pred_off"][s], seg["pred_off"][s + 1]
    order = np.argsort(-seg["pred_score"][p0:p1], kind="stable")
    claimed = 0
    for j in range(10):
        for t, thr in enumerate(C.THRESHOLDS):
            over = [p for p in order if best_gt[p0 + p] == j and best_iou[p0 + p] > thr]
            want = np.zeros(p1 - p0, np.uint8)
            if over:
                want[over[0]] = 1
            mine = best_gt[p0:p1] == j
            assert np.array_equal(tp[t, p0:p1][mine], want[mine])
            claimed += len(over) > 1
    assert claimed >= 20


def test_equal_scores_and_twins_in_a_hand_built_segment():
    """One segment, three identical ground truths and one apart; five predictions of equal score on the twins' place and one on the
    fourth.  The argmax is the first twin for all five, so only the earliest of them is a TP, the twins stay unclaimed."""
    g = np.array([[10, 5, 0, 1, 0, 2, 4, 1.5]] * 3 + [[40, 5, 0, 0, 1, 2, 4, 1.5]], np.float64)
    p = np.concatenate([g[[0] * 5], g[[3]]]).copy()
    p[:5, 0] += np.array([0.4, 0.1, 0.2, 0.0, 0.3])                              # IoU (4 - d) / (4 + d): 0.818 0.951 0.905 1 0.860
    score = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5])
    seg = {"pred": p, "gt": g, "pred_score": score, "pred_off": np.array([0, 6], np.int32), "gt_off": np.array([0, 4], np.int32)}
    best_iou, best_gt, tp = run_kernels(seg)
    assert best_gt.tolist() == [0, 0, 0, 0, 0, 3]
    d = np.array([0.4, 0.1, 0.2, 0.0, 0.3])
    assert np.abs(best_iou[:5] - (4 - d) / (4 + d)).max() < 1e-12 and abs(best_iou[5] - 1) < 1e-12
    # prediction 0 (IoU 0.818) claims the twin up to 0.8; above it the next in position with a larger IoU does: 1 (0.951) up to 0.95
    want = np.zeros((10, 6), np.uint8)
    want[:7, 0] = 1                                                               # 0.5 .. 0.8
    want[7:, 1] = 1                                                               # 0.85, 0.9, 0.95 (0.951 > 0.95)
    want[:, 5] = 1
    assert np.array_equal(tp, want)
    # the same with descending scores in reverse position: the order is by score first
    seg["pred_score"] = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.5])
    _, _, tp = run_kernels(seg)
    want = np.zeros((10, 6), np.uint8)
    want[:8, 4] = 1                                                               # 4 (0.860) first: 0.5 .. 0.85
    want[8:, 3] = 1                                                               # then 3 (IoU 1): 0.9, 0.95
    want[:, 5] = 1
    assert np.array_equal(tp, want)


def test_evaluate_equals_the_restatement_per_class_and_cutoff(edge, tmp_path):
    aps = E.class_aps(edge["seg"], C.THRESHOLDS, len(C.CLASSES))
    diff = np.abs(aps - edge["per_cut"]).max()
    print("AP per class and cut-off (device):\n", np.round(aps, 4), "\nmax |AP - restatement| =", diff)
    assert diff < 1e-9
    assert (aps[C.CLASSES.index("animal")] == -1).all() and (aps[C.CLASSES.index("other_vehicle")] == -1).all()     # predictions, no ground truth
    assert (aps[C.CLASSES.index("bicycle")] == 0).all() and (aps[C.CLASSES.index("bus")] == 0).all()               # ground truth, no predictions
    assert aps[C.CLASSES.index("car")].max() > 0.1 and aps[C.CLASSES.index("motorcycle")].max() > 0.1
    (tmp_path / "data").mkdir()
    for name, records in edge["tables"].items():
        with open(tmp_path / "data" / f"{name}.json", "w") as f:
            json.dump(records, f)
    text, res = E.evaluate(edge["infos"], edge["det_annos"], C.CLASSES, tmp_path, C.THRESHOLDS, version="one_scene")
    assert text.startswith("----------------Lyft one_scene results-----------------\n") and text.count("\n") == 2 + 9 + 2
    assert np.abs(np.array([res[c] for c in C.CLASSES]) - edge["avg"]).max() < 1e-9 and abs(res["mAP"] - edge["avg"].mean()) < 1e-9
    assert res["animal"] == -1.0 and res["mAP"] < res["car"]                      # the -1 classes pull the mean down, as in the reference
    host = E.class_aps(edge["seg"], C.THRESHOLDS, len(C.CLASSES), route="host")
    assert np.abs(host - aps).max() < 1e-9


def test_two_runs_give_the_same_bits(edge):
    a, b = run_kernels(edge["seg"]), run_kernels(edge["seg"])
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert E.class_aps(edge["seg"], C.THRESHOLDS, len(C.CLASSES)).tobytes() == E.class_aps(edge["seg"], C.THRESHOLDS, len(C.CLASSES)).tobytes()


def test_empty_sides_and_refused_arguments_launch_nothing():
    sentinel = -7.0
    none = torch.zeros((0, 8), dtype=torch.float64, device="cuda")
    best_iou, best_gt = ops.lyft_eval_best(none, none, [0], [0])
    assert best_iou.shape == (0,) and best_gt.shape == (0,)
    assert ops.lyft_eval_flags(torch.zeros(0, dtype=torch.float64, device="cuda"), best_iou, best_gt, [0, 0, 0], [0.5, 0.7]).shape == (2, 0)
    rows = torch.ones((3, 8), dtype=torch.float64, device="cuda")
    best_iou, best_gt = ops.lyft_eval_best(rows, none, [0, 2, 3], [0, 0, 0])      # predictions, no ground truth at all
    assert best_gt.tolist() == [-1, -1, -1] and torch.isinf(best_iou).all() and (best_iou < 0).all()
    with pytest.raises(RuntimeError, match="must run from 0 to 3"):
        ops.lyft_eval_best(rows, rows, [0, 2], [0, 3])
    with pytest.raises(RuntimeError, match=r"\[\., 8\]"):
        ops.lyft_eval_best(rows[:, :7].contiguous(), rows, [0, 3], [0, 3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lyft_eval_best(rows.cpu(), rows, [0, 3], [0, 3])
    score = torch.ones(3, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="cut-offs"):
        ops.lyft_eval_flags(score, score, torch.zeros(3, dtype=torch.int32, device="cuda"), [0, 3], [0.5] * 17)
    with pytest.raises(RuntimeError, match="float64"):
        ops.lyft_eval_flags(score.float(), score, torch.zeros(3, dtype=torch.int32, device="cuda"), [0, 3])
    # a refused call leaves its output alone
    lib = L.load()
    out = torch.full((3,), sentinel, dtype=torch.float64, device="cuda")
    idx = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    bad = L.host_i32([0, 4])
    rc = lib.toda_lyft_eval_best(L.ptr(rows), 3, L.ptr(rows), 3, L.hptr(bad), L.hptr(bad), 1, L.ptr(out), L.ptr(idx), L.ptr(ws), 4096, L.stream())
    torch.cuda.synchronize()
    assert rc == -1 and (out == sentinel).all() and (idx == -7).all()
