"""Shared by tests/test_waymo_eval_host.py and tests/test_gpu_waymo_eval.py: the Waymo LEVEL_1 / LEVEL_2 AP and APH metric of
DESIGN.md 3.15 restated in plain Python floats and loops (no code shared with toda_amd), and the case generators.

The IoU is convex clipping in Python floats, statement for statement the arithmetic the definition names, so values on a binary
grid come out bit-equal.  The matching is scipy.optimize.linear_sum_assignment(maximize=True), solved afresh for every distinct
active set on the integer weights padded with one zero column per active prediction."""
import math

import numpy as np
from scipy.optimize import linear_sum_assignment

WAYMO_CLASSES = ["unknown", "Vehicle", "Pedestrian", "Truck", "Cyclist"]
KEY_TYPES = ["VEHICLE", "PEDESTRIAN", "SIGN", "CYCLIST"]           # estimator types 1..4
KEYS = ["OBJECT_TYPE_TYPE_%s_LEVEL_%d/%s" % (t, lv, m) for t in KEY_TYPES for lv in (1, 2) for m in ("AP", "APH")]
N_CUT = 101
TWO_PI = 2 * math.pi


def cutoffs():
    return [float(np.float32(k * 0.01)) for k in range(100)] + [1.0]


def type_threshold(t):
    return 0.7 if t == 1 else 0.5


# ---- IoU ---------------------------------------------------------------------------------------------------------------------
def clip(poly, axis, sign, lim):
    """The part of a convex polygon with sign * coordinate[axis] <= lim."""
    out = []
    n = len(poly)
    for i in range(n):
        p, q = poly[i], poly[(i + 1) % n]
        pc, qc = sign * p[axis], sign * q[axis]
        pin, qin = pc <= lim, qc <= lim
        if pin:
            out.append((p[0], p[1]))
        if pin != qin:
            t = (lim - pc) / (qc - pc)
            o = 1 - axis
            v = [0.0, 0.0]
            v[axis] = sign * lim
            v[o] = p[o] + t * (q[o] - p[o])
            out.append((v[0], v[1]))
    return out


def iou_3d(a, b):
    """7-DOF IoU of two boxes x y z dx dy dz heading: a's rectangle in b's frame, clipped by b's four half-planes."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    ca, sa, cb, sb = math.cos(a[6]), math.sin(a[6]), math.cos(b[6]), math.sin(b[6])
    hx, hy = a[3] / 2, a[4] / 2
    poly = []
    for sx, sy in ((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0)):
        lx, ly = sx * hx, sy * hy
        rx, ry = (a[0] + (lx * ca - ly * sa)) - b[0], (a[1] + (lx * sa + ly * ca)) - b[1]
        poly.append((rx * cb + ry * sb, ry * cb - rx * sb))
    bx, by = b[3] / 2, b[4] / 2
    for axis, sign, lim in ((0, 1.0, bx), (0, -1.0, bx), (1, 1.0, by), (1, -1.0, by)):
        poly = clip(poly, axis, sign, lim)
    area = 0.0
    if len(poly) >= 3:
        acc = 0.0
        for i in range(len(poly)):
            p, q = poly[i], poly[(i + 1) % len(poly)]
            acc += p[0] * q[1] - q[0] * p[1]
        area = abs(acc) / 2
    zlo, zhi = max(a[2] - a[5] / 2, b[2] - b[5] / 2), min(a[2] + a[5] / 2, b[2] + b[5] / 2)
    inter = area * max(zhi - zlo, 0.0)
    den = ((a[3] * a[4]) * a[5] + (b[3] * b[4]) * b[5]) - inter
    if not den > 0.0:
        return 0.0
    return min(max(inter / den, 0.0), 1.0)


def iou_block(pred, gt):
    return np.array([[iou_3d(p, g) for g in gt] for p in pred], np.float64).reshape(len(pred), len(gt))


def weights_of(iou, seg_type):
    t = type_threshold(seg_type)
    return np.array([[int(v * 1000) if v >= t else 0 for v in row] for row in np.asarray(iou, np.float64)], np.int64).reshape(np.shape(iou))


# ---- matching ----------------------------------------------------------------------------------------------------------------
def solve(w):
    """Maximum-weight assignment of the rows of w [n, m] (ints): (column of each row or -1 when it carries no weight, total)."""
    n, m = w.shape
    if n == 0:
        return [], 0
    padded = np.concatenate([w, np.zeros((n, n), np.int64)], 1)
    rows, cols = linear_sum_assignment(padded, maximize=True)
    assign = [-1] * n
    for r, c in zip(rows, cols):
        if c < m and w[r, c] > 0:
            assign[r] = int(c)
    return assign, int(padded[rows, cols].sum())


def active_sets(score):
    """For each of the 101 cutoffs the positions of the predictions with fp32(score) >= cutoff."""
    s32 = [float(np.float32(s)) for s in score]
    return [[i for i, s in enumerate(s32) if s >= c] for c in cutoffs()]


def match_segment(w, score):
    """-> (assign [101][n_pred]: ground truth of each prediction at each cutoff, -1 unmatched or inactive; total [101])."""
    n = len(score)
    w = np.asarray(w, np.int64)
    solved = {}
    table, totals = [], []
    for act in active_sets(score):
        key = tuple(act)
        if key not in solved:
            solved[key] = solve(w[act])
        sub, total = solved[key]
        row = [-1] * n
        for i, c in zip(act, sub):
            row[i] = c
        table.append(row)
        totals.append(total)
    return table, totals


def heading_accuracy(a, b):
    d = math.fmod(abs(a - b), TWO_PI)
    return 1.0 - min(d, TWO_PI - d) / math.pi


def count_segment(table, score, level, pred_heading, gt_heading):
    """-> tp [2][101], fn [2][101], fp [101], sum_ha [2][101] of one segment from its match table."""
    acts = active_sets(score)
    tp = [[0] * N_CUT for _ in range(2)]
    fn = [[0] * N_CUT for _ in range(2)]
    fp = [0] * N_CUT
    ha = [[0.0] * N_CUT for _ in range(2)]
    for k in range(N_CUT):
        row = table[k]
        matched = {c: i for i, c in enumerate(row) if c >= 0}
        fp[k] = sum(1 for i in acts[k] if row[i] < 0)
        for lv in (1, 2):
            for g in range(len(level)):
                if level[g] > lv:
                    continue
                if g in matched:
                    tp[lv - 1][k] += 1
                    ha[lv - 1][k] += heading_accuracy(float(pred_heading[matched[g]]), float(gt_heading[g]))
                else:
                    fn[lv - 1][k] += 1
    return tp, fn, fp, ha


def expect_counts(segments):
    """segments: [(type, iou [n, m], score [n], pred_heading [n], gt_heading [m], level [m])] -> (tp [4, 2, 101], fn, fp [4, 101],
    sum_ha [4, 2, 101], tables: per segment [101][n], totals: per segment [101])."""
    tp, fn = np.zeros((4, 2, N_CUT), np.int64), np.zeros((4, 2, N_CUT), np.int64)
    fp, ha = np.zeros((4, N_CUT), np.int64), np.zeros((4, 2, N_CUT), np.float64)
    tables, totals = [], []
    for t, iou, score, ph, gh, level in segments:
        table, total = match_segment(weights_of(np.asarray(iou).reshape(len(score), len(level)), t), score)
        a, b, c, d = count_segment(table, score, level, ph, gh)
        tp[t - 1] += np.array(a)
        fn[t - 1] += np.array(b)
        fp[t - 1] += np.array(c)
        ha[t - 1] += np.array(d)
        tables.append(table)
        totals.append(total)
    return tp, fn, fp, ha, tables, totals


# ---- curves ------------------------------------------------------------------------------------------------------------------
def ratio(a, b):
    return a / b if b != 0 else 0.0


def average_precision(precision, recall):
    pts = sorted(zip(recall, precision), key=lambda pr: -pr[0]) + [(0.0, 0.0)]
    ap, best = 0.0, 0.0
    for k in range(len(pts) - 1):
        best = max(best, pts[k][1])
        ap += (pts[k][0] - pts[k + 1][0]) * best
    return ap


def scores_of(tp, fn, fp, ha):
    """Counts [4, 2, 101] / [4, 101] -> {key: value} of the 16 numbers, in the order of KEYS."""
    out = {}
    for t in range(4):
        for lv in range(2):
            a, b, c, h = [float(v) for v in tp[t][lv]], [float(v) for v in fn[t][lv]], [float(v) for v in fp[t]], [float(v) for v in ha[t][lv]]
            ap = average_precision([ratio(a[k], a[k] + c[k]) for k in range(N_CUT)], [ratio(a[k], a[k] + b[k]) for k in range(N_CUT)])
            aph = average_precision([ratio(h[k], a[k] + c[k]) for k in range(N_CUT)], [ratio(h[k], a[k] + b[k]) for k in range(N_CUT)])
            out["OBJECT_TYPE_TYPE_%s_LEVEL_%d/AP" % (KEY_TYPES[t], lv + 1)] = ap
            out["OBJECT_TYPE_TYPE_%s_LEVEL_%d/APH" % (KEY_TYPES[t], lv + 1)] = aph
    return out


def result_text(scores):
    text = "\n"
    for key in KEYS:
        text += "%s: %.4f \n" % (key, scores[key])
    return text


# ---- preparation -------------------------------------------------------------------------------------------------------------
def wrap(h):
    return h - math.floor(h / TWO_PI + 0.5) * TWO_PI


def fakelidar_to_lidar(box):
    x, y, z, w, l, h, r = [float(v) for v in box[:7]]
    return [x, y, z + h / 2, l, w, h, -(r + math.pi / 2)]


def to_fp32(v):
    return float(np.float32(v))


def prepare(det_annos, infos, class_names, fakelidar=False):
    """-> (pred rows, gt rows): lists of dicts {frame, type, box (7 fp32-rounded floats), score | level}, the boxes the estimator
    would be fed, in input order."""
    if len(det_annos) != len(infos):
        raise AssertionError("%d vs %d" % (len(det_annos), len(infos)))
    gts, preds = [], []
    for f, info in enumerate(infos):
        anno = info["annos"]
        if "num_points_in_gt" not in anno:
            raise NotImplementedError("num_points_in_gt")
        for name, diff, pts, box in zip(anno["name"], anno["difficulty"], anno["num_points_in_gt"], anno["gt_boxes_lidar"]):
            if name not in class_names or not pts > 0:
                continue
            level = int(diff) if int(diff) != 0 else (1 if pts > 5 else 2)
            box = [float(v) for v in box[:7]]
            if fakelidar:
                box = fakelidar_to_lidar(box)
            if str(name) not in WAYMO_CLASSES:
                raise ValueError(str(name))
            box[6] = wrap(box[6])
            if math.hypot(box[0], box[1]) < 1000.5:
                gts.append({"frame": f, "type": WAYMO_CLASSES.index(str(name)), "box": [to_fp32(v) for v in box], "level": level})
    for f, det in enumerate(det_annos):
        for name, score, box in zip(det["name"], det["score"], det["boxes_lidar"]):
            if str(name) not in WAYMO_CLASSES:
                raise ValueError(str(name))
            box = [float(v) for v in box[:7]]
            box[6] = wrap(box[6])
            if math.hypot(box[0], box[1]) < 1000.5:
                preds.append({"frame": f, "type": WAYMO_CLASSES.index(str(name)), "box": box, "score": float(score)})
    if preds and max(p["score"] for p in preds) > 1:
        for p in preds:
            p["score"] = 1 / (1 + math.exp(-p["score"]))
    for p in preds:
        p["box"] = [to_fp32(v) for v in p["box"]]
        p["score"] = to_fp32(p["score"])
    return preds, gts


def segments_of(preds, gts, n_frames):
    """One (type, iou, score, pred_heading, gt_heading, level) per (frame, type 1..4) that holds a box, frames then types ascending."""
    segs = []
    for f in range(n_frames):
        for t in range(1, 5):
            p = [r for r in preds if r["frame"] == f and r["type"] == t]
            g = [r for r in gts if r["frame"] == f and r["type"] == t]
            if not p and not g:
                continue
            segs.append((t, iou_block([r["box"] for r in p], [r["box"] for r in g]), [r["score"] for r in p], [r["box"][6] for r in p],
                         [r["box"][6] for r in g], [r["level"] for r in g]))
    return segs


def evaluate(det_annos, infos, class_names, fakelidar=False):
    """The whole definition -> (text, {key: value})."""
    preds, gts = prepare(det_annos, infos, class_names, fakelidar)
    tp, fn, fp, ha, _, _ = expect_counts(segments_of(preds, gts, len(infos)))
    scores = scores_of(tp, fn, fp, ha)
    return result_text(scores), scores


# ---- generators --------------------------------------------------------------------------------------------------------------
SCORE_VALUES = [float(np.float32(v)) for v in (1.0, 0.955, 0.9, 0.37, 0.365, 0.3, 0.123, 0.0)]   # 1, 0.9, 0.37, 0.3 and 0 are cutoffs


def draw_scores(rng, n):
    return np.array([SCORE_VALUES[i] for i in rng.integers(0, len(SCORE_VALUES), n)], np.float32)


def grid_iou(rng, shape, lo=0):
    """IoUs (k + 0.5) / 1000, k uniform in [lo, 1000): the quantisation never sits on a boundary."""
    return (rng.integers(lo, 1000, shape) + 0.5) / 1000


def sparse_segment(rng, n_pred, n_gt, seg_type):
    """Each prediction has 1-2 candidates with a uniform IoU (so some fall below the type's threshold); the IoUs of a segment are
    distinct while there are at most 1000 of them, which keeps two edges on one ground truth from tying."""
    iou = np.zeros((n_pred, n_gt), np.float64)
    if n_gt:
        pairs = [(i, int(j)) for i in range(n_pred) for j in rng.choice(n_gt, size=min(n_gt, int(rng.integers(1, 3))), replace=False)]
        ks = rng.permutation(1000)[:len(pairs)] if len(pairs) <= 1000 else rng.integers(0, 1000, len(pairs))
        for (i, j), k in zip(pairs, ks):
            iou[i, j] = (int(k) + 0.5) / 1000
    return _segment(rng, iou, seg_type)


def dense_segment(rng, n_pred, n_gt, seg_type):
    """Every pair carries weight."""
    return _segment(rng, grid_iou(rng, (n_pred, n_gt), int(type_threshold(seg_type) * 1000)).astype(np.float64), seg_type)


def _segment(rng, iou, seg_type):
    n_pred, n_gt = iou.shape
    return (seg_type, iou, draw_scores(rng, n_pred), rng.uniform(-math.pi, math.pi, n_pred), rng.uniform(-math.pi, math.pi, n_gt),
            rng.integers(1, 3, n_gt).astype(np.int32))


def pack_segments(segments):
    """-> the host arrays ops.waymo_eval_match takes: iou (flat), score fp32, pred_heading, gt_heading, level int32, pred_off, gt_off,
    seg_type."""
    cat = lambda parts, dtype: np.concatenate([np.asarray(p, dtype).reshape(-1) for p in parts] + [np.zeros(0, dtype)])    # noqa: E731
    p_off = np.concatenate([[0], np.cumsum([len(s[2]) for s in segments])]).astype(np.int32)
    g_off = np.concatenate([[0], np.cumsum([len(s[5]) for s in segments])]).astype(np.int32)
    return (cat([s[1] for s in segments], np.float64), cat([s[2] for s in segments], np.float32), cat([s[3] for s in segments], np.float64),
            cat([s[4] for s in segments], np.float64), cat([s[5] for s in segments], np.int32), p_off, g_off,
            np.array([s[0] for s in segments], np.int32))


def components(w):
    """Connected components of the bipartite graph of the positive entries of w -> [(rows, cols)]."""
    n, m = w.shape
    parent = list(range(n + m))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i, j in zip(*np.nonzero(w > 0)):
        parent[find(int(i))] = find(n + int(j))
    groups = {}
    for i, j in zip(*np.nonzero(w > 0)):
        rows, cols = groups.setdefault(find(int(i)), (set(), set()))
        rows.add(int(i))
        cols.add(int(j))
    return [(sorted(r), sorted(c)) for r, c in groups.values()]


def optimum_is_unique(w):
    """Whether the maximum-weight matching of w (ints, rows may stay free) is the only one: zero each chosen positive edge in turn
    and solve again; the total must drop.  An edge touches its connected component only, so each component is solved alone."""
    w = np.asarray(w, np.int64)
    for rows, cols in components(w):
        sub = w[np.ix_(rows, cols)]
        assign, total = solve(sub)
        for r, c in enumerate(assign):
            if c < 0:
                continue
            cut = sub.copy()
            cut[r, c] = 0
            if solve(cut)[1] >= total:
                return False
    return True


# ---- frames for the end-to-end tests -----------------------------------------------------------------------------------------
def box(x, y, z=0.0, dx=4.0, dy=2.0, dz=1.5, h=0.0):
    return [x, y, z, dx, dy, dz, h]


def frame_infos():
    """Three frames: Vehicle / Pedestrian / Cyclist with both levels; a frame whose ground truths are all level 2; an empty frame."""
    def annos(names, boxes, pts, diff=None):
        n = len(names)
        return {"annos": {"name": np.array(names, dtype="<U16"), "difficulty": np.array(diff if diff is not None else [0] * n, np.int64),
                          "num_points_in_gt": np.array(pts, np.int64), "gt_boxes_lidar": np.array(boxes, np.float32).reshape(n, 7)}}
    f0 = annos(["Vehicle", "Vehicle", "Pedestrian", "Cyclist", "Vehicle", "Sign"],
               [box(10.0, 0.0, h=0.25), box(20.0, 5.0, h=1.5), box(5.0, -5.0, dx=0.75, dy=0.75, dz=1.75, h=-2.0), box(-8.0, 3.0, dx=1.75, dy=0.75, h=3.0),
                box(30.0, -10.0, h=-0.5), box(0.0, 12.0, dx=0.5, dy=0.5)], [40, 3, 12, 6, 0, 9])
    f1 = annos(["Vehicle", "Pedestrian"], [box(-15.0, 2.0, h=0.75), box(3.0, 3.0, dx=0.75, dy=0.75, dz=1.75, h=1.0)], [4, 2], [0, 2])
    f2 = annos([], [], [])
    return [f0, f1, f2]


def perfect_dets(infos, class_names):
    """One prediction on every kept ground truth, score 0.9."""
    dets = []
    for info in infos:
        a = info["annos"]
        keep = np.array([n in class_names for n in a["name"]], bool) & (a["num_points_in_gt"] > 0)
        dets.append({"name": a["name"][keep], "score": np.full(int(keep.sum()), 0.9), "boxes_lidar": a["gt_boxes_lidar"][keep].astype(np.float64)})
    return dets


def perturbed_dets(infos, class_names, seed=3):
    """perfect_dets shifted, turned and rescored, plus false positives, among them a Cyclist in a frame without one and a Truck (the SIGN slot, no ground truth)."""
    rng = np.random.default_rng(seed)
    dets = perfect_dets(infos, class_names)
    for d in dets:
        n = len(d["name"])
        d["boxes_lidar"] = d["boxes_lidar"] + np.concatenate([rng.uniform(-0.25, 0.25, (n, 3)), rng.uniform(-0.1, 0.1, (n, 3)), rng.uniform(-0.6, 0.6, (n, 1))], 1)
        d["score"] = rng.uniform(0.05, 0.99, n)
    extra = [("Vehicle", box(10.5, 0.25, h=0.3), 0.41), ("Vehicle", box(50.0, 50.0), 0.97), ("Cyclist", box(-30.0, 0.0, dx=1.75, dy=0.75), 0.6),
             ("Truck", box(0.0, 12.0, dx=0.5, dy=0.5), 0.8)]
    for f in (0, 1, 2):
        d = dets[f]
        picks = extra if f != 2 else extra[2:3]
        d["name"] = np.concatenate([d["name"], np.array([e[0] for e in picks], dtype="<U16")])
        d["boxes_lidar"] = np.concatenate([d["boxes_lidar"].reshape(-1, 7), np.array([e[1] for e in picks], np.float64)])
        d["score"] = np.concatenate([d["score"], np.array([e[2] for e in picks])])
    return dets
