"""The Waymo detection metric (LEVEL_1 / LEVEL_2 AP and APH per object type) as the project's own code: `eval_metric: aph` of
WaymoDataset.  The reference hands this to TensorFlow and the waymo_open_dataset package (`eval_metric: waymo`, which keeps
raising ImportError here); its preparation of the two box lists (reference waymo_eval.py:26-84, 169-203) is restated below, the
metric itself is written from its definition in DESIGN.md 3.15.

    host    the preparation (class filter and difficulty of the ground truth, heading wrap, distance mask, logits, fp32 rounding),
            the CSR order by (frame, type), the 16 precision / recall curves (short fp64 vector passes) and the text
    device  ops.waymo_eval_iou      7-DOF IoU of every same-segment pair by exact clipping
            ops.waymo_eval_match    per segment one shortest-augmenting-path assignment that yields all 101 score cutoffs, counts
                                    folded per type in a fixed order (csrc/waymo_eval.hip)

route="host" runs the same definition in numpy with scipy.optimize.linear_sum_assignment solved at every cutoff: the library-free
route of the tests and the baseline of tools/bench_waymo_eval.py.

Agreement with the numbers of the official C++ metric is unmeasured: that tool is on no machine this project runs on.  Its
handling of recall gaps wider than 0.05 (`desired_recall_delta`) is not restated, and the no-label-zone flag is zero, as in the
reference."""
import functools
import warnings

import numpy as np

WAYMO_CLASSES = ["unknown", "Vehicle", "Pedestrian", "Truck", "Cyclist"]          # estimator type = index; 3 is its SIGN slot
KEY_TYPES = ("VEHICLE", "PEDESTRIAN", "SIGN", "CYCLIST")
KEYS = tuple("OBJECT_TYPE_TYPE_%s_LEVEL_%d/%s" % (t, lv, m) for t in KEY_TYPES for lv in (1, 2) for m in ("AP", "APH"))
IOU_THRESHOLDS = (0.0, 0.7, 0.5, 0.5, 0.5)
N_CUT = 101
DISTANCE_THRESH = 1000
MAX_SEGMENTS_PER_LAUNCH = 16384       # the match workspace holds 3.6 KB of snapshots per segment: 59 MB a launch
TWO_PI = 2 * np.pi


def score_cutoffs():
    """The 101 cutoffs as the estimator's fp32 config holds them (ops.waymo_score_cutoffs)."""
    from .... import ops
    return ops.waymo_score_cutoffs()


# ---- preparation
def _types_of(names):
    names = np.asarray(names)
    if names.size == 0:
        return np.zeros(0, np.int32)
    uniq, inverse = np.unique(names.astype(str), return_inverse=True)
    for name in uniq:
        if name not in WAYMO_CLASSES:
            raise ValueError(f"'{name}' is not in list: the Waymo metric knows {WAYMO_CLASSES}")
    return np.array([WAYMO_CLASSES.index(name) for name in uniq], np.int32)[inverse.reshape(-1)]


def _rows7(boxes, n):
    return np.asarray(boxes, np.float64).reshape(n, -1)[:, :7] if n else np.zeros((0, 7))


def _finish(boxes, frame, types, extra):
    """Heading wrap, distance mask, fp32 rounding of one side -> (boxes fp64 [n, 7] holding fp32 values, frame, type, extra)."""
    boxes = np.concatenate(boxes + [np.zeros((0, 7))]).astype(np.float64)
    frame, types, extra = np.concatenate(frame + [np.zeros(0, np.int64)]), np.concatenate(types + [np.zeros(0, np.int32)]), np.concatenate(extra + [np.zeros(0)])
    boxes[:, 6] = boxes[:, 6] - np.floor(boxes[:, 6] / TWO_PI + 0.5) * TWO_PI
    keep = np.hypot(boxes[:, 0], boxes[:, 1]) < DISTANCE_THRESH + 0.5
    return boxes[keep].astype(np.float32).astype(np.float64), frame[keep], types[keep], extra[keep]


def prepare(det_annos, gt_annos, class_names, info_with_fakelidar=False):
    """The two box lists the estimator would be fed.  Nothing passed in is changed.  -> dict of pred_boxes / gt_boxes fp64 [., 7]
    (fp32 values), pred_frame / gt_frame, pred_type / gt_type (index into WAYMO_CLASSES), pred_score fp32, gt_level int32."""
    from ...utils import box_utils
    if len(det_annos) != len(gt_annos):
        raise ValueError("%d frames of predictions vs %d of ground truth: they pair up by position" % (len(det_annos), len(gt_annos)))
    boxes, frame, types, level = [], [], [], []
    for f, anno in enumerate(gt_annos):
        if "num_points_in_gt" not in anno:
            raise NotImplementedError("the infos carry no num_points_in_gt (created before Waymo v1.2 / OpenPCDet 20201126): re-create "
                                      "the validation infos to score with the Waymo metric")
        names, pts = np.asarray(anno["name"]), np.asarray(anno["num_points_in_gt"])
        keep = np.isin(names.astype(str), list(class_names)).reshape(len(names)) & (pts > 0)
        diff = np.array(anno["difficulty"], copy=True).astype(np.int32)
        diff[(diff == 0) & (pts > 5)] = 1
        diff[(diff == 0) & (pts <= 5)] = 2
        b = _rows7(anno["gt_boxes_lidar"], len(names))
        if info_with_fakelidar:
            b = box_utils.boxes3d_kitti_fakelidar_to_lidar(b)
        boxes.append(b[keep])
        frame.append(np.full(int(keep.sum()), f, np.int64))
        types.append(_types_of(names[keep]))
        level.append(diff[keep].astype(np.float64))
    gt_boxes, gt_frame, gt_type, gt_level = _finish(boxes, frame, types, level)
    boxes, frame, types, score = [], [], [], []
    for f, anno in enumerate(det_annos):
        n = len(anno["name"])
        boxes.append(_rows7(anno["boxes_lidar"], n))
        frame.append(np.full(n, f, np.int64))
        types.append(_types_of(anno["name"]))
        score.append(np.asarray(anno["score"], np.float64).reshape(n))
    pred_boxes, pred_frame, pred_type, pred_score = _finish(boxes, frame, types, score)
    if pred_score.size and pred_score.max() > 1:
        warnings.warn("Waymo evaluation only supports normalized scores: the scores exceed 1 and go through the logistic function")
        pred_score = 1 / (1 + np.exp(-pred_score))
    return {"pred_boxes": pred_boxes, "pred_frame": pred_frame, "pred_type": pred_type, "pred_score": pred_score.astype(np.float32),
            "gt_boxes": gt_boxes, "gt_frame": gt_frame, "gt_type": gt_type, "gt_level": gt_level.astype(np.int32)}


def segment(data):
    """CSR order by (frame, type): one segment per (frame, type 1..4) that holds a prediction or a ground truth; boxes of type 0
    (`unknown`) belong to no reported breakdown and leave.  -> dict of the two sides in segment order, pred_off / gt_off int32
    [n_seg + 1] and seg_type int32 [n_seg]."""
    def keys(frame, types):
        return frame.astype(np.int64) * 5 + types
    pk, gk = keys(data["pred_frame"], data["pred_type"]), keys(data["gt_frame"], data["gt_type"])
    pm, gm = data["pred_type"] > 0, data["gt_type"] > 0
    p_order, g_order = np.flatnonzero(pm)[np.argsort(pk[pm], kind="stable")], np.flatnonzero(gm)[np.argsort(gk[gm], kind="stable")]
    seg_keys = np.union1d(pk[pm], gk[gm])
    p_off = np.searchsorted(pk[p_order], np.concatenate([seg_keys, [np.iinfo(np.int64).max]]), side="left").astype(np.int32)
    g_off = np.searchsorted(gk[g_order], np.concatenate([seg_keys, [np.iinfo(np.int64).max]]), side="left").astype(np.int32)
    return {"pred_boxes": data["pred_boxes"][p_order], "pred_score": data["pred_score"][p_order], "gt_boxes": data["gt_boxes"][g_order],
            "gt_level": data["gt_level"][g_order], "pred_off": p_off, "gt_off": g_off, "seg_type": (seg_keys % 5).astype(np.int32)}


def launch_slices(seg, step):
    n_seg = len(seg["seg_type"])
    for lo in range(0, n_seg, step):
        hi = min(lo + step, n_seg)
        p0, p1, g0, g1 = seg["pred_off"][lo], seg["pred_off"][hi], seg["gt_off"][lo], seg["gt_off"][hi]
        yield {"pred_boxes": seg["pred_boxes"][p0:p1], "pred_score": seg["pred_score"][p0:p1], "gt_boxes": seg["gt_boxes"][g0:g1],
               "gt_level": seg["gt_level"][g0:g1], "pred_off": seg["pred_off"][lo:hi + 1] - p0, "gt_off": seg["gt_off"][lo:hi + 1] - g0,
               "seg_type": seg["seg_type"][lo:hi]}


def empty_counts():
    return np.zeros((4, 2, N_CUT), np.int64), np.zeros((4, 2, N_CUT), np.int64), np.zeros((4, N_CUT), np.int64), np.zeros((4, 2, N_CUT), np.float64)


# ---- counts: device route
def counts_device(seg, max_segments=MAX_SEGMENTS_PER_LAUNCH):
    """tp, fn [4, 2, 101] int64, fp [4, 101] int64, sum_ha [4, 2, 101] fp64 through the two kernels; launches of at most
    max_segments segments, added in launch order."""
    import torch

    from .... import ops
    dev = torch.device("cuda")
    up = functools.partial(ops.eval_upload, dev=dev)
    tp, fn, fp, ha = empty_counts()
    for part in launch_slices(seg, max_segments):
        pred, gt = up(part["pred_boxes"], np.float64), up(part["gt_boxes"], np.float64)
        iou = ops.waymo_eval_iou(pred, gt, part["pred_off"], part["gt_off"])
        out = ops.waymo_eval_match(iou, up(part["pred_score"], np.float32), pred[:, 6].contiguous(), gt[:, 6].contiguous(),
                                   up(part["gt_level"], np.int32), part["pred_off"], part["gt_off"], part["seg_type"])
        tp, fn, fp, ha = tp + out[0].cpu().numpy(), fn + out[1].cpu().numpy(), fp + out[2].cpu().numpy(), ha + out[3].cpu().numpy()
    return tp, fn, fp, ha


# ---- counts: numpy / scipy route
def _clip_host(poly, n, axis, sign, lim):
    """One half-plane clip of P convex polygons at once: poly [P, 8, 2], n [P] corners -> (clipped, corners)."""
    count = len(poly)
    out, m, rows, o = np.zeros_like(poly), np.zeros(count, np.int64), np.arange(count), 1 - axis
    for i in range(8):
        valid = i < n
        k = np.where(i + 1 < n, i + 1, 0)
        p, q = poly[:, i], poly[rows, k]
        pc, qc = sign * p[:, axis], sign * q[:, axis]
        pin, qin = pc <= lim, qc <= lim
        put = valid & pin & (m < 8)
        out[rows[put], m[put]] = p[put]
        m = m + put
        cross = valid & (pin != qin) & (m < 8)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (lim - pc) / (qc - pc)
            v = np.empty_like(p)
            v[:, axis] = sign * lim
            v[:, o] = p[:, o] + t * (q[:, o] - p[:, o])
        out[rows[cross], m[cross]] = v[cross]
        m = m + cross
    return out, m


def iou_host(a, b):
    """7-DOF IoU of the row pairs of a and b [P, 7] in numpy: the kernel's arithmetic, statement for statement."""
    a, b = np.asarray(a, np.float64).reshape(-1, 7), np.asarray(b, np.float64).reshape(-1, 7)
    count = len(a)
    ca, sa, cb, sb = np.cos(a[:, 6]), np.sin(a[:, 6]), np.cos(b[:, 6]), np.sin(b[:, 6])
    hx, hy = a[:, 3] / 2, a[:, 4] / 2
    poly = np.zeros((count, 8, 2))
    for k, (sx, sy) in enumerate(((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))):
        lx, ly = sx * hx, sy * hy
        rx, ry = (a[:, 0] + (lx * ca - ly * sa)) - b[:, 0], (a[:, 1] + (lx * sa + ly * ca)) - b[:, 1]
        poly[:, k, 0], poly[:, k, 1] = rx * cb + ry * sb, ry * cb - rx * sb
    n = np.full(count, 4, np.int64)
    bx, by = b[:, 3] / 2, b[:, 4] / 2
    for axis, sign, lim in ((0, 1.0, bx), (0, -1.0, bx), (1, 1.0, by), (1, -1.0, by)):
        poly, n = _clip_host(poly, n, axis, sign, lim)
    acc, rows = np.zeros(count), np.arange(count)
    for i in range(8):
        k = np.where(i + 1 < n, i + 1, 0)
        term = poly[:, i, 0] * poly[rows, k, 1] - poly[rows, k, 0] * poly[:, i, 1]
        acc = np.where(i < n, acc + term, acc)
    area = np.where(n >= 3, np.abs(acc) / 2, 0.0)
    zlo, zhi = np.maximum(a[:, 2] - a[:, 5] / 2, b[:, 2] - b[:, 5] / 2), np.minimum(a[:, 2] + a[:, 5] / 2, b[:, 2] + b[:, 5] / 2)
    inter = area * np.maximum(zhi - zlo, 0.0)
    den = ((a[:, 3] * a[:, 4]) * a[:, 5] + (b[:, 3] * b[:, 4]) * b[:, 5]) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0.0, np.minimum(np.maximum(inter / den, 0.0), 1.0), 0.0)


def heading_accuracy(pred_heading, gt_heading):
    d = np.fmod(np.abs(pred_heading - gt_heading), TWO_PI)
    return 1.0 - np.minimum(d, TWO_PI - d) / np.pi


def match_counts_host(iou, score, pred_heading, gt_heading, gt_level, seg_type, cutoffs):
    """One segment on the host: scipy's assignment solved afresh at every cutoff -> tp [2, 101], fn [2, 101], fp [101], sum_ha [2, 101]."""
    from scipy.optimize import linear_sum_assignment
    n_pred, n_gt = len(score), len(gt_level)
    iou = np.asarray(iou, np.float64).reshape(n_pred, n_gt)
    w = np.where(iou >= IOU_THRESHOLDS[seg_type], (iou * 1000).astype(np.int64), 0)
    tp, fn, fp, ha = np.zeros((2, N_CUT), np.int64), np.zeros((2, N_CUT), np.int64), np.zeros(N_CUT, np.int64), np.zeros((2, N_CUT))
    for k, c in enumerate(cutoffs):
        act = np.flatnonzero(score >= c)
        sub = np.concatenate([w[act], np.zeros((len(act), len(act)), np.int64)], 1)
        rows, cols = linear_sum_assignment(sub, maximize=True) if len(act) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        hit = sub[rows, cols] > 0
        rows, cols = act[rows[hit]], cols[hit]
        fp[k] = len(act) - len(rows)
        acc = heading_accuracy(pred_heading[rows], gt_heading[cols])
        for lv in (1, 2):
            inl = gt_level[cols] <= lv
            tp[lv - 1, k] = inl.sum()
            fn[lv - 1, k] = (gt_level <= lv).sum() - inl.sum()
            ha[lv - 1, k] = acc[inl].sum()
    return tp, fn, fp, ha


def counts_host(seg, iou=None):
    """counts_device in numpy and scipy.  iou: the flat IoU blocks when they are already known."""
    tp, fn, fp, ha = empty_counts()
    cutoffs, at = score_cutoffs(), 0
    for s, t in enumerate(seg["seg_type"]):
        p0, p1, g0, g1 = seg["pred_off"][s], seg["pred_off"][s + 1], seg["gt_off"][s], seg["gt_off"][s + 1]
        pred, gt = seg["pred_boxes"][p0:p1], seg["gt_boxes"][g0:g1]
        n = len(pred) * len(gt)
        if iou is None:
            block = iou_host(np.repeat(pred, len(gt), 0), np.tile(gt, (len(pred), 1)))
        else:
            block = iou[at:at + n]
        at += n
        out = match_counts_host(block, seg["pred_score"][p0:p1], pred[:, 6], gt[:, 6], seg["gt_level"][g0:g1], int(t), cutoffs)
        tp[t - 1], fn[t - 1], fp[t - 1], ha[t - 1] = tp[t - 1] + out[0], fn[t - 1] + out[1], fp[t - 1] + out[2], ha[t - 1] + out[3]
    return tp, fn, fp, ha


# ---- curves
def _ratio(a, b):
    return np.divide(a, b, out=np.zeros_like(a, dtype=np.float64), where=b != 0)


def average_precision(precision, recall):
    """Area under the non-increasing precision envelope over the 101 points and recall 0."""
    order = np.argsort(-recall, kind="stable")
    r, best = np.concatenate([recall[order], [0.0]]), np.maximum.accumulate(precision[order])
    return float(((r[:-1] - r[1:]) * best).sum())


def curves(tp, fn, fp, sum_ha):
    """The 16 numbers in the order of KEYS."""
    out = {}
    for t, name in enumerate(KEY_TYPES):
        for lv in range(2):
            a, b, c, h = tp[t, lv].astype(np.float64), fn[t, lv].astype(np.float64), fp[t].astype(np.float64), sum_ha[t, lv]
            out["OBJECT_TYPE_TYPE_%s_LEVEL_%d/AP" % (name, lv + 1)] = average_precision(_ratio(a, a + c), _ratio(a, a + b))
            out["OBJECT_TYPE_TYPE_%s_LEVEL_%d/APH" % (name, lv + 1)] = average_precision(_ratio(h, a + c), _ratio(h, a + b))
    return out


def result_text(ap_dict):
    text = "\n"
    for key in KEYS:
        text += "%s: %.4f \n" % (key, ap_dict[key])
    return text


def evaluate(det_annos, gt_annos, class_names, info_with_fakelidar=False, route="device"):
    """-> (result text, {key: value}) of the 16 numbers.  gt_annos: the `annos` of the infos, position by position with det_annos."""
    if route not in ("device", "host"):
        raise ValueError(f"route '{route}': 'device' or 'host'")
    seg = segment(prepare(det_annos, gt_annos, class_names, info_with_fakelidar))
    ap_dict = curves(*(counts_device(seg) if route == "device" else counts_host(seg)))
    return result_text(ap_dict), ap_dict
