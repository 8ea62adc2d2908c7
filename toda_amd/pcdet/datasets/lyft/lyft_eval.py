"""The Lyft detection metric (mAP over the IoU cut-offs 0.5 .. 0.95) as the project's own code: `eval_metric: lyft` of
LyftDataset.  The reference (lyft_mAP_eval/lyft_eval.py get_average_precisions, lyft_utils.py) intersects one shapely polygon
pair per (prediction, ground truth) inside a Python loop over every prediction, and reads the boxes through lyft_dataset_sdk and
pyquaternion; none of the three is needed here.  The metric is written from its definition.

    host    the tables (<root>/data/{sample_annotation,instance,category}.json), the global-frame rows of both sides in fp64
            (O(n)), the CSR order by (sample, class), the text
    device  ops.lyft_eval_best     per prediction the largest IoU over its segment's ground truths and its first argmax
            ops.lyft_eval_flags    the true-positive flags at every cut-off (csrc/lyft_eval.hip)
            torch                  per class: stable sort by score, int64 cumsums, precision envelope, area under the curve

A row is centre x y z, c, s, width, length, height; (c, s) is the first column of the box's rotation and is not normalised: with
a tilted pose the ground rectangle shrinks by its norm while the volume stays w l h, as in the reference.

route="host" runs the same definition in numpy with the reference's sequential gt_checked walk: the library-free route and the
baseline of tools/bench_lyft_eval.py.

Deviations from the reference, all in how the boxes are read, none in the metric: the ground truths come from the tables in table
order (the SDK walks sample['anns']; the order matters only between ground truths of identical IoU); predictions are moved by
the infos' car_to_global . ref_to_car instead of the SDK's quaternions; a class with predictions but without ground truths
scores -1, and that -1 enters the mean, as it does in the reference."""
import json
from pathlib import Path

import numpy as np

TABLES = ("sample_annotation", "instance", "category")
ROW_COLS = 8
EPS64 = float(np.finfo(np.float64).eps)


# ---- the tables
def load_tables(root):
    """{name: list of records} of <root>/data/{sample_annotation,instance,category}.json."""
    tables = {}
    for name in TABLES:
        path = Path(root) / "data" / f"{name}.json"
        if not path.exists():
            raise FileNotFoundError(f"Lyft table {name}.json not found at {path}: eval_metric 'lyft' reads the ground truths from the tables "
                                    f"{', '.join(TABLES)}; without them score with eval_metric 'kitti'")
        with open(path) as f:
            tables[name] = json.load(f)
    return tables


def ground_truth_rows(tables, sample_tokens=None):
    """{sample token: (rows fp64 [n, 8], names [n])}: every annotation of the samples (all of them with sample_tokens None),
    grouped by sample_token in table order.  c and s come from the normalised quaternion; the name is the instance's category."""
    cat_name = {c["token"]: c["name"] for c in tables["category"]}
    inst_cat = {i["token"]: cat_name[i["category_token"]] for i in tables["instance"]}
    wanted = None if sample_tokens is None else set(sample_tokens)
    anns = [a for a in tables["sample_annotation"] if wanted is None or a["sample_token"] in wanted]
    if not anns:
        return {}
    for ann in anns:
        if len(ann["translation"]) != 3 or len(ann["size"]) != 3 or len(ann["rotation"]) != 4:
            raise ValueError(f"annotation {ann.get('token')}: translation, size and rotation must have 3, 3 and 4 elements")
    t, size, q = (np.array([a[key] for a in anns], np.float64) for key in ("translation", "size", "rotation"))
    norm = np.sqrt((q * q).sum(1))
    bad = ~(np.isfinite(t).all(1) & np.isfinite(size).all(1) & np.isfinite(q).all(1))
    if bad.any():
        raise ValueError(f"annotation {anns[int(np.flatnonzero(bad)[0])].get('token')}: translation, size or rotation is not finite")
    if not (size > 0).all():
        k = int(np.flatnonzero(~(size > 0).all(1))[0])
        raise ValueError(f"annotation {anns[k].get('token')}: size {size[k].tolist()} is not positive")
    if not (norm > 0).all():
        raise ValueError(f"annotation {anns[int(np.flatnonzero(~(norm > 0))[0])].get('token')}: zero rotation quaternion")
    w, x, y, z = (q / norm[:, None]).T
    rows = np.stack([t[:, 0], t[:, 1], t[:, 2], 1 - 2 * (y * y + z * z), 2 * (x * y + z * w), size[:, 0], size[:, 1], size[:, 2]], 1)
    names = np.array([inst_cat[a["instance_token"]] for a in anns], dtype=object)
    members = {}
    for k, ann in enumerate(anns):                     # table order within each sample
        members.setdefault(ann["sample_token"], []).append(k)
    return {tok: (rows[idx], names[idx]) for tok, idx in members.items()}


# ---- predictions
def prediction_rows(info, boxes):
    """LiDAR-frame boxes [n, >= 7] (x y z dx dy dz heading) of one sample -> global rows fp64 [n, 8] by G = car_to_global .
    ref_to_car of the sample's info: centre = G (x, y, z, 1), R = rot(G) Rz(heading), c = R[0, 0], s = R[1, 0], width dy,
    length dx, height dz."""
    boxes = np.asarray(boxes, np.float64)
    boxes = boxes.reshape(len(boxes), -1)[:, :7] if boxes.size else np.zeros((0, 7))
    G = np.asarray(info["car_to_global"], np.float64) @ np.asarray(info["ref_to_car"], np.float64)
    out = np.empty((len(boxes), ROW_COLS), np.float64)
    out[:, 0:3] = boxes[:, 0:3] @ G[:3, :3].T + G[:3, 3]
    ch, sh = np.cos(boxes[:, 6]), np.sin(boxes[:, 6])
    out[:, 3] = G[0, 0] * ch + G[0, 1] * sh
    out[:, 4] = G[1, 0] * ch + G[1, 1] * sh
    out[:, 5], out[:, 6], out[:, 7] = boxes[:, 4], boxes[:, 3], boxes[:, 5]
    return out


def segment(infos, det_annos, class_names, gt_by_token):
    """CSR order by (sample, class): one segment per (sample of det_annos, class of class_names) that holds a prediction.
    Predictions of other names belong to no class and leave; within a segment both sides keep their order.  -> dict of pred /
    gt rows, pred_score fp64, pred_cls (index into class_names) per prediction, pred_off / gt_off int32 [n_seg + 1] and n_gt
    int64 [n_classes], the ground truths of each class over the evaluated samples (in a segment or not)."""
    info_of = {info["token"]: info for info in infos}
    cls_of = {name: k for k, name in enumerate(class_names)}
    pred, score, pcls, gt, p_off, g_off = [], [], [], [], [0], [0]
    n_gt = np.zeros(len(class_names), np.int64)
    seen = set()
    for anno in det_annos:
        tok = anno["metadata"]["token"]
        if tok in seen:
            raise ValueError(f"sample {tok} appears twice among the detections")
        seen.add(tok)
        if tok not in info_of:
            raise KeyError(f"sample {tok} of the detections is not among the infos")
        g_rows, g_names = gt_by_token.get(tok, (np.zeros((0, ROW_COLS)), np.zeros(0, dtype=object)))
        g_cls = np.array([cls_of.get(n, -1) for n in g_names], np.int64)
        n_gt += np.bincount(g_cls[g_cls >= 0], minlength=len(class_names))
        n = len(anno["name"])
        if n == 0:
            continue
        rows = prediction_rows(info_of[tok], np.asarray(anno["boxes_lidar"], np.float64).reshape(n, -1))
        sc = np.asarray(anno["score"], np.float64).reshape(n)
        p_cls = np.array([cls_of.get(name, -1) for name in anno["name"]], np.int64)
        for c in np.unique(p_cls[p_cls >= 0]):
            sel = p_cls == c
            pred.append(rows[sel])
            score.append(sc[sel])
            pcls.append(np.full(int(sel.sum()), c, np.int64))
            gt.append(g_rows[g_cls == c])
            p_off.append(p_off[-1] + int(sel.sum()))
            g_off.append(g_off[-1] + int((g_cls == c).sum()))
    seg = {"pred": np.concatenate(pred + [np.zeros((0, ROW_COLS))]), "pred_score": np.concatenate(score + [np.zeros(0)]),
           "pred_cls": np.concatenate(pcls + [np.zeros(0, np.int64)]), "gt": np.concatenate(gt + [np.zeros((0, ROW_COLS))]),
           "pred_off": np.asarray(p_off, np.int32), "gt_off": np.asarray(g_off, np.int32), "n_gt": n_gt}
    if np.isnan(seg["pred_score"]).any():
        raise ValueError("a prediction's score is NaN: the metric orders the predictions by score")
    if not np.isfinite(seg["pred"]).all():
        raise ValueError("a prediction's box or its sample's pose is not finite")
    if not (seg["pred"][:, 5:8] > 0).all():
        raise ValueError("a prediction's size is not positive")
    return seg


# ---- flags: device route
def flags_device(seg, thresholds):
    """(tp uint8 [T, n_pred] on the device, best_iou, best_gt) through the two kernels."""
    import torch

    from .... import ops
    dev = torch.device("cuda")
    pred, gt = ops.eval_upload(seg["pred"], np.float64, dev), ops.eval_upload(seg["gt"], np.float64, dev)
    best_iou, best_gt = ops.lyft_eval_best(pred, gt, seg["pred_off"], seg["gt_off"])
    tp = ops.lyft_eval_flags(ops.eval_upload(seg["pred_score"], np.float64, dev), best_iou, best_gt, seg["pred_off"], thresholds)
    return tp, best_iou, best_gt


# ---- flags: numpy route
def corners_host(rows):
    """[n, 4, 2] ground corners in the reference's order: centre +- length / 2 (c, s) +- width / 2 (s, -c)."""
    x, y, c, s, hw, hl = rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4], rows[:, 5] / 2, rows[:, 6] / 2
    return np.stack([np.stack([(x + hl * c) + hw * s, (y + hl * s) - hw * c], 1), np.stack([(x + hl * c) - hw * s, (y + hl * s) + hw * c], 1),
                     np.stack([(x - hl * c) - hw * s, (y - hl * s) + hw * c], 1), np.stack([(x - hl * c) + hw * s, (y - hl * s) - hw * c], 1)], 1)


def _clip_host(poly, n, a, b):
    """One Sutherland-Hodgman step of P convex polygons at once: the part of poly [P, 8, 2] (n [P] corners) on or left of the
    lines a -> b [P, 2] -> (clipped, corners)."""
    count = len(poly)
    out, m, rows = np.zeros_like(poly), np.zeros(count, np.int64), np.arange(count)
    ex, ey = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    for i in range(8):
        valid = i < n
        k = np.where(i + 1 < n, i + 1, 0)
        p, q = poly[:, i], poly[rows, k]
        dp = ex * (p[:, 1] - a[:, 1]) - ey * (p[:, 0] - a[:, 0])
        dq = ex * (q[:, 1] - a[:, 1]) - ey * (q[:, 0] - a[:, 0])
        pin, qin = dp >= 0.0, dq >= 0.0
        put = valid & pin & (m < 8)
        out[rows[put], m[put]] = p[put]
        m = m + put
        cross = valid & (pin != qin) & (m < 8)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = dp / (dp - dq)
            v = p + t[:, None] * (q - p)
        out[rows[cross], m[cross]] = v[cross]
        m = m + cross
    return out, m


def iou_host(a, b):
    """IoU of the row pairs of a and b [P, 8] in numpy: the kernel's arithmetic, statement for statement."""
    a, b = np.asarray(a, np.float64).reshape(-1, ROW_COLS), np.asarray(b, np.float64).reshape(-1, ROW_COLS)
    count = len(a)
    poly = np.zeros((count, 8, 2))
    poly[:, :4] = corners_host(a)
    g = corners_host(b)
    n = np.full(count, 4, np.int64)
    for e in range(4):
        poly, n = _clip_host(poly, n, g[:, e], g[:, (e + 1) % 4])
    acc, rows = np.zeros(count), np.arange(count)
    for i in range(1, 7):
        term = ((poly[:, i, 0] - poly[:, 0, 0]) * (poly[:, i + 1, 1] - poly[:, 0, 1])
                - (poly[:, i + 1, 0] - poly[:, 0, 0]) * (poly[:, i, 1] - poly[:, 0, 1]))
        acc = np.where(i + 1 < n, acc + term, acc)
    area = np.where(n >= 3, np.abs(acc) / 2, 0.0)
    zlo, zhi = np.maximum(a[:, 2] - a[:, 7] / 2, b[:, 2] - b[:, 7] / 2), np.minimum(a[:, 2] + a[:, 7] / 2, b[:, 2] + b[:, 7] / 2)
    inter = np.maximum(zhi - zlo, 0.0) * area
    uni = ((a[:, 5] * a[:, 6]) * a[:, 7] + (b[:, 5] * b[:, 6]) * b[:, 7]) - inter
    ex, ey = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    ra = np.sqrt((a[:, 5] * a[:, 5] + a[:, 6] * a[:, 6]) * (a[:, 3] * a[:, 3] + a[:, 4] * a[:, 4])) / 2
    rb = np.sqrt((b[:, 5] * b[:, 5] + b[:, 6] * b[:, 6]) * (b[:, 3] * b[:, 3] + b[:, 4] * b[:, 4])) / 2
    apart = ex * ex + ey * ey > ((ra + rb) * (ra + rb)) * 1.002                      # circumcircles apart: nothing to clip
    return np.where(apart, 0.0, np.minimum(np.maximum(inter / uni, 0.0), 1.0))


def flags_host(seg, thresholds):
    """flags_device in numpy: per segment the IoU block, max / argmax, and the reference's walk down the predictions by score
    over a gt_checked table."""
    ths = np.asarray(thresholds, np.float64)
    n_pred = len(seg["pred"])
    tp, best_iou, best_gt = np.zeros((len(ths), n_pred), np.uint8), np.full(n_pred, -np.inf), np.full(n_pred, -1, np.int32)
    for s in range(len(seg["pred_off"]) - 1):
        p0, p1, g0, g1 = seg["pred_off"][s], seg["pred_off"][s + 1], seg["gt_off"][s], seg["gt_off"][s + 1]
        np_, ng = p1 - p0, g1 - g0
        if ng == 0 or np_ == 0:
            continue
        block = iou_host(np.repeat(seg["pred"][p0:p1], ng, 0), np.tile(seg["gt"][g0:g1], (np_, 1))).reshape(np_, ng)
        best_iou[p0:p1], best_gt[p0:p1] = block.max(1), block.argmax(1)
        checked = np.zeros((ng, len(ths)), bool)
        for p in np.argsort(-seg["pred_score"][p0:p1], kind="stable"):
            j, over = best_gt[p0 + p], best_iou[p0 + p] > ths
            tp[:, p0 + p] = over & ~checked[j]
            checked[j] |= over
    return tp, best_iou, best_gt


# ---- curves
def average_precisions(tp, pred_score, pred_cls, n_gt, n_classes):
    """[n_classes, T] AP per class and cut-off from the flags (a device or host array [T, n_pred]); a class with predictions but
    no ground truth holds -1 in every cut-off, a class without predictions 0.  Runs with torch on tp's device."""
    import torch
    tp = torch.as_tensor(tp)
    dev = tp.device
    score, cls = torch.as_tensor(pred_score, dtype=torch.float64).to(dev), torch.as_tensor(pred_cls, dtype=torch.int64).to(dev)
    n_cut = int(tp.shape[0])
    out = torch.zeros((n_classes, n_cut), dtype=torch.float64)
    for c in range(n_classes):
        sel = torch.nonzero(cls == c).reshape(-1)               # segment order = det_annos order within a class
        if sel.numel() == 0:
            continue
        if int(n_gt[c]) == 0:
            out[c] = -1.0
            continue
        order = sel[torch.sort(score[sel], descending=True, stable=True).indices]
        hit = tp[:, order].to(torch.int64)
        ctp, cfp = torch.cumsum(hit, 1), torch.cumsum(1 - hit, 1)
        recall = ctp.to(torch.float64) / float(n_gt[c])
        precision = ctp.to(torch.float64) / torch.clamp((ctp + cfp).to(torch.float64), min=EPS64)
        zero, one = torch.zeros((n_cut, 1), dtype=torch.float64, device=dev), torch.ones((n_cut, 1), dtype=torch.float64, device=dev)
        r = torch.cat([zero, recall, one], 1)
        p = torch.cat([zero, precision, zero], 1)
        p = torch.flip(torch.cummax(torch.flip(p, [1]), 1).values, [1])
        step = r[:, 1:] - r[:, :-1]
        out[c] = torch.where(step != 0, step * p[:, 1:], torch.zeros_like(step)).sum(1).cpu()
    return out.numpy()


def format_lyft_results(classwise_ap, class_names, iou_threshold_list, version="trainval"):
    """The reference's report text and {class: AP, 'mAP': mean} (lyft_utils.py format_lyft_results)."""
    mean = np.mean(classwise_ap)
    lines = ["----------------Lyft %s results-----------------" % version, "Average precision over IoUs: %s" % str(iou_threshold_list)]
    lines += ["{:<20}: \t {:.4f}".format(name, ap) for name, ap in zip(class_names, classwise_ap)]
    lines += ["--------------average performance-------------", "mAP:\t {:.4f}".format(mean)]
    ret = {name: ap for name, ap in zip(class_names, classwise_ap)}
    ret["mAP"] = mean
    return "\n".join(lines) + "\n", ret


def class_aps(seg, thresholds, n_classes, route="device"):
    """[n_classes, T] of one segmented workload through either route."""
    if route not in ("device", "host"):
        raise ValueError(f"route '{route}': 'device' or 'host'")
    ths = [float(t) for t in thresholds]
    if not ths or any(not (0 <= t <= 1) for t in ths) or any(b <= a for a, b in zip(ths, ths[1:])):
        raise ValueError(f"the IoU cut-offs {ths} must ascend within [0, 1]")
    tp = (flags_device if route == "device" else flags_host)(seg, ths)[0]
    return average_precisions(tp, seg["pred_score"], seg["pred_cls"], seg["n_gt"], n_classes)


def evaluate(infos, det_annos, class_names, root, iou_thresholds, version="trainval", route="device", tables=None):
    """-> (result text, {class: AP averaged over the cut-offs, 'mAP'}).  tables: the loaded tables when they are already known."""
    class_names, ths = list(class_names), [float(t) for t in iou_thresholds]
    tables = load_tables(root) if tables is None else tables
    tokens = [anno["metadata"]["token"] for anno in det_annos]
    seg = segment(infos, det_annos, class_names, ground_truth_rows(tables, tokens))
    aps = class_aps(seg, ths, len(class_names), route)
    return format_lyft_results(aps.mean(1), class_names, list(iou_thresholds), version=version)
