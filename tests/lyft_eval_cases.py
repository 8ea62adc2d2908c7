"""The Lyft mAP restated in numpy fp64 and plain Python, and the inputs of tests/test_lyft_eval_host.py and
tests/test_gpu_lyft_eval.py.

The restatement follows the reference's lyft_mAP_eval/lyft_eval.py function by function (Box3D, get_ious, recall_precision with
its sequential gt_checked walk, get_envelope, get_ap, get_average_precisions) on the reference's box dictionaries
{sample_token, translation, size, rotation, name, score}.  Two libraries are replaced: pyquaternion by quat_matrix, and shapely's
polygon intersection by Sutherland-Hodgman clipping of one convex quadrilateral by the other (exact for convex polygons) with the
shoelace area taken about the first corner.  recall_precision additionally returns what it saw per prediction (largest IoU, its
argmax, TP flags) so that the kernels can be checked before the curves.

The worlds: samples with a pose (ego pose and sensor calibration as translation + quaternion), ground truths and predictions in
the LiDAR frame.  build() turns a world into everything both sides read: the infos (4 x 4 matrices), det_annos, the three JSON
tables, and the reference's two dictionary lists, the predictions moved as lyft_utils.lidar_lyft_box_to_global moves them
(rotate, translate, rotate, translate on quaternions), not by the matrices."""
from collections import defaultdict

import numpy as np

THRESHOLDS = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]
CLASSES = ["car", "truck", "bus", "emergency_vehicle", "other_vehicle", "motorcycle", "bicycle", "pedestrian", "animal"]
EDGE = 1e-9                  # the exact-flag checks hold where no IoU lies this close to a cut-off or to the runner-up


# ---- quaternions (w, x, y, z), in place of pyquaternion
def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], np.float64)


def quat_matrix(q):
    """Rotation matrix of q after normalisation, as Quaternion(q).rotation_matrix."""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def quat_axis(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def quat_ypr(yaw, pitch, roll):
    return quat_mul(quat_axis([0, 0, 1], yaw), quat_mul(quat_axis([0, 1, 0], pitch), quat_axis([1, 0, 0], roll)))


def transform_matrix(translation, q):
    m = np.eye(4)
    m[:3, :3] = quat_matrix(q)
    m[:3, 3] = translation
    return m


# ---- the reference's Box3D
class Box3D:
    def __init__(self, sample_token, translation, size, rotation, name, score=-1):
        self.sample_token, self.name, self.score = sample_token, name, score
        self.translation, self.size, self.rotation = translation, size, rotation
        assert all(x > 0 for x in size)
        self.volume = np.prod(size)
        self.width, self.length, self.height = size
        self.center_x, self.center_y, self.center_z = translation
        self.min_z, self.max_z = self.center_z - self.height / 2, self.center_z + self.height / 2
        rot = quat_matrix(rotation)
        c, s = rot[0, 0], rot[1, 0]
        x, y, hl, hw = self.center_x, self.center_y, self.length / 2, self.width / 2
        self.ground = [(x + hl * c + hw * s, y + hl * s - hw * c), (x + hl * c - hw * s, y + hl * s + hw * c),
                       (x - hl * c - hw * s, y - hl * s + hw * c), (x - hl * c + hw * s, y - hl * s - hw * c)]

    def get_height_intersection(self, other):
        return max(0, min(other.max_z, self.max_z) - max(other.min_z, self.min_z))

    def get_intersection(self, other):
        return self.get_height_intersection(other) * polygon_area(convex_intersection(self.ground, other.ground))

    def get_iou(self, other):
        inter = self.get_intersection(other)
        return float(np.clip(inter / (self.volume + other.volume - inter), 0, 1))


def convex_intersection(subject, clip):
    """Sutherland-Hodgman: `subject` cut by every edge of the counter-clockwise convex polygon `clip`."""
    out = list(subject)
    for i in range(len(clip)):
        (ax, ay), (bx, by) = clip[i], clip[(i + 1) % len(clip)]
        ex, ey = bx - ax, by - ay
        src, out = out, []
        for k in range(len(src)):
            (px, py), (qx, qy) = src[k], src[(k + 1) % len(src)]
            dp, dq = ex * (py - ay) - ey * (px - ax), ex * (qy - ay) - ey * (qx - ax)
            if dp >= 0:
                out.append((px, py))
            if (dp >= 0) != (dq >= 0):
                t = dp / (dp - dq)
                out.append((px + t * (qx - px), py + t * (qy - py)))
        if not out:
            break
    return out


def polygon_area(poly):
    if len(poly) < 3:
        return 0.0
    x0, y0 = poly[0]
    acc = 0.0
    for i in range(1, len(poly) - 1):
        acc += (poly[i][0] - x0) * (poly[i + 1][1] - y0) - (poly[i + 1][0] - x0) * (poly[i][1] - y0)
    return abs(acc) / 2


# ---- the reference's curves
def group_by_key(items, key):
    groups = defaultdict(list)
    for item in items:
        groups[item[key]].append(item)
    return groups


def get_envelope(precisions):
    """Every precision raised to the largest one at or after it."""
    return np.maximum.accumulate(precisions[::-1])[::-1]


def get_ap(recalls, precisions):
    """Sentinels at both ends, the envelope, and (delta recall) x precision summed where recall moves."""
    r = np.concatenate(([0.0], recalls, [1.0]))
    p = get_envelope(np.concatenate(([0.0], precisions, [0.0])))
    moves = np.flatnonzero(r[1:] != r[:-1])
    return np.sum((r[moves + 1] - r[moves]) * p[moves + 1])


def recall_precision(gt, predictions, iou_threshold_list):
    """-> (recalls, precisions, ap_list, seen); seen[id(prediction dict)] = (all IoUs, max_overlap, jmax, tp flags [T])."""
    num_gts = len(gt)
    if num_gts == 0:
        return -1, -1, -1, {}
    image_gts = {tok: [Box3D(**x) for x in boxes] for tok, boxes in group_by_key(gt, "sample_token").items()}
    sample_gt_checked = {tok: np.zeros((len(boxes), len(iou_threshold_list))) for tok, boxes in image_gts.items()}
    predictions = sorted(predictions, key=lambda x: x["score"], reverse=True)
    tp, fp = np.zeros((len(predictions), len(iou_threshold_list))), np.zeros((len(predictions), len(iou_threshold_list)))
    seen = {}
    for k, prediction in enumerate(predictions):
        box = Box3D(**{key: prediction[key] for key in ("sample_token", "translation", "size", "rotation", "name", "score")})
        max_overlap, jmax, overlaps = -np.inf, -1, []
        gt_boxes = image_gts.get(prediction["sample_token"], [])
        gt_checked = sample_gt_checked.get(prediction["sample_token"], None)
        if len(gt_boxes) > 0:
            overlaps = [box.get_iou(x) for x in gt_boxes]
            max_overlap, jmax = np.max(overlaps), int(np.argmax(overlaps))
        for i, thr in enumerate(iou_threshold_list):
            if max_overlap > thr:
                if gt_checked[jmax, i] == 0:
                    tp[k, i] = 1.0
                    gt_checked[jmax, i] = 1
                else:
                    fp[k, i] = 1.0
            else:
                fp[k, i] = 1.0
        seen[prediction["uid"]] = (overlaps, max_overlap, jmax, tp[k].copy())
    fp, tp = np.cumsum(fp, axis=0), np.cumsum(tp, axis=0)
    recalls = tp / float(num_gts)
    assert np.all(0 <= recalls) & np.all(recalls <= 1)
    precisions = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    assert np.all(0 <= precisions) & np.all(precisions <= 1)
    return recalls, precisions, [get_ap(recalls[:, i], precisions[:, i]) for i in range(len(iou_threshold_list))], seen


def get_average_precisions(gt, predictions, class_names, iou_thresholds):
    """-> (average_precisions [n_classes], per-cut-off [n_classes, T], seen of every prediction of an evaluated class)."""
    assert all(0 <= t <= 1 for t in iou_thresholds)
    gt_by_class, pred_by_class = group_by_key(gt, "name"), group_by_key(predictions, "name")
    average, per_cut, seen = np.zeros(len(class_names)), np.zeros((len(class_names), len(iou_thresholds))), {}
    for class_id, name in enumerate(class_names):
        if name in pred_by_class:
            _, _, ap_list, s = recall_precision(gt_by_class[name], pred_by_class[name], iou_thresholds)
            seen.update(s)
            average[class_id] = np.mean(ap_list)
            per_cut[class_id] = ap_list
    return average, per_cut, seen


# ---- worlds
def pose(rng, tilt, reach=300.0):
    """{ego_t, ego_q, cs_t, cs_q}: an ego pose up to `reach` metres from the map origin with roll and pitch up to `tilt`, and a
    sensor a metre above the car with a slight mounting tilt."""
    return {"ego_t": np.concatenate([rng.uniform(-reach, reach, 2), rng.uniform(-20, 20, 1)]),
            "ego_q": quat_ypr(rng.uniform(-np.pi, np.pi), rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt)),
            "cs_t": np.array([1.2, 0.0, 1.8]) + rng.uniform(-0.1, 0.1, 3),
            "cs_q": quat_ypr(rng.uniform(-0.05, 0.05), rng.uniform(-tilt, tilt) / 4, rng.uniform(-tilt, tilt) / 4)}


SIZES = {"car": (4.6, 1.9, 1.7), "truck": (8.0, 2.6, 3.2), "bus": (11.0, 2.9, 3.4), "emergency_vehicle": (6.0, 2.3, 2.4), "other_vehicle": (7.5, 2.6, 3.0),
         "motorcycle": (2.2, 0.9, 1.5), "bicycle": (1.8, 0.6, 1.4), "pedestrian": (0.8, 0.7, 1.75), "animal": (0.9, 0.4, 0.6)}


def random_boxes(rng, name, n, spread=45.0):
    """[n, 7] LiDAR-frame boxes of a class, scattered so that most do not touch."""
    dx, dy, dz = SIZES[name]
    return np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), rng.uniform(-1.5, 0.5, n), dx * rng.uniform(0.8, 1.2, n),
                     dy * rng.uniform(0.8, 1.2, n), dz * rng.uniform(0.8, 1.2, n), rng.uniform(-np.pi, np.pi, n)], 1).reshape(n, 7)


def jittered(rng, box, k, strength):
    """k copies of a box moved, resized and turned by up to `strength` (a fraction of its size), so that their IoU with it spreads
    over the cut-offs."""
    out = np.tile(box, (k, 1))
    amount = rng.uniform(0, strength, (k, 1))
    out[:, 0:3] += amount * rng.uniform(-1, 1, (k, 3)) * box[3:6]
    out[:, 3:6] *= 1 + amount * rng.uniform(-0.5, 0.5, (k, 3))
    out[:, 6] += amount[:, 0] * rng.uniform(-0.6, 0.6, k)
    return out


def make_sample(rng, token, tilt, spec, tie_scores=False, twins=()):
    """spec: {class: (n_gt, n_pred)}.  Predictions are jittered copies of the class's ground truths (round robin, so several land on
    one ground truth) or, without ground truths, free boxes.  tie_scores: scores on a grid of 0.05, so many are equal.  twins:
    classes whose second ground truth repeats the first one's geometry."""
    gt_boxes, gt_names, pred_boxes, pred_names, scores = [], [], [], [], []
    for name, (n_gt, n_pred) in spec.items():
        g = random_boxes(rng, name, n_gt)
        if name in twins and n_gt >= 2:
            g[1] = g[0]
        p = np.concatenate([jittered(rng, g[k % n_gt], 1, 0.35) for k in range(n_pred)] + [np.zeros((0, 7))]) if n_gt else random_boxes(rng, name, n_pred)
        gt_boxes.append(g)
        gt_names += [name] * n_gt
        pred_boxes.append(p)
        pred_names += [name] * n_pred
        sc = rng.uniform(0.05, 1.0, n_pred)
        scores.append(np.round(sc * 20) / 20 if tie_scores else sc)
    order = rng.permutation(len(pred_names))                # the classes' predictions interleave, as a detector's do
    return {"token": token, "pose": pose(rng, tilt), "gt_boxes": np.concatenate(gt_boxes + [np.zeros((0, 7))]),
            "gt_names": gt_names, "pred_boxes": np.concatenate(pred_boxes + [np.zeros((0, 7))])[order], "pred_names": [pred_names[k] for k in order],
            "scores": np.concatenate(scores + [np.zeros(0)])[order].astype(np.float32)}


def build(samples):
    """-> dict: infos, det_annos, tables, and the reference's gt / prediction dictionary lists (each prediction carries `uid` =
    (sample index, position in det_annos) for the per-prediction checks)."""
    infos, det_annos, anns, instances, gts, preds = [], [], [], [], [], []
    categories = [{"token": f"cat_{name}", "name": name} for name in CLASSES + ["unlisted"]]
    for k, s in enumerate(samples):
        po = s["pose"]
        ref_to_car, car_to_global = transform_matrix(po["cs_t"], po["cs_q"]), transform_matrix(po["ego_t"], po["ego_q"])
        infos.append({"token": s["token"], "lidar_path": f"lidar/{s['token']}.bin", "ref_to_car": ref_to_car, "car_to_global": car_to_global,
                      "gt_boxes": s["gt_boxes"], "gt_names": np.array(s["gt_names"])})

        def to_global(box):
            centre = quat_matrix(po["cs_q"]) @ box[:3] + po["cs_t"]
            centre = quat_matrix(po["ego_q"]) @ centre + po["ego_t"]
            q = quat_mul(po["ego_q"], quat_mul(po["cs_q"], quat_axis([0, 0, 1], box[6])))
            return centre.tolist(), [float(box[4]), float(box[3]), float(box[5])], q.tolist()

        for i, (box, name) in enumerate(zip(s["gt_boxes"], s["gt_names"])):
            t, size, q = to_global(box)
            instances.append({"token": f"inst_{k}_{i}", "category_token": f"cat_{name}"})
            anns.append({"token": f"ann_{k}_{i}", "sample_token": s["token"], "instance_token": f"inst_{k}_{i}", "translation": t, "size": size, "rotation": q})
            gts.append({"sample_token": s["token"], "translation": t, "size": size, "rotation": q, "name": name})
        for i, (box, name, score) in enumerate(zip(s["pred_boxes"], s["pred_names"], s["scores"])):
            t, size, q = to_global(box.astype(np.float64))
            preds.append({"sample_token": s["token"], "translation": t, "size": size, "rotation": q, "name": name, "score": float(score), "uid": (k, i)})
        n = len(s["pred_names"])
        det_annos.append({"name": np.array(s["pred_names"]) if n else np.zeros(0), "score": s["scores"] if n else np.zeros(0),
                          "boxes_lidar": s["pred_boxes"] if n else np.zeros((0, 7)),
                          "pred_labels": np.array([CLASSES.index(c) + 1 for c in s["pred_names"]], np.int64) if n else np.zeros(0),
                          "frame_id": s["token"], "metadata": {"token": s["token"]}})
    return {"infos": infos, "det_annos": det_annos, "gt": gts, "pred": preds,
            "tables": {"sample_annotation": anns, "instance": instances, "category": categories}}


def segment_uids(det_annos, class_names):
    """The uid of every prediction in the evaluator's segment order: sample by sample, class by class in class_names order, then
    the position in det_annos."""
    uids = []
    for k, anno in enumerate(det_annos):
        for name in class_names:
            uids += [(k, i) for i, n in enumerate(anno["name"]) if n == name]
    return uids


def interleaved_tables(tables, rng):
    """The same records with the annotations of different samples interleaved: grouping by sample_token must keep each sample's order."""
    anns = tables["sample_annotation"]
    keys = rng.uniform(0, 1, len(anns))
    by_sample = defaultdict(list)
    for a in anns:
        by_sample[a["sample_token"]].append(a)
    # a random merge of the per-sample queues
    queues, merged = {tok: list(v) for tok, v in by_sample.items()}, []
    for key in keys:
        live = sorted(tok for tok, v in queues.items() if v)
        merged.append(queues[live[int(key * len(live))]].pop(0))
    return {**tables, "sample_annotation": merged}


def edge_world():
    """The segment shapes of the GPU test: 0 / 1 / 63 / 64 / 65 ground truths, 0 / 1 / 65 / 257 predictions (one more than the flags
    kernel's LDS chunk of 256), a sample with predictions of a class it has no ground truth of (truck in s0), a class with no
    ground truth at all (animal), a class without predictions (bicycle), twin ground truths, equal scores within and across
    samples, level and tilted poses."""
    rng = np.random.default_rng(20240521)
    return [make_sample(rng, "s0", 0.0, {"car": (64, 65), "pedestrian": (1, 1), "truck": (0, 3), "bus": (5, 0), "bicycle": (3, 0)}, tie_scores=True),
            make_sample(rng, "s1", 0.06, {"car": (10, 257), "pedestrian": (65, 66), "truck": (2, 2), "animal": (0, 4)}, tie_scores=True, twins=("car", "truck")),
            make_sample(rng, "s2", 0.35, {"pedestrian": (63, 5), "car": (1, 9), "motorcycle": (4, 12), "truck": (3, 1), "other_vehicle": (0, 1)}, twins=("motorcycle",)),
            make_sample(rng, "s3", 0.1, {"bus": (2, 0)}),
            make_sample(rng, "s4", 0.1, {})]


def small_world(seed=7):
    """Three samples, a few dozen boxes: the host tests' world."""
    rng = np.random.default_rng(seed)
    return [make_sample(rng, "a", 0.05, {"car": (6, 14), "pedestrian": (3, 5), "truck": (0, 2)}, tie_scores=True, twins=("car",)),
            make_sample(rng, "b", 0.3, {"car": (4, 7), "bus": (2, 3), "animal": (0, 2), "bicycle": (2, 0)}),
            make_sample(rng, "c", 0.0, {"pedestrian": (5, 9)}, tie_scores=True)]


def away_from_edges(seen, gt_twin_free=None):
    """The condition of the exact-flag checks, on the restatement's own numbers: every |largest IoU - cut-off| and every gap between
    the largest and the next smaller DIFFERENT IoU exceeds EDGE (an exactly equal runner-up is a constructed tie: twin ground
    truths, or several ground truths the prediction does not touch)."""
    for overlaps, best, _, _ in seen.values():
        if not overlaps:
            continue
        if min(abs(best - t) for t in THRESHOLDS) <= EDGE:
            return False
        lower = [v for v in overlaps if v != best]
        if lower and best - max(lower) <= EDGE:
            return False
    return True
