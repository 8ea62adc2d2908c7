"""Shared by tests/test_nusc_eval_host.py and tests/test_gpu_nusc_eval.py:
  * a loop-for-loop fp64 restatement of the nuScenes detection metric (`detection_cvpr_2019`) in plain Python floats: frame,
    filter, matching, the five errors, the curves and the scores.  It shares no code with toda_amd's evaluator;
  * segments for the match kernel on a 1/8 grid of the global frame (a subset of the 1/64 grid): every squared distance is exact,
    every distance is exact or a correctly rounded square root, so ties and threshold-equal cases are decided alike everywhere;
  * a mini nuScenes tree: three samples with non-trivial ref_from_car / car_from_global (sample 1 pitched by 4 degrees), the four
    devkit tables, a bike rack that holds the only bicycle, a car without an attribute, a pedestrian with NaN velocity."""
import json
import math
import pickle

import numpy as np

CLASSES = ["car", "truck", "bus", "trailer", "construction_vehicle", "pedestrian", "motorcycle", "bicycle", "traffic_cone", "barrier"]
RANGE = {"car": 50.0, "truck": 50.0, "bus": 50.0, "trailer": 50.0, "construction_vehicle": 50.0, "pedestrian": 40.0, "motorcycle": 40.0,
         "bicycle": 40.0, "traffic_cone": 30.0, "barrier": 30.0}
THS = [0.5, 1.0, 2.0, 4.0]
TP_TH = 2.0
METRICS = ["trans_err", "scale_err", "orient_err", "vel_err", "attr_err"]
ERR_ROWS = ["trans_err", "vel_err", "scale_err", "orient_err", "attr_err"]            # row order of the kernel's err output
NAN = float("nan")
VERSION = "v1.0-mini"


# ---- the restatement
def to_global(row, G, ego):
    """row = x y z dx dy dz h vx vy vz in the LiDAR frame -> {c, yaw, v, size, dist}."""
    x, y, z, h = row[0], row[1], row[2], row[6]
    c = [((G[r][0] * x + G[r][1] * y) + G[r][2] * z) + G[r][3] for r in range(3)]
    ch, sh = math.cos(h), math.sin(h)
    yaw = math.atan2(G[1][0] * ch + G[1][1] * sh, G[0][0] * ch + G[0][1] * sh)
    v = [(G[r][0] * row[7] + G[r][1] * row[8]) + G[r][2] * row[9] for r in range(2)]
    dist = math.sqrt((c[0] - ego[0]) ** 2 + (c[1] - ego[1]) ** 2)
    return {"c": c, "yaw": yaw, "v": v, "size": [row[3], row[4], row[5]], "dist": dist}


def quat_matrix(q):
    w, x, y, z = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def in_rack(c, rack):
    """Closed test of the point c in the rack's own axes; rack = (translation, size wlh, quaternion wxyz)."""
    t, wlh, q = rack
    R = quat_matrix(q)
    d = [c[k] - t[k] for k in range(3)]
    local = [sum(R[r][k] * d[r] for r in range(3)) for k in range(3)]              # R^T d
    half = [wlh[1] / 2, wlh[0] / 2, wlh[2] / 2]
    return all(abs(local[k]) <= half[k] for k in range(3))


def keeps(box, name, racks):
    if name not in RANGE or not box["dist"] < RANGE[name]:
        return False
    if name in ("bicycle", "motorcycle") and any(in_rack(box["c"], r) for r in racks):
        return False
    return True


def orient_err(gt_yaw, pred_yaw, name):
    p = math.pi if name == "barrier" else 2 * math.pi
    d = (gt_yaw - pred_yaw + p / 2) % p - p / 2              # Python's % on floats is the floored remainder
    if d > math.pi:
        d -= 2 * math.pi
    return abs(d)


def errors(g, p, dist, name):
    """[trans, vel, scale, orient, attr] of a matched pair (the kernel's row order)."""
    inter = min(g["size"][0], p["size"][0]) * min(g["size"][1], p["size"][1]) * min(g["size"][2], p["size"][2])
    vg, vp = g["size"][0] * g["size"][1] * g["size"][2], p["size"][0] * p["size"][1] * p["size"][2]
    vel = math.sqrt((g["v"][0] - p["v"][0]) ** 2 + (g["v"][1] - p["v"][1]) ** 2)         # NaN when the ground truth's is
    attr = NAN if g["attr"] == "" else (0.0 if g["attr"] == p["attr"] else 1.0)
    return [dist, vel, 1.0 - inter / (vg + vp - inter), orient_err(g["yaw"], p["yaw"], name), attr]


def match_segment(preds, gts, thr, name):
    """One (sample, class): preds / gts are lists of boxes ({c, yaw, v, size, attr}, preds with score) in index order ->
    ([gt index or -1 per prediction], [errors or None per prediction])."""
    order = sorted(range(len(preds)), key=lambda i: (-preds[i]["score"], -i))
    taken = [False] * len(gts)
    match, errs = [-1] * len(preds), [None] * len(preds)
    for i in order:
        best, best_d = -1, math.inf
        for j, g in enumerate(gts):
            if taken[j]:
                continue
            d = math.sqrt((g["c"][0] - preds[i]["c"][0]) ** 2 + (g["c"][1] - preds[i]["c"][1]) ** 2)
            if d < best_d:
                best, best_d = j, d
        if best_d < thr:
            taken[best] = True
            match[i] = best
            errs[i] = errors(gts[best], preds[i], best_d, name)
    return match, errs


def cummean(vals):
    if all(math.isnan(v) for v in vals):
        return [1.0] * len(vals)
    out, total, count = [], 0.0, 0
    for v in vals:
        if not math.isnan(v):
            total += v
            count += 1
        out.append(total / count if count else 0.0)
    return out


def curve(tp, conf, errs, npos):
    """tp [n] bool, conf [n], errs [n] (list of five, kernel row order, or None) in the global order ->
    (precision [101], confidence [101], {metric: [101]})."""
    ones = {m: np.ones(101) for m in METRICS}
    if npos == 0 or not any(tp):
        return np.zeros(101), np.zeros(101), ones
    prec, rec, ntp, nfp = [], [], 0, 0
    for hit in tp:
        ntp += 1 if hit else 0
        nfp += 0 if hit else 1
        prec.append(ntp / (ntp + nfp))
        rec.append(ntp / npos)
    grid = np.linspace(0, 1, 101)
    precision = np.interp(grid, rec, prec, right=0)
    confidence = np.interp(grid, rec, conf, right=0)
    tp_conf = [c for c, hit in zip(conf, tp) if hit]
    out = {}
    for m in METRICS:
        mean = cummean([e[ERR_ROWS.index(m)] for e, hit in zip(errs, tp) if hit])
        out[m] = np.interp(confidence[::-1], tp_conf[::-1], mean[::-1])[::-1]
    return precision, confidence, out


def ap_of(precision):
    return sum(max(float(v) - 0.1, 0.0) for v in precision[11:]) / 90 / 0.9


def tp_of(confidence, err_curve):
    last = max([k for k in range(101) if confidence[k] != 0], default=0)
    if last < 11:
        return 1.0
    return sum(float(v) for v in err_curve[11:last + 1]) / (last + 1 - 11)


def metric(samples):
    """samples: list of {"preds": [(name, box + score + attr)], "gts": [(name, box + attr)], "racks": [...]}, predictions in
    det_annos order -> the metrics_summary dict (without eval_time)."""
    kept = []
    index = 0
    for s in samples:
        preds = []
        for name, box in s["preds"]:
            if keeps(box, name, s["racks"]):
                preds.append((name, dict(box, index=index)))
            index += 1
        kept.append((preds, [(name, box) for name, box in s["gts"] if keeps(box, name, s["racks"])]))
    label_aps, label_tp = {}, {}
    for name in CLASSES:
        npos = sum(1 for _, gts in kept for n, _ in gts if n == name)
        label_aps[name] = {}
        for thr in THS:
            rows = []                                            # (score, index, tp, errs)
            for preds, gts in kept:
                mine, theirs = [b for n, b in preds if n == name], [b for n, b in gts if n == name]
                match, errs = match_segment(mine, theirs, thr, name)
                rows += [(b["score"], b["index"], match[k] >= 0, errs[k]) for k, b in enumerate(mine)]
            rows.sort(key=lambda r: (-r[0], -r[1]))
            precision, confidence, err_curves = curve([r[2] for r in rows], [r[0] for r in rows], [r[3] for r in rows], npos)
            label_aps[name][str(thr)] = ap_of(precision)
            if thr == TP_TH:
                label_tp[name] = {m: tp_of(confidence, err_curves[m]) for m in METRICS}
        for m in ("attr_err", "vel_err", "orient_err"):
            if name == "traffic_cone" or (name == "barrier" and m != "orient_err"):
                label_tp[name][m] = NAN
    mean_dist_aps = {n: sum(label_aps[n].values()) / len(THS) for n in CLASSES}
    mean_ap = sum(mean_dist_aps.values()) / len(CLASSES)
    tp_errors = {}
    for m in METRICS:
        vals = [label_tp[n][m] for n in CLASSES if not math.isnan(label_tp[n][m])]
        tp_errors[m] = sum(vals) / len(vals)
    tp_scores = {m: max(1.0 - tp_errors[m], 0.0) for m in METRICS}
    return {"label_aps": label_aps, "label_tp_errors": label_tp, "mean_dist_aps": mean_dist_aps, "mean_ap": mean_ap, "tp_errors": tp_errors,
            "tp_scores": tp_scores, "nd_score": (5 * mean_ap + sum(tp_scores.values())) / 10}


# ---- segments for the match kernel
def grid_boxes(rng, n, span, with_score, attrs=4):
    """n boxes with centres on the 1/8 grid in [0, span]^2; scores are sixteenths, so equal scores are common."""
    boxes = []
    for _ in range(n):
        b = {"c": [int(rng.integers(0, 8 * span + 1)) / 8.0, int(rng.integers(0, 8 * span + 1)) / 8.0, 0.0], "yaw": float(rng.uniform(-3.5, 3.5)),
             "v": [float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3))], "size": [float(v) for v in rng.uniform(0.5, 5.0, 3)]}
        if with_score:
            b["score"] = int(rng.integers(1, 16)) / 16.0
            b["attr"] = int(rng.integers(0, attrs))
        else:
            b["attr"] = "" if rng.random() < 0.2 else int(rng.integers(0, attrs))
            if rng.random() < 0.15:
                b["v"] = [NAN, NAN]
        boxes.append(b)
    return boxes


def hand_box(x, y, score=None, yaw=0.0, attr=0):
    b = {"c": [x, y, 0.0], "yaw": yaw, "v": [0.0, 0.0], "size": [2.0, 1.0, 1.5], "attr": attr}
    if score is not None:
        b["score"] = score
    return b


def pack_segments(segments):
    """[(class name, preds, gts)] -> the arrays ops.nusc_eval_match takes (numpy): pred [N, 8], score, pred_attr, gt [M, 8], gt_attr,
    pred_off, gt_off, seg_cls."""
    rows = lambda b: [b["c"][0], b["c"][1], b["yaw"], b["v"][0], b["v"][1]] + list(b["size"])      # noqa: E731
    preds = [b for _, ps, _ in segments for b in ps]
    gts = [b for _, _, gs in segments for b in gs]
    return (np.array([rows(b) for b in preds], np.float64).reshape(-1, 8), np.array([b["score"] for b in preds], np.float64),
            np.array([b["attr"] for b in preds], np.int32), np.array([rows(b) for b in gts], np.float64).reshape(-1, 8),
            np.array([-1 if b["attr"] == "" else b["attr"] for b in gts], np.int32),
            np.concatenate([[0], np.cumsum([len(ps) for _, ps, _ in segments])]).astype(np.int32),
            np.concatenate([[0], np.cumsum([len(gs) for _, _, gs in segments])]).astype(np.int32),
            np.array([CLASSES.index(n) for n, _, _ in segments], np.int32))


def expect_segments(segments):
    """The restatement on the segments -> (match [4, N] with rows of the packed gt array, err [5, N] at 2 m, NaN where unmatched)."""
    n = sum(len(ps) for _, ps, _ in segments)
    match, err = np.full((4, n), -1, np.int32), np.full((5, n), NAN)
    p0 = g0 = 0
    for name, preds, gts in segments:
        for t, thr in enumerate(THS):
            m, e = match_segment(preds, gts, thr, name)
            for k in range(len(preds)):
                if m[k] >= 0:
                    match[t, p0 + k] = g0 + m[k]
                    if thr == TP_TH:
                        err[:, p0 + k] = e[k]
        p0 += len(preds)
        g0 += len(gts)
    return match, err


# ---- the mini tree
def _rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    m = np.eye(4)
    i, j = {"z": (0, 1), "y": (2, 0), "x": (1, 2)}[axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def _shift(x, y, z):
    m = np.eye(4)
    m[:3, 3] = [x, y, z]
    return m


def sample_poses():
    """(ref_from_car, car_from_global) of the three samples.  Sample 1 drives up a 4-degree slope."""
    out = []
    for k, (yaw, pitch, pos) in enumerate([(30.0, 0.0, (410.0, 1180.0, 0.5)), (-75.0, 4.0, (655.5, 1604.25, 2.0)), (160.0, 0.0, (300.0, 900.0, 0.0))]):
        car_to_global = _shift(*pos) @ _rot("z", yaw) @ _rot("y", pitch)
        lidar_to_car = _shift(0.94, 0.0, 1.84) @ _rot("z", -89.5 + k) @ _rot("x", 0.3)
        out.append((np.linalg.inv(lidar_to_car), np.linalg.inv(car_to_global)))
    return out


# name, x, y, z, dx, dy, dz, heading, vx, vy, attribute ('' none), note
_GT = {
    0: [("car", 10.0, 3.0, -1.0, 4.2, 1.9, 1.6, 0.3, 3.0, 0.5, "vehicle.moving"),
        ("car", -20.0, 8.0, -1.0, 4.5, 2.0, 1.7, -1.2, 0.0, 0.0, "vehicle.parked"),
        ("car", 30.0, -12.0, -0.8, 4.0, 1.8, 1.5, 2.9, 0.0, 0.0, ""),                       # a ground truth without an attribute
        ("car", 54.0, 8.0, -0.5, 4.4, 1.9, 1.6, 0.1, 0.0, 0.0, "vehicle.parked"),            # beyond 50 m
        ("pedestrian", 5.0, -6.0, -0.9, 0.7, 0.6, 1.8, 0.5, NAN, NAN, "pedestrian.standing"),  # NaN velocity
        ("pedestrian", -8.0, -15.0, -0.9, 0.8, 0.7, 1.7, 1.5, 1.0, 0.4, "pedestrian.moving"),
        ("bicycle", 12.0, 14.0, -1.2, 1.8, 0.6, 1.2, 0.8, 0.0, 0.0, "cycle.without_rider"),   # stands in the rack
        ("ignore", 3.0, 3.0, -1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, "")],
    1: [("car", -15.0, -22.0, -1.1, 4.6, 1.9, 1.5, 1.9, -2.0, 1.0, "vehicle.moving"),
        ("truck", 18.0, 20.0, -0.3, 8.0, 2.6, 3.2, -0.4, 0.0, 0.0, "vehicle.stopped"),      # a prediction at rest is stated as parked
        ("motorcycle", -6.0, 9.0, -1.0, 2.1, 0.8, 1.4, 2.2, 0.0, 0.0, "cycle.without_rider"),
        ("barrier", 25.0, 24.0, -1.0, 0.5, 2.5, 1.0, 0.2, 0.0, 0.0, "")],                    # 34.7 m away: beyond 30 m
    2: [("car", 7.0, -30.0, -1.0, 4.3, 1.9, 1.6, -2.6, 0.0, 0.0, "vehicle.parked"),
        ("traffic_cone", 4.0, 11.0, -1.3, 0.4, 0.4, 0.7, 0.0, 0.0, 0.0, "")],
}
RACK_OF_SAMPLE_0 = (11.5, 14.0, -1.0, 2.0, 6.0, 1.5, 0.8)       # LiDAR frame x y z, size w l h, heading: holds the bicycle


def sample_gt(k):
    """(boxes [n, 9] fp32, velocity [n, 3] fp32 with vz 0, names, attributes) of sample k."""
    rows = _GT[k]
    boxes = np.array([r[1:10] for r in rows], np.float32)
    vel = np.concatenate([boxes[:, 7:9], np.zeros((len(rows), 1), np.float32)], 1)
    return boxes, vel, np.array([r[0] for r in rows]), [r[10] for r in rows]


def _quat_of(R):
    """(w, x, y, z) of a rotation matrix with a positive trace-or-pivot: Shepperd's method, independent of toda_amd's helper."""
    w = math.sqrt(max(0.0, 1 + R[0][0] + R[1][1] + R[2][2])) / 2
    x = math.copysign(math.sqrt(max(0.0, 1 + R[0][0] - R[1][1] - R[2][2])) / 2, R[2][1] - R[1][2])
    y = math.copysign(math.sqrt(max(0.0, 1 - R[0][0] + R[1][1] - R[2][2])) / 2, R[0][2] - R[2][0])
    z = math.copysign(math.sqrt(max(0.0, 1 - R[0][0] - R[1][1] + R[2][2])) / 2, R[1][0] - R[0][1])
    return [w, x, y, z]


def write_tree(data_path, with_gt=True, with_poses=True):
    """The mini tree under data_path / VERSION (infos of the `val` split and the four tables in VERSION / VERSION); returns
    (root, infos)."""
    root = data_path / VERSION
    (root / VERSION).mkdir(parents=True)
    poses = sample_poses()
    attributes = ["vehicle.moving", "vehicle.parked", "vehicle.stopped", "pedestrian.standing", "pedestrian.moving", "cycle.without_rider", "cycle.with_rider"]
    categories = {"car": "vehicle.car", "truck": "vehicle.truck", "pedestrian": "human.pedestrian.adult", "bicycle": "vehicle.bicycle",
                  "motorcycle": "vehicle.motorcycle", "barrier": "movable_object.barrier", "traffic_cone": "movable_object.trafficcone",
                  "ignore": "animal", "rack": "static_object.bicycle_rack"}
    tables = {"attribute": [{"token": f"attr_{a}", "name": a, "description": ""} for a in attributes],
              "category": [{"token": f"cat_{c}", "name": c, "description": ""} for c in sorted(set(categories.values()))],
              "instance": [], "sample_annotation": []}
    infos = []
    for k in range(3):
        boxes, vel, names, attrs = sample_gt(k)
        G = np.linalg.inv(poses[k][1]) @ np.linalg.inv(poses[k][0])
        info = {"lidar_path": f"samples/LIDAR_TOP/s{k}.pcd.bin", "token": f"sample{k}", "sweeps": []}
        if with_poses:
            info["ref_from_car"], info["car_from_global"] = poses[k]
        if with_gt:
            info.update(gt_boxes=boxes, gt_boxes_velocity=vel, gt_names=names, gt_boxes_token=np.array([f"ann{k}_{i}" for i in range(len(boxes))]),
                        num_lidar_pts=np.full(len(boxes), 9, np.int64), num_radar_pts=np.zeros(len(boxes), np.int64))
        infos.append(info)
        entries = [(f"ann{k}_{i}", names[i], boxes[i], attrs[i]) for i in range(len(boxes))]
        if k == 0:
            r = RACK_OF_SAMPLE_0
            entries.append(("rack0", "rack", np.array([r[0], r[1], r[2], r[4], r[3], r[5], r[6], 0, 0], np.float64), ""))
        for tok, name, b, attr in entries:
            Rg = G[:3, :3] @ _rot("z", math.degrees(float(b[6])))[:3, :3]
            tables["instance"].append({"token": f"inst_{tok}", "category_token": f"cat_{categories[str(name)]}"})
            tables["sample_annotation"].append({"token": tok, "sample_token": f"sample{k}", "instance_token": f"inst_{tok}",
                                                "attribute_tokens": [f"attr_{attr}"] if attr else [],
                                                "translation": (G[:3, :3] @ np.asarray(b[:3], np.float64) + G[:3, 3]).tolist(),
                                                "size": [float(b[4]), float(b[3]), float(b[5])], "rotation": _quat_of(Rg.tolist()),
                                                "num_lidar_pts": 9, "num_radar_pts": 0})
    for name, rows in tables.items():
        with open(root / VERSION / f"{name}.json", "w") as f:
            json.dump(rows, f)
    with open(root / "nuscenes_infos_10sweeps_val.pkl", "wb") as f:
        pickle.dump(infos, f)
    return root, infos


def dataset_cfg(data_path, version=VERSION):
    from toda_amd.pcdet.config import AttrDict
    return AttrDict({"DATASET": "NuScenesDataset", "DATA_PATH": str(data_path), "VERSION": version, "MAX_SWEEPS": 1, "PRED_VELOCITY": True,
                     "POINT_CLOUD_RANGE": [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], "DATA_SPLIT": {"train": "train", "test": "val"},
                     "INFO_PATH": {"train": ["nuscenes_infos_10sweeps_train.pkl"], "test": ["nuscenes_infos_10sweeps_val.pkl"]},
                     "POINT_FEATURE_ENCODING": {"encoding_type": "absolute_coordinates_encoding", "used_feature_list": ["x", "y", "z", "intensity", "timestamp"],
                                                "src_feature_list": ["x", "y", "z", "intensity", "timestamp"]},
                     "DATA_PROCESSOR": [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True}]})


def perfect_detections(infos):
    """A copy of every ground truth of a class (score 0.9 down in steps of 1/64 per sample) except the car beyond 50 m, which gets
    no prediction; the pedestrian with NaN velocity is predicted at rest.  The racked bicycle and the barrier beyond 30 m ARE
    copied: were they not filtered on both sides, they would match and their classes would score AP 1."""
    dets = []
    for k, info in enumerate(infos):
        boxes, _, names, _ = sample_gt(k)
        keep = [i for i in range(len(names)) if names[i] != "ignore" and not (k == 0 and i == 3)]
        b = np.nan_to_num(boxes[keep].astype(np.float64), nan=0.0)
        dets.append({"name": names[keep], "score": 0.9 - np.arange(len(keep)) / 64.0, "boxes_lidar": b, "pred_labels": np.ones(len(keep), np.int64),
                     "frame_id": f"s{k}", "metadata": {"token": info["token"]}})
    return dets


def perturbed_detections(infos, seed=5):
    """Moved, turned, resized copies with drawn scores (some equal), some ground truths missed, and false positives of every
    class, the samples in another order than the infos."""
    rng = np.random.default_rng(seed)
    dets = []
    for k in (2, 0, 1):
        boxes, _, names, _ = sample_gt(k)
        keep = [i for i in range(len(names)) if names[i] != "ignore" and rng.random() < 0.85]
        b = np.nan_to_num(boxes[keep].astype(np.float64), nan=0.0)
        b[:, :2] += rng.uniform(-1.6, 1.6, (len(keep), 2))
        b[:, 3:6] *= rng.uniform(0.8, 1.25, (len(keep), 3))
        b[:, 6] += rng.uniform(-0.5, 0.5, len(keep))
        b[:, 7:9] += rng.uniform(-0.4, 0.4, (len(keep), 2))
        extra = 12
        fp = np.concatenate([rng.uniform(-45, 45, (extra, 2)), rng.uniform(-1.5, 0, (extra, 1)), rng.uniform(0.5, 4.5, (extra, 3)),
                             rng.uniform(-3.1, 3.1, (extra, 1)), rng.uniform(-1, 1, (extra, 2))], 1)
        fp_names = np.array([CLASSES[(k + j) % 10] for j in range(extra)])
        fp[:2, :2] = b[:2, :2] + 0.25 if len(b) >= 2 else fp[:2, :2]           # two duplicates next to true positives
        fp_names[:2] = names[keep][:2] if len(b) >= 2 else fp_names[:2]
        score = np.maximum(np.round(rng.uniform(0.05, 0.95, len(keep) + extra) * 8), 1) / 8     # eighths: ties across and inside samples
        dets.append({"name": np.concatenate([names[keep], fp_names]), "score": score, "boxes_lidar": np.concatenate([b, fp], 0),
                     "pred_labels": np.ones(len(keep) + extra, np.int64), "frame_id": f"s{k}", "metadata": {"token": infos[k]["token"]}})
    return dets


def stated_attribute(name, speed):
    """The attribute a prediction is given in the submission."""
    if speed > 0.2 and name in ("car", "truck", "bus", "trailer", "construction_vehicle"):
        return "vehicle.moving"
    if speed > 0.2 and name in ("bicycle", "motorcycle"):
        return "cycle.with_rider"
    if not speed > 0.2 and name == "pedestrian":
        return "pedestrian.standing"
    if not speed > 0.2 and name == "bus":
        return "vehicle.stopped"
    return {"car": "vehicle.parked", "truck": "vehicle.parked", "trailer": "vehicle.parked", "construction_vehicle": "vehicle.parked",
            "bus": "vehicle.moving", "pedestrian": "pedestrian.moving", "bicycle": "cycle.without_rider", "motorcycle": "cycle.without_rider",
            "barrier": "", "traffic_cone": ""}[name]


def restate_evaluation(infos, dets):
    """The restatement on the mini tree's own ingredients (poses, sample_gt, the rack) and a list of detections."""
    by_token = {d["metadata"]["token"]: d for d in dets}
    order = {d["metadata"]["token"]: k for k, d in enumerate(dets)}
    samples = [None] * len(dets)
    for k, info in enumerate(infos):
        G = (np.linalg.inv(info["car_from_global"]) @ np.linalg.inv(info["ref_from_car"])).tolist()
        ego = np.linalg.inv(info["car_from_global"])[:3, 3].tolist()
        boxes, vel, names, attrs = sample_gt(k)
        gts = []
        for i in range(len(names)):
            g = to_global([float(v) for v in boxes[i, :7]] + [float(v) for v in vel[i]], G, ego)
            gts.append((str(names[i]), dict(g, attr=attrs[i])))
        racks = []
        if k == 0:
            r = RACK_OF_SAMPLE_0
            rg = to_global([r[0], r[1], r[2], 0, 0, 0, r[6], 0, 0, 0], G, ego)
            Rg = (np.asarray(G)[:3, :3] @ _rot("z", math.degrees(r[6]))[:3, :3]).tolist()
            racks.append((rg["c"], [r[3], r[4], r[5]], _quat_of(Rg)))
        det = by_token[info["token"]]
        preds = []
        for i in range(len(det["name"])):
            row = [float(v) for v in det["boxes_lidar"][i, :7]] + [float(v) for v in det["boxes_lidar"][i, 7:9]] + [0.0]
            p = to_global(row, G, ego)
            name = str(det["name"][i])
            preds.append((name, dict(p, score=float(det["score"][i]), attr=stated_attribute(name, math.sqrt(p["v"][0] ** 2 + p["v"][1] ** 2)))))
        samples[order[info["token"]]] = {"preds": preds, "gts": gts, "racks": racks}
    return metric(samples)
