"""The nuScenes detection metric (mAP, the five true-positive errors and NDS; public definition `detection_cvpr_2019`) as the
project's own code: `eval_metric: nds` of NuScenesDataset.  The reference hands this to the nuScenes devkit (`eval_metric:
nuscenes`, which keeps raising ImportError here); the devkit walks every prediction against every ground truth in Python.

    device  ops.nusc_eval_prepare   every box, prediction or ground truth, from the LiDAR frame to the global frame + range flag
            ops.nusc_eval_match     greedy centre-distance matching of every (sample, class) at 0.5 / 1 / 2 / 4 m, the five
                                    errors of the 2 m matches (csrc/nuscenes_eval.hip)
    host    the devkit tables (attributes of the ground truths, bike racks), the orders, the 40 precision / error curves
            (short fp64 vector passes), the two JSON files and the text

The ground truth comes from the info pickles.  They keep a ground truth's LiDAR-frame yaw only, so its global yaw is rebuilt
from the rotation of G = inv(car_from_global) . inv(ref_from_car); bike racks come from the tables, because a rack without a
LiDAR point is absent from the infos."""
import functools
import json
import time
from pathlib import Path

import numpy as np

CLASSES = ("car", "truck", "bus", "trailer", "construction_vehicle", "pedestrian", "motorcycle", "bicycle", "traffic_cone", "barrier")
DIST_THS = (0.5, 1.0, 2.0, 4.0)
DIST_TH_TP = 2.0
MIN_RECALL, MIN_PRECISION = 0.1, 0.1
MAX_BOXES_PER_SAMPLE = 500
MEAN_AP_WEIGHT = 5
TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")
ERR_ROW = {"trans_err": 0, "vel_err": 1, "scale_err": 2, "orient_err": 3, "attr_err": 4}      # rows of ops.nusc_eval_match's err
NAN_ENTRIES = {"traffic_cone": ("attr_err", "vel_err", "orient_err"), "barrier": ("attr_err", "vel_err")}
TABLES = ("attribute", "category", "instance", "sample_annotation")
RACK_CATEGORY = "static_object.bicycle_rack"
EVAL_VERSION = "detection_cvpr_2019"
NO_GT_TEXT = "No ground-truth annotations for evaluation"
DEFAULT_ATTRIBUTE = {"car": "vehicle.parked", "truck": "vehicle.parked", "trailer": "vehicle.parked", "construction_vehicle": "vehicle.parked",
                     "bus": "vehicle.moving", "pedestrian": "pedestrian.moving", "bicycle": "cycle.without_rider",
                     "motorcycle": "cycle.without_rider", "barrier": "", "traffic_cone": ""}
META = {"use_camera": False, "use_lidar": True, "use_radar": False, "use_map": False, "use_external": False}


# ---- rotations
def quat_to_matrix(q):
    """Rotation matrix of the unit quaternion (w, x, y, z)."""
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def matrix_to_quat(R):
    """Unit quaternion (w, x, y, z), w >= 0, of a rotation matrix."""
    return matrices_to_quats(np.asarray(R, np.float64)[None])[0]


def matrices_to_quats(R):
    """Unit quaternions (w, x, y, z), w >= 0, of a stack [n, 3, 3] of rotation matrices -> [n, 4]: per matrix the branch with the
    largest pivot, so no small divisor."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    d = np.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], 1)
    t = np.stack([d.sum(1), d[:, 0] - d[:, 1] - d[:, 2], d[:, 1] - d[:, 0] - d[:, 2], d[:, 2] - d[:, 0] - d[:, 1]], 1)
    k = np.argmax(t, 1)
    s = 2.0 * np.sqrt(1.0 + t[np.arange(len(R)), k])
    a, b, c = R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]            # 4 w x, 4 w y, 4 w z
    xy, xz, yz = R[:, 0, 1] + R[:, 1, 0], R[:, 0, 2] + R[:, 2, 0], R[:, 1, 2] + R[:, 2, 1]          # 4 x y, 4 x z, 4 y z
    branches = np.stack([np.stack([s * s / 4, a, b, c], 1), np.stack([a, s * s / 4, xy, xz], 1), np.stack([b, xy, s * s / 4, yz], 1),
                         np.stack([c, xz, yz, s * s / 4], 1)], 1)                                   # each row is s times the quaternion
    q = branches[np.arange(len(R)), k] / s[:, None]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.where(q[:, :1] < 0, -q, q)


def rot_z(h):
    c, s = np.cos(h), np.sin(h)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


# ---- the devkit tables
def load_tables(root, version):
    """{name: list of records} of <root>/<version>/{attribute,category,instance,sample_annotation}.json."""
    tables = {}
    for name in TABLES:
        path = Path(root) / version / f"{name}.json"
        if not path.exists():
            raise FileNotFoundError(f"nuScenes table {name}.json not found at {path}: eval_metric 'nds' reads the ground truths' attributes "
                                    f"and the bike racks from the tables {', '.join(TABLES)}")
        with open(path) as f:
            tables[name] = json.load(f)
    return tables


def annotation_index(tables):
    """(attribute name of every annotation token ('' without one), bike racks per sample token as (translation, size wlh,
    rotation matrix))."""
    attr_name = {a["token"]: a["name"] for a in tables["attribute"]}
    cat_name = {c["token"]: c["name"] for c in tables["category"]}
    inst_cat = {i["token"]: cat_name[i["category_token"]] for i in tables["instance"]}
    attr_of, racks = {}, {}
    for ann in tables["sample_annotation"]:
        toks = ann["attribute_tokens"]
        if len(toks) > 1:
            raise ValueError(f"annotation {ann['token']} carries {len(toks)} attributes; the detection metric knows at most one")
        attr_of[ann["token"]] = attr_name[toks[0]] if toks else ""
        if inst_cat[ann["instance_token"]] == RACK_CATEGORY:
            racks.setdefault(ann["sample_token"], []).append((np.array(ann["translation"], np.float64), np.array(ann["size"], np.float64),
                                                              quat_to_matrix(ann["rotation"])))
    return attr_of, racks


def in_racks(centres, racks):
    """[n] bool: centre (global xyz) inside one of the racks, boundary included, tested in the rack's own axes (x along the
    length, y along the width, z up)."""
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    hit = np.zeros(len(centres), bool)
    for trans, wlh, R in racks:
        local = (centres - trans) @ R                    # R^T (c - t), row-wise
        half = np.array([wlh[1], wlh[0], wlh[2]]) / 2
        hit |= (np.abs(local) <= half).all(1)
    return hit


# ---- predictions
def prediction_attribute(name, speed):
    """The attribute a submission states for a prediction: by speed where the class has a moving / standing pair, else the
    class's usual one ('' for barrier and traffic_cone, whose attributes the metric never reads)."""
    if speed > 0.2:
        if name in ("car", "construction_vehicle", "bus", "truck", "trailer"):
            return "vehicle.moving"
        if name in ("bicycle", "motorcycle"):
            return "cycle.with_rider"
    else:
        if name == "pedestrian":
            return "pedestrian.standing"
        if name == "bus":
            return "vehicle.stopped"
    return DEFAULT_ATTRIBUTE[name]


def submission_results(sample_tokens, counts, glob, rows, R, names, scores, attributes):
    """The `results` block of a nuScenes submission: {sample token: [box, ...]}.  counts[k] boxes belong to sample_tokens[k];
    per box glob [6] = global centre xyz, yaw, velocity xy, rows [>= 7] the LiDAR-frame box (for the size and the heading) and
    R [3, 3] the rotation LiDAR -> global, so that the box's rotation is R . Rz(heading)."""
    glob, rows = np.asarray(glob, np.float64).reshape(-1, 6), np.asarray(rows, np.float64)
    c, s = np.cos(rows[:, 6]), np.sin(rows[:, 6])
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    turned = np.stack([R[:, :, 0] * c[:, None] + R[:, :, 1] * s[:, None], R[:, :, 1] * c[:, None] - R[:, :, 0] * s[:, None], R[:, :, 2]], 2)   # R . Rz(h)
    trans, size, quat, vel = glob[:, :3].tolist(), rows[:, [4, 3, 5]].tolist(), matrices_to_quats(turned).tolist(), glob[:, 4:6].tolist()
    results, k = {}, 0
    for token, n in zip(sample_tokens, counts):
        results[token] = [{"sample_token": token, "translation": trans[i], "size": size[i], "rotation": quat[i], "velocity": vel[i],
                           "detection_name": names[i], "detection_score": float(scores[i]), "attribute_name": attributes[i]} for i in range(k, k + n)]
        k += n
    return results


# ---- curves
def cummean(x):
    """NaN-aware cumulative mean: NaNs are skipped (0 before the first number); all NaN gives ones."""
    x = np.asarray(x, np.float64)
    nan = np.isnan(x)
    if nan.all():
        return np.ones(len(x))
    total, count = np.cumsum(np.where(nan, 0.0, x)), np.cumsum(~nan)
    return np.divide(total, count, out=np.zeros(len(x)), where=count != 0)


def empty_curve():
    return {"precision": np.zeros(101), "confidence": np.zeros(101), **{k: np.ones(101) for k in TP_METRICS}}


def accumulate(tp, score, errs, npos):
    """The curves of one class and threshold.  tp [n] bool and score [n] in the global order (score descending), errs
    {metric: [n]} (read where tp; None: no error curves, for the thresholds whose errors the metric does not read), npos ground
    truths -> {precision, confidence, five error curves}, each [101]."""
    tp = np.asarray(tp, bool)
    score = np.asarray(score, np.float64)
    if npos == 0 or not tp.any():
        return empty_curve()
    tps, fps = np.cumsum(tp).astype(np.float64), np.cumsum(~tp).astype(np.float64)
    prec, rec = tps / (fps + tps), tps / float(npos)
    grid = np.linspace(0, 1, 101)
    out = {"precision": np.interp(grid, rec, prec, right=0), "confidence": np.interp(grid, rec, score, right=0)}
    tp_score = score[tp]
    for k in TP_METRICS if errs is not None else ():
        mean = cummean(np.asarray(errs[k], np.float64)[tp])
        out[k] = np.interp(out["confidence"][::-1], tp_score[::-1], mean[::-1])[::-1]
    return out


def calc_ap(curve):
    prec = curve["precision"][round(100 * MIN_RECALL) + 1:] - MIN_PRECISION
    return float(np.mean(np.maximum(prec, 0.0))) / (1.0 - MIN_PRECISION)


def calc_tp(curve, metric):
    first = round(100 * MIN_RECALL) + 1
    nonzero = np.nonzero(curve["confidence"])[0]
    last = int(nonzero[-1]) if len(nonzero) else 0
    if last < first:
        return 1.0
    return float(np.mean(curve[metric][first:last + 1]))


def summarise(curves, eval_time=0.0):
    """curves {(class, threshold): curve} -> the metrics_summary dict."""
    label_aps = {c: {str(t): calc_ap(curves[c, t]) for t in DIST_THS} for c in CLASSES}
    label_tp = {c: {m: (float("nan") if m in NAN_ENTRIES.get(c, ()) else calc_tp(curves[c, DIST_TH_TP], m)) for m in TP_METRICS} for c in CLASSES}
    mean_dist_aps = {c: float(np.mean(list(label_aps[c].values()))) for c in CLASSES}
    tp_errors = {m: float(np.nanmean([label_tp[c][m] for c in CLASSES])) for m in TP_METRICS}
    tp_scores = {m: max(1.0 - tp_errors[m], 0.0) for m in TP_METRICS}
    mean_ap = float(np.mean(list(mean_dist_aps.values())))
    return {"label_aps": label_aps, "label_tp_errors": label_tp, "mean_dist_aps": mean_dist_aps, "mean_ap": mean_ap, "tp_errors": tp_errors,
            "tp_scores": tp_scores, "nd_score": nd_score(mean_ap, tp_scores), "eval_time": float(eval_time)}


def nd_score(mean_ap, tp_scores):
    return float((MEAN_AP_WEIGHT * mean_ap + np.sum(list(tp_scores.values()))) / (MEAN_AP_WEIGHT + len(tp_scores)))


def format_results(metrics, class_names, version=EVAL_VERSION):
    """(text, dict) in the layout of the reference's report: per class the errors and the APs, then the means, mAP and NDS."""
    text = "----------------Nuscene %s results-----------------\n" % version
    for name in class_names:
        aps, errs = metrics["label_aps"][name], metrics["label_tp_errors"][name]
        text += f"***{name} error@{', '.join(k.split('_')[0] for k in errs)} | AP@{', '.join(aps)}\n"
        text += ", ".join("%.2f" % v for v in errs.values()) + " | " + ", ".join("%.2f" % (v * 100) for v in aps.values())
        text += f" | mean AP: {metrics['mean_dist_aps'][name]}\n"
    text += "--------------average performance-------------\n"
    details = {}
    for key, val in metrics["tp_errors"].items():
        text += "%s:\t %.4f\n" % (key, val)
        details[key] = val
    text += "mAP:\t %.4f\n" % metrics["mean_ap"]
    text += "NDS:\t %.4f\n" % metrics["nd_score"]
    details.update({"mAP": metrics["mean_ap"], "NDS": metrics["nd_score"]})
    return text, details


# ---- the evaluation
def sample_transforms(infos):
    """(G [S, 3, 4], R [S, 3, 3], ego [S, 3]): LiDAR -> global of every info, its rotation, and the ego position."""
    for key in ("ref_from_car", "car_from_global"):
        missing = [info.get("token", k) for k, info in enumerate(infos) if key not in info]
        if missing:
            raise KeyError(f"eval_metric 'nds' compares boxes in the global frame and needs 'ref_from_car' and 'car_from_global' in the infos "
                           f"(a stock preparation writes both); '{key}' is missing from {len(missing)} infos, first {missing[0]}")
    G, ego = np.empty((len(infos), 3, 4)), np.empty((len(infos), 3))
    for s, info in enumerate(infos):
        global_from_car = np.linalg.inv(np.asarray(info["car_from_global"], np.float64))
        G[s] = (global_from_car @ np.linalg.inv(np.asarray(info["ref_from_car"], np.float64)))[:3]
        ego[s] = global_from_car[:3, 3]
    return G, G[:, :, :3].copy(), ego


def _class_ids(names):
    index = {c: k for k, c in enumerate(CLASSES)}
    return np.array([index.get(str(n), -1) for n in names], np.int32).reshape(-1)


def _prepare(rows, sample, cls, G, ego):
    import torch

    from .... import ops
    dev = torch.device("cuda")
    out, keep = ops.nusc_eval_prepare(torch.from_numpy(np.ascontiguousarray(rows)).to(dev), torch.from_numpy(sample).to(dev),
                                      torch.from_numpy(cls).to(dev), torch.from_numpy(np.ascontiguousarray(G)).to(dev),
                                      torch.from_numpy(np.ascontiguousarray(ego)).to(dev))
    return out.cpu().numpy(), keep.cpu().numpy().astype(bool)


def _drop_racked(keep, cls, sample, centres, racks, tokens):
    """Clear keep for bicycles and motorcycles whose centre lies in a bike rack of their sample."""
    cycles = keep & np.isin(cls, (CLASSES.index("bicycle"), CLASSES.index("motorcycle")))
    for s in np.unique(sample[cycles]):
        boxes = racks.get(tokens[s])
        if boxes:
            rows = np.nonzero(cycles & (sample == s))[0]
            keep[rows[in_racks(centres[rows], boxes)]] = False
    return keep


def _segments(keep, sample, cls, n_samples):
    """Kept rows ordered by (sample, class), the order of `rows` inside a segment unchanged -> (rows, CSR offsets [S * 10 + 1])."""
    rows = np.nonzero(keep)[0]
    key = sample[rows].astype(np.int64) * len(CLASSES) + cls[rows]
    rows = rows[np.argsort(key, kind="stable")]
    counts = np.bincount(sample[rows].astype(np.int64) * len(CLASSES) + cls[rows], minlength=n_samples * len(CLASSES))
    return rows, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def match_on_device(pred, score, pred_attr, gt, gt_attr, pred_off, gt_off, seg_cls):
    """ops.nusc_eval_match on host arrays -> (match [4, n_pred], err [5, n_pred]) as numpy."""
    import torch

    from .... import ops
    dev = torch.device("cuda")
    up = functools.partial(ops.eval_upload, dev=dev)
    match, err = ops.nusc_eval_match(up(pred, np.float64), up(score, np.float64), up(pred_attr, np.int32), up(gt, np.float64),
                                     up(gt_attr, np.int32), pred_off, gt_off, seg_cls, DIST_THS, DIST_THS.index(DIST_TH_TP))
    return match.cpu().numpy(), err.cpu().numpy()


def evaluate(infos, det_annos, class_names, root_path, version, output_path, logger=None, match_fn=match_on_device):
    """`eval_metric: nds`: writes results_nusc.json (and, with ground truth, metrics_summary.json) under output_path and
    returns (text, {trans_err, ..., mAP, NDS}).  root_path is the directory that holds the infos, the tables lie in
    root_path / version."""
    start = time.time()
    tokens = [info["token"] for info in infos]
    det_tokens = [det["metadata"]["token"] for det in det_annos]
    if len(set(tokens)) != len(tokens) or sorted(det_tokens) != sorted(tokens):
        extra, lacking = sorted(set(det_tokens) - set(tokens)), sorted(set(tokens) - set(det_tokens))
        raise ValueError(f"eval_metric 'nds': the detections must cover exactly the {len(tokens)} samples of the infos, each once "
                         f"({len(det_tokens)} given, {len(extra)} unknown tokens such as {extra[:1]}, {len(lacking)} samples without detections such as {lacking[:1]})")
    for det in det_annos:
        if len(det["name"]) > MAX_BOXES_PER_SAMPLE:
            raise ValueError(f"eval_metric 'nds': sample {det['metadata']['token']} has {len(det['name'])} predictions, the metric allows {MAX_BOXES_PER_SAMPLE}")
    G, R, ego = sample_transforms(infos)
    index_of = {tok: s for s, tok in enumerate(tokens)}

    # predictions, in det_annos order: that position is the index of the score ties
    counts = [len(det["name"]) for det in det_annos]
    n_pred = int(np.sum(counts))
    p_rows = np.zeros((n_pred, 10))
    lo = 0
    for det, n in zip(det_annos, counts):
        if n == 0:                                       # a frame without detections: its box array may have any width
            continue
        boxes = np.asarray(det["boxes_lidar"], np.float64).reshape(n, -1)
        p_rows[lo:lo + n, :7] = boxes[:, :7]
        if boxes.shape[1] >= 9:
            p_rows[lo:lo + n, 7:9] = boxes[:, 7:9]
        lo += n
    p_sample = np.repeat(np.array([index_of[t] for t in det_tokens], np.int32), counts).astype(np.int32)
    p_names = [str(n) for det in det_annos for n in det["name"]]
    p_cls = _class_ids(p_names)
    p_score = np.concatenate([np.asarray(det["score"], np.float64).reshape(-1) for det in det_annos] + [np.zeros(0)])
    if not np.isfinite(p_score).all():
        raise ValueError("eval_metric 'nds': a prediction's score is not finite")
    p_out, p_keep = _prepare(p_rows, p_sample, p_cls, G, ego)
    speed = np.sqrt(p_out[:, 4] ** 2 + p_out[:, 5] ** 2)
    p_attr_name = [prediction_attribute(n, v) if c >= 0 else "" for n, v, c in zip(p_names, speed, p_cls)]

    output_path = Path(output_path)
    output_path.mkdir(exist_ok=True, parents=True)
    results = submission_results(det_tokens, counts, p_out, p_rows, R[p_sample], p_names, p_score, p_attr_name)
    res_path = output_path / "results_nusc.json"
    with open(res_path, "w") as f:
        f.write(json.dumps({"results": results, "meta": dict(META)}))      # dumps, not dump: one pass of the C encoder over ~2 M boxes
    if logger is not None:
        logger.info(f"The predictions of NuScenes have been saved to {res_path}")
    if version == "v1.0-test" or any("gt_boxes" not in info for info in infos):
        return NO_GT_TEXT, {}

    # ground truths
    attr_of, racks = annotation_index(load_tables(root_path, version))
    g_counts = [len(info["gt_boxes"]) for info in infos]
    n_gt = int(np.sum(g_counts))
    g_rows = np.zeros((n_gt, 10))
    g_names, g_attr_name = [], []
    lo = 0
    for info, n in zip(infos, g_counts):
        if n == 0:
            continue
        g_rows[lo:lo + n, :7] = np.asarray(info["gt_boxes"], np.float64).reshape(n, -1)[:, :7]
        velocity = np.asarray(info["gt_boxes_velocity"], np.float64).reshape(n, -1)
        g_rows[lo:lo + n, 7:7 + velocity.shape[1]] = velocity[:, :3]
        g_names += [str(v) for v in info["gt_names"]]
        for tok in info["gt_boxes_token"]:
            if str(tok) not in attr_of:
                raise KeyError(f"ground truth {tok} of sample {info['token']} is not in sample_annotation.json")
            g_attr_name.append(attr_of[str(tok)])
        lo += n
    g_sample = np.repeat(np.arange(len(infos), dtype=np.int32), g_counts).astype(np.int32)
    g_cls = _class_ids(g_names)
    g_out, g_keep = _prepare(g_rows, g_sample, g_cls, G, ego)
    p_keep = _drop_racked(p_keep, p_cls, p_sample, p_out[:, :3], racks, tokens)
    g_keep = _drop_racked(g_keep, g_cls, g_sample, g_out[:, :3], racks, tokens)

    attr_id = {name: k for k, name in enumerate(sorted(set(g_attr_name) | set(p_attr_name))) if name}
    p_attr = np.array([attr_id.get(a, -1) for a in p_attr_name], np.int32).reshape(-1)
    g_attr = np.array([attr_id.get(a, -1) for a in g_attr_name], np.int32).reshape(-1)
    p_sel, p_off = _segments(p_keep, p_sample, p_cls, len(infos))
    g_sel, g_off = _segments(g_keep, g_sample, g_cls, len(infos))
    box = lambda out, rows, sel: np.concatenate([out[sel][:, [0, 1, 3, 4, 5]], rows[sel][:, 3:6]], 1)     # noqa: E731
    seg_cls = np.tile(np.arange(len(CLASSES), dtype=np.int32), len(infos))
    match, err = match_fn(box(p_out, p_rows, p_sel), p_score[p_sel], p_attr[p_sel], box(g_out, g_rows, g_sel), g_attr[g_sel], p_off, g_off, seg_cls)

    curves = {}
    for c, name in enumerate(CLASSES):
        mine = np.nonzero(p_cls[p_sel] == c)[0]
        order = mine[np.lexsort((-p_sel[mine], -p_score[p_sel[mine]]))]                 # score descending, then index descending
        npos = int(np.sum(g_cls[g_sel] == c))
        errs = {m: err[ERR_ROW[m]][order] for m in TP_METRICS}
        for t, th in enumerate(DIST_THS):
            curves[name, th] = accumulate(match[t][order] >= 0, p_score[p_sel[order]], errs if th == DIST_TH_TP else None, npos)
    metrics = summarise(curves, eval_time=time.time() - start)
    with open(output_path / "metrics_summary.json", "w") as f:
        json.dump(metrics, f, indent=2)
    return format_results(metrics, [c for c in class_names if c in CLASSES], version=EVAL_VERSION)
