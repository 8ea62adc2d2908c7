"""The KITTI evaluator's overlap and matching rules restated in numpy (fp64 or fp32), as a yardstick for the HIP kernels
and as the host baseline of tools/bench_kitti_eval.py; plus the seeded annotation generators, the fixture (un)packing and the
screening the capture script and the tests share.  Written from the algorithm: corners inside the other rectangle with no
margin (a corner equal to a corner of the other rectangle is on it, whatever the rounding of the dot products says),
strict-sign edge crossings, an angular sort about the centroid, a triangle fan; greedy matching by a stateless rule."""
import math

import numpy as np

GOLDEN_LEVELS = (0.25, 0.5, 0.7)
KITTI_CLASSES = ["Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "Truck"]


# ---- overlaps ---------------------------------------------------------------------------------------------------------

def _from(o, p):
    return (p[0] - o[0], p[1] - o[1])


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1]


def _det(u, v):
    return u[0] * v[1] - v[0] * u[1]


def _turn(o, u, v):
    """Orientation predicate: seen from o, u strictly on the turning side of v; a zero determinant is False."""
    s, t = _from(o, u), _from(o, v)
    return s[1] * t[0] > t[1] * s[0]


def _rect(r, T):
    """Corners (-,-) (-,+) (+,+) (+,-) of (cx, cy, dx, dy, angle), turned clockwise by the angle."""
    co, si = T(math.cos(float(r[4]))), T(math.sin(float(r[4])))
    hx, hy = r[2] / T(2), r[3] / T(2)
    return [(co * lx + si * ly + r[0], -si * lx + co * ly + r[1]) for lx, ly in ((-hx, -hy), (-hx, hy), (hx, hy), (hx, -hy))]


def _holds(rect, p):
    """p in the closed rectangle: its offset from corner 0 projects into [0, |side|^2] on both sides leaving corner 0; a
    point equal to a corner is in whatever the rounding says."""
    if any(p[0] == k[0] and p[1] == k[1] for k in rect):
        return True
    off = _from(rect[0], p)
    for side in (1, 3):
        e = _from(rect[0], rect[side])
        len2, proj = _dot(e, e), _dot(e, off)
        if not (len2 >= proj and proj >= 0):
            return False
    return True


def _meet(a, b, c, d):
    """Proper crossing of segments a-b and c-d (strict on both), as the intersection of the carrier lines, or None."""
    if _turn(a, d, c) == _turn(b, d, c) or _turn(a, c, b) == _turn(a, d, b):
        return None
    s, t = _from(a, b), _from(c, d)
    wa, wc = _det(a, b), _det(c, d)
    den = s[1] * t[0] - s[0] * t[1]
    return ((wa * t[0] - s[0] * wc) / den, (wa * t[1] - s[1] * wc) / den)


def rect_inter(a, b, dtype=np.float64):
    """Intersection area of two rectangles (cx, cy, dx, dy, angle clockwise-positive); `a` is the first operand."""
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        p, q = _rect([T(v) for v in a], T), _rect([T(v) for v in b], T)
        pts = []
        for k in range(4):
            if _holds(q, p[k]):
                pts.append(p[k])
            if _holds(p, q[k]):
                pts.append(q[k])
        for i in range(4):
            for j in range(4):
                at = _meet(p[i], p[(i + 1) % 4], q[j], q[(j + 1) % 4])
                if at is not None:
                    pts.append(at)
        n = len(pts)
        if n < 3:
            return T(0)
        mx, my = T(0), T(0)
        for x, y in pts:
            mx, my = mx + x, my + y
        mean = (mx / T(n), my / T(n))
        keys = []
        for pt in pts:
            dx, dy = _from(mean, pt)
            length = np.sqrt(dx * dx + dy * dy)
            dx, dy = dx / length, dy / length
            keys.append(T(-2) - dx if dy < 0 else dx)
        order = list(range(n))                   # a stable index sort by hand, not sorted(): a NaN key must stay in place
        for i in range(1, n):
            moving, slot = order[i], i
            while slot > 0 and keys[order[slot - 1]] > keys[moving]:
                order[slot] = order[slot - 1]
                slot -= 1
            order[slot] = moving
        apex, area = pts[order[0]], T(0)
        for i in range(1, n - 1):
            u, v = pts[order[i]], pts[order[i + 1]]
            area = area + abs(((apex[0] - v[0]) * (u[1] - v[1]) - (apex[1] - v[1]) * (u[0] - v[0])) / T(2))
        return area


def _norm(inter, first, second, criterion):
    with np.errstate(all="ignore"):
        if criterion == -1:
            return inter / (first + second - inter)
        if criterion == 0:
            return inter / first
        if criterion == 1:
            return inter / second
        return inter


def overlaps(box3d, bbox, q3d, qbbox, metric, criterion=-1, dtype=np.float32):
    """[n_box, n_query] overlaps; box3d rows x, y, z, l, h, w, ry; bbox rows x1, y1, x2, y2.  dtype: the arithmetic of the
    image and rotated parts (the vertical part of metric 2 is fp64 on the rounded area, as in the kernel)."""
    T = np.dtype(dtype).type
    n, k = (len(bbox), len(qbbox)) if metric == 0 else (len(box3d), len(q3d))
    out = np.zeros((n, k), dtype)
    for i in range(n):
        for j in range(k):
            if metric == 0:
                b, q = [T(v) for v in bbox[i]], [T(v) for v in qbbox[j]]
                iw, ih = min(b[2], q[2]) - max(b[0], q[0]), min(b[3], q[3]) - max(b[1], q[1])
                if iw > 0 and ih > 0:
                    ba, qa = (b[2] - b[0]) * (b[3] - b[1]), (q[2] - q[0]) * (q[3] - q[1])
                    ua = {-1: ba + qa - iw * ih, 0: ba, 1: qa}.get(criterion, T(1))
                    out[i, j] = iw * ih / ua
                continue
            b, q = [T(v) for v in box3d[i]], [T(v) for v in q3d[j]]
            rb, rq = [b[0], b[2], b[3], b[5], b[6]], [q[0], q[2], q[3], q[5], q[6]]
            inter = rect_inter(rq, rb, dtype)
            if metric == 1:
                out[i, j] = _norm(inter, rq[2] * rq[3], rb[2] * rb[3], criterion)
            elif inter > 0:
                b, q, inter = [float(v) for v in b], [float(v) for v in q], float(inter)
                ih = min(b[1], q[1]) - max(b[1] - b[4], q[1] - q[4])
                if ih > 0:
                    vb, vq, inc = b[3] * b[4] * b[5], q[3] * q[4] * q[5], ih * inter
                    out[i, j] = inc / {-1: vb + vq - inc, 0: vb, 1: vq}.get(criterion, inc)
    return out


# ---- matching ---------------------------------------------------------------------------------------------------------

def match_frame(ov, ign_gt, ign_det, score, min_overlap, thresh=0.0, compute_fp=False, metric=1, det_bbox=None, dc_bbox=None,
                compute_aos=False, gt_alpha=None, det_alpha=None):
    """One frame at one threshold -> (tp, fp, fn, similarity, matched scores).  ov [n_det, n_gt]."""
    ov = np.asarray(ov, np.float64)
    nd, ng = len(ign_det), len(ign_gt)
    assigned = np.zeros(nd, bool)
    under = (score < thresh) if compute_fp else np.zeros(nd, bool)
    tp = fn = 0
    sim, matched = [], []
    for i in range(ng):
        if ign_gt[i] == -1:
            continue
        cand = (ign_det != -1) & ~assigned & ~under & (ov[:, i] > min_overlap) if nd else np.zeros(0, bool)
        if not cand.any():
            fn += int(ign_gt[i] == 0)
            continue
        if compute_fp:
            counted = cand & (ign_det == 0)
            j = int(np.argmax(np.where(counted, ov[:, i], -np.inf))) if counted.any() else int(np.flatnonzero(cand)[0])
        else:
            j = int(np.argmax(np.where(cand, score, -np.inf)))
        assigned[j] = True
        if ign_gt[i] == 1 or ign_det[j] == 1:
            continue
        tp += 1
        matched.append(score[j])
        if compute_aos:
            sim.append((1.0 + math.cos(gt_alpha[i] - det_alpha[j])) / 2.0)
    fp = 0
    if compute_fp:
        for j in np.flatnonzero(~assigned & (ign_det == 0) & ~under):
            stuff = False
            if metric == 0:
                b = det_bbox[j]
                for q in dc_bbox:
                    iw, ih = min(b[2], q[2]) - max(b[0], q[0]), min(b[3], q[3]) - max(b[1], q[1])
                    if iw > 0 and ih > 0 and iw * ih / ((b[2] - b[0]) * (b[3] - b[1])) > min_overlap:
                        stuff = True
                        break
            fp += not stuff
    return tp, fp, fn, float(np.sum(sim)) if sim else 0.0, matched


class HostBackend:
    """The evaluator's three device steps in numpy (see eval.DeviceBackend), arithmetic of the overlaps in `dtype`."""
    dtype = np.float32

    def __init__(self, prep):
        self.p, self.ov = prep, {}

    def _frames(self):
        p = self.p
        for f in range(p["n_frames"]):
            yield f, slice(p["dt_off"][f], p["dt_off"][f + 1]), slice(p["gt_off"][f], p["gt_off"][f + 1])

    def overlaps(self, metric):
        p = self.p
        self.ov[metric] = [overlaps(p["dt_box3d"][d], p["dt_bbox"][d], p["gt_box3d"][g], p["gt_bbox"][g], metric, -1, self.dtype)
                           for _, d, g in self._frames()]

    def match_scores(self, metric, ign_gt, ign_det, min_overlap):
        out = []
        for f, d, g in self._frames():
            out += match_frame(self.ov[metric][f], ign_gt[g], ign_det[d], self.p["score"][d], min_overlap)[4]
        return np.array(out, np.float64)

    def match(self, metric, ign_gt, ign_det, thresholds, min_overlap, compute_aos):
        p, pr = self.p, np.zeros((len(thresholds), 4))
        for f, d, g in self._frames():
            dc = p["dc_bbox"][p["dc_off"][f]:p["dc_off"][f + 1]]
            for t, th in enumerate(thresholds):
                pr[t] += match_frame(self.ov[metric][f], ign_gt[g], ign_det[d], p["score"][d], min_overlap, th, True, metric,
                                     p["dt_bbox"][d], dc, compute_aos, p["gt_alpha"][g], p["dt_alpha"][d])[:4]
        return pr


class HostBackend64(HostBackend):
    dtype = np.float64


# ---- annotations: generators, packing, screening --------------------------------------------------------------------------

SIZES = {"Car": (3.9, 1.56, 1.6), "Van": (5.0, 2.2, 1.9), "Truck": (9.0, 3.2, 2.6), "Pedestrian": (0.8, 1.75, 0.6),
         "Person_sitting": (0.8, 1.25, 0.6), "Cyclist": (1.76, 1.73, 0.6)}          # l, h, w
SIBLING = {"Car": "Van", "Van": "Car", "Pedestrian": "Person_sitting", "Person_sitting": "Pedestrian"}
ANNO_KEYS = ("bbox", "alpha", "location", "dimensions", "rotation_y", "occluded", "truncated", "score")


def _anno(rows, with_score):
    keys = [k for k in ANNO_KEYS if with_score or k != "score"]
    a = {"name": np.array([r["name"] for r in rows], dtype="<U16")}
    for k in keys:
        width = {"bbox": (0, 4), "location": (0, 3), "dimensions": (0, 3)}.get(k, (0,))
        a[k] = np.array([r[k] for r in rows], np.float64) if rows else np.zeros(width)
    return a


def _image_box(rng, loc, dims):
    """A pinhole-looking box: centre and height from the depth, so near objects are tall and far ones short."""
    x, y, z = loc
    h_px = 720.0 * dims[1] / z
    w_px = 720.0 * max(dims[0], dims[2]) * rng.uniform(0.5, 1.0) / z
    cx, cy = 620.0 + 720.0 * x / z, 180.0 + 720.0 * (y - dims[1] / 2) / z
    return [cx - w_px / 2, cy - h_px / 2, cx + w_px / 2, cy + h_px / 2]


def kitti_frames(seed, n_frames=40, classes=("Car", "Van", "Pedestrian", "Person_sitting", "Cyclist", "Truck"), mean_gt=6,
                 extra_det=3, dontcare=True):
    """Seeded camera-frame annotations: (gt_annos, dt_annos).  Frame 3 has no ground truth, frame 5 no detections, frame 7
    neither; occlusion 0..3 and truncation 0..0.6 span the three difficulties; detections are jittered ground truths (some
    with the sibling class), free false positives and boxes inside DontCare regions."""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for f in range(n_frames):
        g_rows, d_rows = [], []
        n_gt = 0 if f in (3, 7) else int(rng.integers(1, 2 * mean_gt))
        for _ in range(n_gt):
            name = classes[int(rng.integers(len(classes)))]
            dims = np.array(SIZES[name]) * rng.uniform(0.85, 1.15, 3)
            loc = np.array([rng.uniform(-20, 20), rng.uniform(1.4, 1.9), rng.uniform(6, 70)])
            ry = rng.uniform(-np.pi, np.pi)
            g_rows.append({"name": name, "location": loc, "dimensions": dims, "rotation_y": ry,
                           "alpha": ry - np.arctan2(loc[0], loc[2]), "bbox": _image_box(rng, loc, dims),
                           "occluded": float(rng.integers(0, 4)), "truncated": float(rng.choice([0.0, 0.1, 0.2, 0.4, 0.6]))})
        n_obj = len(g_rows)
        for _ in range(int(rng.integers(0, 3)) if dontcare and n_gt else 0):
            x1, y1 = rng.uniform(0, 1000), rng.uniform(100, 300)
            g_rows.append({"name": "DontCare", "location": [-1000.0] * 3, "dimensions": [-1.0] * 3, "rotation_y": -10.0, "alpha": -10.0,
                           "bbox": [x1, y1, x1 + rng.uniform(40, 200), y1 + rng.uniform(30, 80)], "occluded": -1.0, "truncated": -1.0})
        if f not in (5, 7):
            for g in g_rows[:n_obj]:
                if rng.uniform() < 0.2:
                    continue
                noise = rng.choice([0.05, 0.15, 0.4])
                loc = g["location"] + rng.normal(0, noise, 3) * [1, 0.3, 1]
                dims = g["dimensions"] * rng.uniform(0.92, 1.08, 3)
                ry = g["rotation_y"] + rng.normal(0, 0.08) + (np.pi if rng.uniform() < 0.1 else 0.0)
                name = SIBLING.get(g["name"], g["name"]) if rng.uniform() < 0.12 else g["name"]
                d_rows.append({"name": name, "location": loc, "dimensions": dims, "rotation_y": ry,
                               "alpha": ry - np.arctan2(loc[0], loc[2]),
                               "bbox": list(np.array(g["bbox"]) + rng.normal(0, 1.0 + 20 * noise, 4)), "occluded": 0.0, "truncated": 0.0})
            for _ in range(int(rng.integers(0, 2 * extra_det))):
                name = classes[int(rng.integers(len(classes)))]
                dims = np.array(SIZES[name]) * rng.uniform(0.85, 1.15, 3)
                loc = np.array([rng.uniform(-20, 20), rng.uniform(1.4, 1.9), rng.uniform(6, 70)])
                ry = rng.uniform(-np.pi, np.pi)
                d_rows.append({"name": name, "location": loc, "dimensions": dims, "rotation_y": ry,
                               "alpha": ry - np.arctan2(loc[0], loc[2]), "bbox": _image_box(rng, loc, dims), "occluded": 0.0, "truncated": 0.0})
            for g in g_rows[n_obj:]:             # a detection inside each DontCare region: not a false positive for bbox
                if d_rows and rng.uniform() < 0.7:
                    b = np.array(g["bbox"])
                    row = dict(d_rows[int(rng.integers(len(d_rows)))])
                    row["location"] = row["location"] + np.array([40.0, 0, 0])
                    row["bbox"] = [b[0] + 2, b[1] + 2, b[2] - 2, b[3] - 2]
                    d_rows.append(row)
            for r in d_rows:
                r["score"] = rng.uniform(0.05, 1.0)
        gts.append(_anno(g_rows, False))
        dts.append(_anno(d_rows, True))
    return gts, dts


def lidar_frames(seed, n_frames=12, names=("car", "truck", "pedestrian", "barrier"), mean_gt=8, max_fp=5):
    """Seeded LiDAR-frame infos and detection annos in the layout the LiDAR-only datasets hand to
    transform_annotations_to_kitti_format: gt_boxes_lidar / gt_names, boxes_lidar / name / score."""
    rng = np.random.default_rng(seed)
    size = {"car": (4.6, 1.9, 1.7), "truck": (8.0, 2.8, 3.0), "pedestrian": (0.7, 0.7, 1.8), "barrier": (0.5, 2.5, 1.0),
            "bicycle": (1.8, 0.6, 1.4)}
    infos, dets = [], []
    for f in range(n_frames):
        n = int(rng.integers(0 if f == 2 else 1, 2 * mean_gt))
        nm = np.array([names[int(i)] for i in rng.integers(0, len(names), n)], dtype="<U16")
        boxes = np.zeros((n, 7))
        boxes[:, 0], boxes[:, 1], boxes[:, 2] = rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(-1.5, 0.5, n)
        boxes[:, 3:6] = np.array([size[k] for k in nm]).reshape(n, 3) * rng.uniform(0.85, 1.15, (n, 3))
        boxes[:, 6] = rng.uniform(-np.pi, np.pi, n)
        keep = rng.uniform(size=n) < 0.8
        det = boxes[keep].copy()
        det[:, :3] += rng.normal(0, 1, (len(det), 3)) * rng.choice([0.05, 0.15, 0.4], (len(det), 1))
        det[:, 3:6] *= rng.uniform(0.92, 1.08, (len(det), 3))
        det[:, 6] += rng.normal(0, 0.08, len(det))
        n_fp = int(rng.integers(0, max_fp))
        fp = np.zeros((n_fp, 7))
        fp[:, 0], fp[:, 1], fp[:, 6] = rng.uniform(-50, 50, n_fp), rng.uniform(-50, 50, n_fp), rng.uniform(-np.pi, np.pi, n_fp)
        fp_nm = np.array([names[int(i)] for i in rng.integers(0, len(names), n_fp)], dtype="<U16")
        fp[:, 3:6] = np.array([size[k] for k in fp_nm]).reshape(n_fp, 3)
        det, det_nm = np.concatenate([det, fp], 0), np.concatenate([nm[keep], fp_nm])
        infos.append({"gt_boxes_lidar": boxes, "gt_names": nm})
        dets.append({"boxes_lidar": det, "name": det_nm.astype("<U16"), "score": rng.uniform(0.05, 1.0, len(det)), "frame_id": f})
    return infos, dets


def pack(annos, prefix):
    """A list of annos as flat arrays + offsets (npz-storable: no pickles)."""
    out = {f"{prefix}_off": np.concatenate([[0], np.cumsum([len(a["name"]) for a in annos])]).astype(np.int64),
           f"{prefix}_name": np.concatenate([np.asarray(a["name"], dtype="<U16") for a in annos]) if annos else np.zeros(0, "<U16")}
    for k in ANNO_KEYS:
        if all(k in a for a in annos):
            out[f"{prefix}_{k}"] = np.concatenate([np.asarray(a[k], np.float64) for a in annos], 0)
    return out


def unpack(z, prefix):
    off = z[f"{prefix}_off"]
    annos = []
    for f in range(len(off) - 1):
        a = {"name": z[f"{prefix}_name"][off[f]:off[f + 1]].copy()}
        for k in ANNO_KEYS:
            if f"{prefix}_{k}" in z:
                a[k] = z[f"{prefix}_{k}"][off[f]:off[f + 1]].copy()
        annos.append(a)
    return annos


def screen(overlap_blocks, dt_annos, levels=GOLDEN_LEVELS, margin=1e-3):
    """The fixtures' two conditions: no overlap within `margin` of a min_overlap level; no two detections of a frame share
    a score.  Returns (smallest distance to a level, frames with a shared score)."""
    gap = np.inf
    for block in overlap_blocks:
        b = np.asarray(block, np.float64).reshape(-1)
        for lv in levels:
            if b.size:
                gap = min(gap, float(np.abs(b - lv).min()))
    shared = sum(len(np.unique(a["score"])) != len(a["score"]) for a in dt_annos)
    return gap, shared
