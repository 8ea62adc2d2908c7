"""KITTI AP evaluation (reference pcdet/datasets/kitti/kitti_object_eval_python/eval.py), the metric every dataset's
`eval_metric: kitti` goes through: AP_bbox / AP_BEV / AP_3D / AOS at 11 and 40 recall points per class and difficulty.

The pairwise overlaps and the greedy matching run on the GPU (toda_amd/csrc/kitti_eval.hip through ops.eval_overlaps,
ops.eval_match_scores, ops.eval_match): one overlap launch per metric over all frames, and per (class, difficulty,
min_overlap) one threshold-free matching launch plus one launch over every (frame, threshold) pair.  What stays on the host,
in numpy over the flat arrays of all frames: class / difficulty filtering (clean_data), the recall-sampled score thresholds
(get_thresholds), the running maximum over the precision curve, the means and the text.

`eval_class` and `get_official_eval_result` take a `backend` class; the default is the device one below, the tests pass a
numpy restatement with the same three methods."""
import functools

import numpy as np

CLASS_TO_NAME = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting", 5: "Truck"}
MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
N_SAMPLE_PTS = 41
# [overlap level, metric (bbox, bev, 3d), class]
MIN_OVERLAPS = np.array([[[0.7, 0.5, 0.5, 0.7, 0.5, 0.7], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7]],
                         [[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]]])


def get_thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """The score thresholds at which recall reaches 0, 1/40, 2/40, ...  The matched scores are ranked downwards; a target
    recall starts at 0 and moves on by one sample step whenever a score is kept.  A score is left out when the next one
    brings the recall (rank / num_gt) nearer to the target than this one does; the last score is always kept."""
    ranked = -np.sort(-np.asarray(scores, dtype=np.float64))
    step = 1 / (num_sample_pts - 1.0)
    target, kept = 0, []
    for rank, score in enumerate(ranked, start=1):
        if rank < len(ranked):
            here, after = rank / num_gt, (rank + 1) / num_gt
            if after - target < target - here:
                continue
        kept.append(score)
        target += step
    return kept


def _flags(gt_name, gt_height, occluded, truncated, dt_name, dt_height, current_class, difficulty):
    """ignored_gt / ignored_det (-1 another class, 0 counts, 1 ignored) for flat arrays of lower-case names."""
    cls = CLASS_TO_NAME[current_class].lower()
    valid = np.where(gt_name == cls, 1, -1)
    if cls == "pedestrian":
        valid[gt_name == "person_sitting"] = 0
    elif cls == "car":
        valid[gt_name == "van"] = 0
    hard = (occluded > MAX_OCCLUSION[difficulty]) | (truncated > MAX_TRUNCATION[difficulty]) | (gt_height <= MIN_HEIGHT[difficulty])
    ign_gt = np.full(len(gt_name), -1, np.int32)
    ign_gt[(valid == 0) | ((valid == 1) & hard)] = 1
    ign_gt[(valid == 1) & ~hard] = 0
    ign_det = np.where(dt_name == cls, 0, -1).astype(np.int32)
    ign_det[dt_height < MIN_HEIGHT[difficulty]] = 1          # the height test comes first, whatever the class
    return ign_gt, ign_det


def _lower(names):
    return np.array([str(n).lower() for n in names], dtype=object)


def clean_data(gt_anno, dt_anno, current_class, difficulty):
    """One frame: (number of counted ground truths, ignored_gt, ignored_det, DontCare image boxes)."""
    gt_bbox = np.asarray(gt_anno["bbox"], np.float64).reshape(-1, 4)
    dt_bbox = np.asarray(dt_anno["bbox"], np.float64).reshape(-1, 4)
    ign_gt, ign_det = _flags(_lower(gt_anno["name"]), gt_bbox[:, 3] - gt_bbox[:, 1], np.asarray(gt_anno["occluded"]),
                             np.asarray(gt_anno["truncated"]), _lower(dt_anno["name"]), np.abs(dt_bbox[:, 3] - dt_bbox[:, 1]),
                             current_class, difficulty)
    dc = [gt_bbox[i] for i in range(len(gt_bbox)) if gt_anno["name"][i] == "DontCare"]
    return int((ign_gt == 0).sum()), ign_gt.tolist(), ign_det.tolist(), dc


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return off


def _cat(annos, key, width=None, dtype=np.float64):
    shape = (0,) if width is None else (0, width)
    parts = [np.asarray(a[key], dtype).reshape((-1,) + shape[1:]) for a in annos]
    return np.concatenate(parts, 0) if parts else np.zeros(shape, dtype)


def prepare(gt_annos, dt_annos):
    """All frames as flat arrays with CSR offsets: what the backends read."""
    assert len(gt_annos) == len(dt_annos)
    p = {"n_frames": len(gt_annos)}
    for side, annos in (("gt", gt_annos), ("dt", dt_annos)):
        p[f"{side}_off"] = _offsets([len(a["name"]) for a in annos])
        p[f"{side}_bbox"] = _cat(annos, "bbox", 4)
        p[f"{side}_alpha"] = _cat(annos, "alpha")
        p[f"{side}_box3d"] = np.concatenate([_cat(annos, "location", 3), _cat(annos, "dimensions", 3),
                                             _cat(annos, "rotation_y")[:, None]], 1)
        names = [n for a in annos for n in a["name"]]
        p[f"{side}_rawname"] = np.array(names, dtype=object)
        p[f"{side}_name"] = _lower(names)
    p["score"] = _cat(dt_annos, "score")
    p["occluded"] = _cat(gt_annos, "occluded")
    p["truncated"] = _cat(gt_annos, "truncated")
    is_dc = p["gt_rawname"] == "DontCare" if len(p["gt_rawname"]) else np.zeros(0, bool)
    frame_of_gt = np.repeat(np.arange(p["n_frames"]), np.diff(p["gt_off"]))
    p["dc_bbox"] = p["gt_bbox"][is_dc]
    p["dc_off"] = _offsets(np.bincount(frame_of_gt[is_dc], minlength=p["n_frames"]))
    p["ov_off"] = _offsets(np.diff(p["dt_off"]) * np.diff(p["gt_off"]))
    return p


class DeviceBackend:
    """The flat arrays on the GPU and the three device steps.  `stats` counts launches and uploads / read-backs; with
    `timed` every step is bracketed by device synchronisations and its seconds are added up (a measurement mode: the
    synchronisations serialise what otherwise overlaps)."""

    def __init__(self, prep, timed=False):
        import torch

        from ..... import ops
        self.ops, self.torch, self.p, self.timed = ops, torch, prep, timed
        self.stats = {"launches": 0, "transfers": 0, "overlap_s": 0.0, "match_s": 0.0, "transfer_s": 0.0}
        if not torch.cuda.is_available():
            raise RuntimeError("the KITTI evaluator's overlap and matching kernels need a GPU (there is no CPU path)")
        self.dev = torch.device("cuda", torch.cuda.current_device())
        up = self._up
        self.off = {k: up(prep[k], torch.int32) for k in ("gt_off", "dt_off", "dc_off")}
        self.ov_off = up(prep["ov_off"], torch.int64)
        self.box3d = {s: up(prep[f"{s}_box3d"], torch.float32) for s in ("gt", "dt")}
        self.bbox = {s: up(prep[f"{s}_bbox"], torch.float32) for s in ("gt", "dt")}
        self.f64 = {k: up(prep[k], torch.float64) for k in ("score", "dt_alpha", "gt_alpha", "dt_bbox", "dc_bbox")}
        self.ov = {}
        self._held = None                        # (ign_gt, ign_det) last uploaded, host copies and device tensors

    def _clock(self, key, t0=None):
        import time
        if not self.timed:
            return 0.0
        self.torch.cuda.synchronize()
        if t0 is not None:
            self.stats[key] += time.perf_counter() - t0
        return time.perf_counter()

    def _up(self, arr, dtype):
        t0 = self._clock("transfer_s")
        t = self.torch.from_numpy(np.ascontiguousarray(arr)).to(dtype).to(self.dev)
        self.stats["transfers"] += 1
        self._clock("transfer_s", t0)
        return t

    def _down(self, t):
        t0 = self._clock("transfer_s")
        a = t.cpu().numpy()
        self.stats["transfers"] += 1
        self._clock("transfer_s", t0)
        return a

    def _device_flags(self, ign_gt, ign_det):
        """The two flag arrays on the device; the pair uploaded last is kept, so the thresholded pass that follows a first
        pass with the same flags uploads nothing."""
        held = self._held
        if held is None or not (np.array_equal(held[0], ign_gt) and np.array_equal(held[1], ign_det)):
            self._held = (np.array(ign_gt, np.int32), np.array(ign_det, np.int32),
                          self._up(ign_gt, self.torch.int32), self._up(ign_det, self.torch.int32))
        return self._held[2], self._held[3]

    def overlaps(self, metric):
        t0 = self._clock("overlap_s")
        self.ov[metric] = self.ops.eval_overlaps(self.box3d["dt"], self.bbox["dt"], self.off["dt_off"], self.box3d["gt"],
                                                 self.bbox["gt"], self.off["gt_off"], self.ov_off, int(self.p["ov_off"][-1]),
                                                 metric, -1)
        self.stats["launches"] += 1
        self._clock("overlap_s", t0)

    def match_scores(self, metric, ign_gt, ign_det, min_overlap):
        ig, idt = self._device_flags(ign_gt, ign_det)
        t0 = self._clock("match_s")
        scores, counts = self.ops.eval_match_scores(self.ov[metric], self.ov_off, self.off["dt_off"], self.off["gt_off"], idt, ig,
                                                    self.f64["score"], float(min_overlap))
        self.stats["launches"] += 1
        self._clock("match_s", t0)
        scores, counts = self._down(scores), self._down(counts)
        start = self.p["gt_off"][:-1]
        keep = np.arange(len(scores)) < np.repeat(start + counts, np.diff(self.p["gt_off"]))
        return scores[keep]

    def match(self, metric, ign_gt, ign_det, thresholds, min_overlap, compute_aos):
        ig, idt = self._device_flags(ign_gt, ign_det)
        th = self._up(np.asarray(thresholds, np.float64), self.torch.float64)
        t0 = self._clock("match_s")
        pr = self.ops.eval_match(self.ov[metric], self.ov_off, self.off["dt_off"], self.off["gt_off"], idt, ig, self.f64["score"],
                                 self.f64["dt_alpha"], self.f64["gt_alpha"], self.f64["dt_bbox"], self.f64["dc_bbox"],
                                 self.off["dc_off"], th, float(min_overlap), metric, bool(compute_aos))
        self.stats["launches"] += 2
        self._clock("match_s", t0)
        return self._down(pr)


def _eval_prepared(backend, prep, current_classes, difficultys, metric, min_overlaps, compute_aos):
    shape = [len(current_classes), len(difficultys), len(min_overlaps), N_SAMPLE_PTS]
    precision, recall, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    counts = {}
    backend.overlaps(metric)
    gt_h = prep["gt_bbox"][:, 3] - prep["gt_bbox"][:, 1]
    dt_h = np.abs(prep["dt_bbox"][:, 3] - prep["dt_bbox"][:, 1])
    for m, current_class in enumerate(current_classes):
        for l, difficulty in enumerate(difficultys):
            ign_gt, ign_det = _flags(prep["gt_name"], gt_h, prep["occluded"], prep["truncated"], prep["dt_name"], dt_h,
                                     current_class, difficulty)
            num_valid_gt = int((ign_gt == 0).sum())
            for k, min_overlap in enumerate(min_overlaps[:, metric, m]):
                scores = backend.match_scores(metric, ign_gt, ign_det, min_overlap)
                thresholds = np.array(get_thresholds(scores, num_valid_gt))
                n = len(thresholds)
                pr = np.zeros((0, 4))
                if n:
                    pr = np.asarray(backend.match(metric, ign_gt, ign_det, thresholds, min_overlap, compute_aos), np.float64)
                counts[(m, l, k)] = (thresholds, pr)
                with np.errstate(divide="ignore", invalid="ignore"):
                    recall[m, l, k, :n] = pr[:, 0] / (pr[:, 0] + pr[:, 2])
                    precision[m, l, k, :n] = pr[:, 0] / (pr[:, 0] + pr[:, 1])
                    if compute_aos:
                        aos[m, l, k, :n] = pr[:, 3] / (pr[:, 0] + pr[:, 1])
                # the running maximum from the right, over all 41 points (np.max: a NaN anywhere to the right spreads)
                for curve in (precision, recall) + ((aos,) if compute_aos else ()):
                    for i in range(n):
                        curve[m, l, k, i] = np.max(curve[m, l, k, i:], axis=-1)
    return {"recall": recall, "precision": precision, "orientation": aos, "counts": counts}


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, num_parts=100,
               backend=None):
    """recall / precision / orientation [class, difficulty, overlap level, 41] for one metric (0 bbox, 1 bev, 2 3d).
    `counts` holds, per (class, difficulty, level) index, the thresholds and pr[T, 4] = (tp, fp, fn, similarity).
    num_parts is accepted for the reference's signature; only same-frame pairs are ever computed here."""
    prep = prepare(gt_annos, dt_annos)
    return _eval_prepared((backend or DeviceBackend)(prep), prep, current_classes, difficultys, metric, np.asarray(min_overlaps),
                          compute_aos)


def _mean_precision(curve, points, n_points):
    """100 x the mean of the chosen recall points of curve[..., 41], added up one point after the other."""
    columns = np.moveaxis(np.asarray(curve)[..., points], -1, 0)
    return functools.reduce(np.add, columns) / n_points * 100


def get_mAP(prec):
    """The 11-point AP: recall points 0, 4, ..., 40."""
    return _mean_precision(prec, slice(0, None, 4), 11)


def get_mAP_R40(prec):
    """The 40-point AP: recall points 1 ... 40."""
    return _mean_precision(prec, slice(1, None), 40)


def _class_ids(current_classes):
    """Class indices for a name, an index, or a sequence mixing both."""
    by_name = {name: idx for idx, name in CLASS_TO_NAME.items()}
    wanted = list(current_classes) if isinstance(current_classes, (list, tuple, np.ndarray)) else [current_classes]
    return [by_name[c] if isinstance(c, str) else int(c) for c in wanted]


def get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None, backend=None):
    current_classes = _class_ids(current_classes)
    min_overlaps = MIN_OVERLAPS[:, :, current_classes]
    # orientation is scored unless the first detection of the first non-empty frame carries the "no angle" value -10
    first_alpha = next((a["alpha"] for a in dt_annos if len(a["alpha"])), None)
    compute_aos = bool(first_alpha is not None and first_alpha[0] != -10)
    prep = prepare(gt_annos, dt_annos)
    be = (backend or DeviceBackend)(prep)
    ap, ap40 = {}, {}
    for metric, key in ((0, "bbox"), (1, "bev"), (2, "3d")):
        ret = _eval_prepared(be, prep, current_classes, [0, 1, 2], metric, min_overlaps, compute_aos and metric == 0)
        ap[key], ap40[key] = get_mAP(ret["precision"]), get_mAP_R40(ret["precision"])
        if PR_detail_dict is not None:
            PR_detail_dict[key] = ret["precision"]
        if metric == 0 and compute_aos:
            ap["aos"], ap40["aos"] = get_mAP(ret["orientation"]), get_mAP_R40(ret["orientation"])
            if PR_detail_dict is not None:
                PR_detail_dict["aos"] = ret["orientation"]

    def row(label, table, j, i, digits):
        return f"{label} AP:" + ", ".join(f"{table[j, d, i]:.{digits}f}" for d in range(3)) + "\n"

    result, ret_dict = "", {}
    for j, curcls in enumerate(current_classes):
        name = CLASS_TO_NAME[curcls]
        for i in range(min_overlaps.shape[0]):
            levels = "{:.2f}, {:.2f}, {:.2f}:".format(*min_overlaps[i, :, j])
            for title, tables in ((f"{name} AP@", ap), (f"{name} AP_R40@", ap40)):
                result += title + levels + "\n"
                result += row("bbox", tables["bbox"], j, i, 4) + row("bev ", tables["bev"], j, i, 4) + row("3d  ", tables["3d"], j, i, 4)
                if compute_aos:
                    result += row("aos ", tables["aos"], j, i, 2)
            if i == 0:
                for key, label in (("aos", "aos"), ("3d", "3d"), ("bev", "bev"), ("bbox", "image")):
                    if key == "aos" and not compute_aos:
                        continue
                    for d, diff in enumerate(("easy", "moderate", "hard")):
                        ret_dict[f"{name}_{label}/{diff}_R40"] = ap40[key][j, d, 0]
    return result, ret_dict
