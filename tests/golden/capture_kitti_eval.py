#!/usr/bin/env python
"""Capture the KITTI-evaluator fixtures from the REFERENCE's own Python (build container only).

    python tests/golden/capture_kitti_eval.py

writes tests/golden/kitti_eval_overlaps.npz (box pairs for metrics 0, 1, 2 and criteria -1, 0, 1, 2), kitti_eval_match.npz
(40 frames of camera-frame annotations with eval_class's precision / recall / orientation and its tp / fp / fn /
similarity table per (class, difficulty, level) for the three metrics, and get_official_eval_result's text and numbers), kitti_eval_ties.npz (hand-built frames with duplicated detections: identical
overlaps, and identical scores) and kitti_eval_lidar.npz (LiDAR-frame annotations through
transform_annotations_to_kitti_format, and their result).

The reference's rotate_iou.py and eval.py are loaded by path.  numba is not installed: numba.jit and numba.cuda.jit become
pass-through decorators, cuda.local.array becomes np.zeros, numba.float32 np.float32, and rotate_iou_gpu_eval becomes a double
loop over the reference's own devRotateIoUEval in the kernel's operand order (query first).  get_split_parts is made to
return one frame per part: the parts only bound the cross product whose off-diagonal blocks the reference throws away, and
in pure Python the full product would take hours.  Only inputs and outputs are stored.

Screening is a condition, not a mask: a seed is rejected and the next one drawn unless no reference overlap lies within
1e-3 of a min_overlap level (0.25, 0.5, 0.7) and no two detections of a frame share a score;
tests/test_kitti_eval_host.py recomputes both from the committed inputs.  The ties fixture is exempt from the second by design.
"""
import copy
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import kitti_eval_cases as cases  # noqa: E402

REF = os.environ.get("TODA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
A = "refkitti"


def _jit(*a, **k):
    if len(a) == 1 and callable(a[0]) and not k:
        return a[0]
    return lambda fn: fn


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def setup():
    numba = types.ModuleType("numba")
    cuda = types.ModuleType("numba.cuda")
    numba.jit, numba.float32, numba.cuda = _jit, np.float32, cuda
    cuda.jit = _jit
    cuda.local = types.SimpleNamespace(array=lambda shape, dtype: np.zeros(shape, dtype))
    sys.modules["numba"], sys.modules["numba.cuda"] = numba, cuda
    for pkg in (A, f"{A}.utils", f"{A}.datasets", f"{A}.datasets.kitti", f"{A}.datasets.kitti.kitti_object_eval_python"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    sys.modules[f"{A}.utils.box_utils"] = types.ModuleType(f"{A}.utils.box_utils")       # only the fake-lidar branch reads it
    sys.modules[f"{A}.utils"].box_utils = sys.modules[f"{A}.utils.box_utils"]
    base = "pcdet/datasets/kitti"
    R = _load(f"{A}.datasets.kitti.kitti_object_eval_python.rotate_iou", f"{base}/kitti_object_eval_python/rotate_iou.py")
    E = _load(f"{A}.datasets.kitti.kitti_object_eval_python.eval", f"{base}/kitti_object_eval_python/eval.py")
    K = _load(f"{A}.datasets.kitti.kitti_utils", f"{base}/kitti_utils.py")
    memo = {}

    def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
        b32, q32 = boxes.astype(np.float32), query_boxes.astype(np.float32)
        key = (b32.tobytes(), q32.tobytes(), criterion)
        if key not in memo:
            iou = np.zeros((len(b32), len(q32)), np.float32)
            with np.errstate(all="ignore"):
                for n in range(len(b32)):
                    for k in range(len(q32)):
                        iou[n, k] = R.devRotateIoUEval(q32[k], b32[n], criterion)
            memo[key] = iou
        return memo[key].astype(boxes.dtype)

    E.rotate_iou_gpu_eval = rotate_iou_gpu_eval
    E.get_split_parts = lambda num, num_part: [1] * num
    return R, E, K


def ref_blocks(E, gts, dts):
    """The reference's per-frame overlaps [n_det, n_gt] for the three metrics."""
    return {m: E.calculate_iou_partly(dts, gts, m, 100)[0] for m in (0, 1, 2)}


def ref_results(E, gts, dts, classes):
    out = {}
    names = {v: k for k, v in enumerate(cases.KITTI_CLASSES)}
    ids = [names[c] for c in classes]
    ov7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7]] * 3)
    ov5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])
    min_overlaps = np.stack([ov7, ov5], 0)[:, :, ids]
    with np.errstate(all="ignore"):
        for m in (0, 1, 2):
            # the reference's own pr[T, 4] = (tp, fp, fn, similarity) per (class, difficulty, level), in loop order: every
            # call of fused_compute_statistics adds one part's frames into the array it is handed
            tables, fused = [], E.fused_compute_statistics

            def spy(overlaps, pr, *rest, **kw):
                if not any(pr is t for t in tables):
                    tables.append(pr)
                return fused(overlaps, pr, *rest, **kw)

            E.fused_compute_statistics = spy
            try:
                ret = E.eval_class(gts, dts, ids, [0, 1, 2], m, min_overlaps, compute_aos=(m == 0))
            finally:
                E.fused_compute_statistics = fused
            for k in ("precision", "recall", "orientation"):
                out[f"{k}_{m}"] = ret[k]
            out[f"counts_{m}"] = np.concatenate(tables + [np.zeros((0, 4))], 0)
            out[f"counts_len_{m}"] = np.array([len(t) for t in tables], np.int64)
        text, res = E.get_official_eval_result(gts, dts, classes)
    out["result_str"] = np.array(text)
    out["ret_keys"] = np.array(sorted(res), dtype="<U64")
    out["ret_vals"] = np.array([res[k] for k in sorted(res)], np.float64)
    out["classes"] = np.array(classes, dtype="<U16")
    return out


def cap_overlaps(R, E):
    rng = np.random.default_rng(20261017)
    B, Q = [], []          # per frame: (box3d [n, 7], bbox [n, 4])

    def frame(b3, bb, q3, qb):
        B.append((np.asarray(b3, np.float64).reshape(-1, 7), np.asarray(bb, np.float64).reshape(-1, 4)))
        Q.append((np.asarray(q3, np.float64).reshape(-1, 7), np.asarray(qb, np.float64).reshape(-1, 4)))

    base3, baseb = [2.0, 1.6, 20.0, 4.0, 1.5, 1.8, 0.3], [100.0, 100.0, 200.0, 180.0]
    # The identical pair is axis-parallel.  For bit-identical rectangles every corner lies exactly on the other boundary, and
    # the reference's inside test then hangs on the sign of dot products that are zero in exact arithmetic: at angle 0 they
    # are zero in fp32 too and it returns IoU 1; at a general angle rounding decides and it returns 0, 1/3 or 1 (IoU 0.0 for
    # base3 against itself).  Those values are noise, not a rule, so they are no fixture; the evaluator returns 1 there
    # (tests/test_gpu_kitti_eval.py::test_a_rotated_box_against_itself_has_iou_one).
    flat3 = [2.0, 1.6, 20.0, 4.0, 1.5, 1.8, 0.0]
    special = [
        (flat3, baseb, flat3, baseb),                                                                  # identical
        (base3, baseb, [2.0, 1.6, 20.0, 2.0, 1.0, 0.9, 0.3], [120.0, 110.0, 180.0, 170.0]),             # containment
        ([0.0, 1.6, 10.0, 4.0, 1.5, 2.0, 0.0], baseb, [4.0, 1.6, 10.0, 4.0, 1.5, 2.0, 0.0], [200.0, 100.0, 300.0, 180.0]),  # touching
        (base3, baseb, [40.0, 1.6, 60.0, 4.0, 1.5, 1.8, 1.0], [400.0, 300.0, 450.0, 350.0]),            # disjoint
        (base3, baseb, [2.0, 1.6, 20.0, 4.0, 1.5, 1.8, 0.3 + np.pi / 2], [150.0, 60.0, 250.0, 140.0]),   # 90 degrees
        (base3, baseb, [2.1, 1.6, 20.2, 4.0, 1.5, 1.8, 0.301], [101.0, 99.0, 203.0, 181.0]),            # near parallel
        (base3, baseb, [2.1, 4.0, 20.2, 4.0, 1.5, 1.8, 0.301], [100.0, 180.0, 200.0, 260.0]),           # no height overlap
        ([0.0, 1.6, 10.0, 4.0, 1.5, 2.0, 0.0], baseb, [0.0, 1.0, 10.0, 2.0, 1.5, 4.0, np.pi / 2], baseb),  # same rectangle, turned
    ]
    for b3, bb, q3, qb in special:
        frame([b3], [bb], [q3], [qb])
    for _ in range(40):
        n, k = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        q3 = np.stack([rng.uniform(-5, 5, k), rng.uniform(1.2, 2.2, k), rng.uniform(10, 20, k), rng.uniform(1, 5, k),
                       rng.uniform(1, 2, k), rng.uniform(0.5, 2.5, k), rng.uniform(-np.pi, np.pi, k)], 1)
        pick = rng.integers(0, k, n)
        b3 = q3[pick] + rng.normal(0, 1, (n, 7)) * [0.6, 0.2, 0.6, 0.3, 0.1, 0.2, 0.3]
        qb = np.stack([rng.uniform(0, 600, k), rng.uniform(100, 200, k)], 1)
        qb = np.concatenate([qb, qb + rng.uniform(20, 150, (k, 2))], 1)
        bb = qb[pick] + rng.normal(0, 12, (n, 4))
        frame(b3, bb, q3, qb)
    out = {"box_off": np.concatenate([[0], np.cumsum([len(b[0]) for b in B])]).astype(np.int64),
           "query_off": np.concatenate([[0], np.cumsum([len(q[0]) for q in Q])]).astype(np.int64),
           "box3d": np.concatenate([b[0] for b in B]), "bbox": np.concatenate([b[1] for b in B]),
           "query3d": np.concatenate([q[0] for q in Q]), "query_bbox": np.concatenate([q[1] for q in Q])}
    with np.errstate(all="ignore"):
        for crit in (-1, 0, 1, 2):
            img, bev, d3 = [], [], []
            for (b3, bb), (q3, qb) in zip(B, Q):
                img.append(E.image_box_overlap(bb, qb, crit).reshape(-1))
                bev.append(E.bev_box_overlap(b3[:, [0, 2, 3, 5, 6]], q3[:, [0, 2, 3, 5, 6]], crit).reshape(-1))
                d3.append(E.d3_box_overlap(b3, q3, crit).reshape(-1))
            for m, parts in enumerate((img, bev, d3)):
                out[f"expect_m{m}_c{crit}"] = np.concatenate(parts).astype(np.float64)
    np.savez_compressed(os.path.join(OUT, "kitti_eval_overlaps.npz"), **out)
    print("overlaps:", len(B), "frames,", len(out["expect_m1_c-1"]), "pairs")


def screened(E, make, first_seed):
    seed = first_seed
    while True:
        gts, dts = make(seed)
        blocks = ref_blocks(E, gts, dts)
        gap, shared = cases.screen([b for m in (0, 1, 2) for b in blocks[m]], dts)
        print(f"seed {seed}: nearest overlap to a level {gap:.2e}, frames with shared scores {shared}")
        if gap >= 1e-3 and shared == 0:
            return seed, gts, dts, blocks
        seed += 1


def save_set(path, E, gts, dts, blocks, classes, extra=None):
    out = dict(extra or {})
    out.update(cases.pack(gts, "gt"))
    out.update(cases.pack(dts, "dt"))
    for m in (0, 1, 2):
        out[f"overlaps_{m}"] = np.concatenate([np.asarray(b, np.float64).reshape(-1) for b in blocks[m]] + [np.zeros(0)])
    out.update(ref_results(E, gts, dts, classes))
    np.savez_compressed(path, **out)
    print(os.path.basename(path), "\n" + str(out["result_str"])[:400])


def cap_match(E):
    seed, gts, dts, blocks = screened(E, lambda s: cases.kitti_frames(s, 40), 100)
    save_set(os.path.join(OUT, "kitti_eval_match.npz"), E, gts, dts, blocks, ["Car", "Pedestrian", "Cyclist"], {"seed": np.array(seed)})


def cap_ties(E):
    """Frame 0: two detections with the same box on one Car (identical overlaps, scores 0.6 < 0.9) next to a third, better
    aligned one on a second Car.  Frame 1: two different boxes on one Car sharing the score 0.8.  Frames 2-5: ordinary."""
    seed, gts, dts, _ = screened(E, lambda s: cases.kitti_frames(s, 6, classes=("Car", "Pedestrian"), dontcare=False), 300)
    car = {"name": "Car", "location": [1.0, 1.6, 15.0], "dimensions": [4.0, 1.5, 1.8], "rotation_y": 0.2, "alpha": 0.1,
           "bbox": [300.0, 150.0, 420.0, 230.0], "occluded": 0.0, "truncated": 0.0}
    car2 = dict(car, location=[-8.0, 1.6, 25.0], bbox=[100.0, 160.0, 180.0, 215.0])

    def det(src, score, shift=0.0):
        return dict(src, location=[src["location"][0] + shift, src["location"][1], src["location"][2]], score=score,
                    bbox=[src["bbox"][0] + 10 * shift, src["bbox"][1], src["bbox"][2] + 10 * shift, src["bbox"][3]])

    gts[0], dts[0] = cases._anno([car, car2], False), cases._anno([det(car, 0.6, 0.2), det(car, 0.9, 0.2), det(car2, 0.7, 0.1)], True)
    gts[1], dts[1] = cases._anno([car], False), cases._anno([det(car, 0.8, 0.3), det(car, 0.8, 0.1), det(car2, 0.3)], True)
    blocks = ref_blocks(E, gts, dts)
    gap, _ = cases.screen([b for m in (0, 1, 2) for b in blocks[m]], dts)
    assert gap >= 1e-3, gap
    save_set(os.path.join(OUT, "kitti_eval_ties.npz"), E, gts, dts, blocks, ["Car", "Pedestrian"], {"seed": np.array(seed)})


def cap_lidar(E, K):
    mapping = {"car": "Car", "truck": "Truck", "pedestrian": "Pedestrian", "barrier": "Person_sitting"}

    def make(s):
        infos, dets = cases.lidar_frames(s)
        g, d = copy.deepcopy(infos), copy.deepcopy(dets)
        K.transform_annotations_to_kitti_format(d, map_name_to_kitti=mapping)
        K.transform_annotations_to_kitti_format(g, map_name_to_kitti=mapping)
        return g, d

    seed, gts, dts, blocks = screened(E, make, 500)
    for a in gts:
        a["alpha"] = np.asarray(a["alpha"], np.float64)
    save_set(os.path.join(OUT, "kitti_eval_lidar.npz"), E, gts, dts, blocks, ["Car", "Truck", "Pedestrian"],
             {"seed": np.array(seed), "map_keys": np.array(sorted(mapping), dtype="<U16"),
              "map_vals": np.array([mapping[k] for k in sorted(mapping)], dtype="<U16")})


if __name__ == "__main__":
    R, E, K = setup()
    cap_overlaps(R, E)
    cap_match(E)
    cap_ties(E)
    cap_lidar(E, K)
