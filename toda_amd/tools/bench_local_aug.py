#!/usr/bin/env python
"""Timing of the per-object and pyramid augmentations on device clouds:
    python -m toda_amd.tools.bench_local_aug [--out profiles/local_aug_bench.json]
At a Waymo-shape sample (180 k points, 60 boxes) and a KITTI-shape one (20 k points, 15 boxes) every box-loop augmentation
is timed on the fused road (host draws + one toda_points_box_steps launch, wall time with a final sync) against the
straightforward device composition of the reference's loop: per box one points_in_boxes mode-1 launch plus a masked torch
update.  The pyramid family has no such composition (the reference asks scipy per pyramid) and is timed against this
project's numpy road on the host copy of the cloud.  The step kernel alone is also timed with HIP events; its rate is
given at 8 n c algorithmic bytes (the table read once and written once) as a fraction of the 8 TB/s HBM roof.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from toda_amd import ops  # noqa: E402
from toda_amd.pcdet.datasets.augmentor import augmentor_utils as U  # noqa: E402
from toda_amd.pcdet.datasets.synthetic import synth_cloud  # noqa: E402

HBM_ROOF = 8e12


def wall(fn, iters):
    """Mean wall time in ms of fn(), seeded alike every time, device idle at both ends."""
    for _ in range(3):
        np.random.seed(0)
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        np.random.seed(0)
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def events(fn, iters=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def composed(kind, boxes, points, arg):
    """The reference's loop with its numpy passes replaced one for one by device calls."""
    boxes = boxes.copy()
    for idx in range(len(boxes)):
        u = np.random.uniform(arg[0], arg[1])
        box = torch.from_numpy(boxes[idx:idx + 1, :7]).cuda()
        mask = ops.points_in_boxes(points, box, mode=1).bool()
        centre = box[0, :3]
        if kind == "translation":
            points[:, 0] = torch.where(mask, points[:, 0] + np.float32(u), points[:, 0])
            boxes[idx, 0] += u
        elif kind == "scaling":
            points[:, :3] = torch.where(mask[:, None], (points[:, :3] - centre) * np.float32(u) + centre, points[:, :3])
            boxes[idx, 3:6] *= u
        elif kind == "rotation":
            cs, sn = float(np.cos(np.float32(u))), float(np.sin(np.float32(u)))
            rot = torch.tensor([[cs, sn, 0], [-sn, cs, 0], [0, 0, 1]], dtype=torch.float32, device=points.device)
            points[:, :3] = torch.where(mask[:, None], (points[:, :3] - centre) @ rot + centre, points[:, :3])
            boxes[idx, 6] += u
        else:
            thr = (boxes[idx, 2] + boxes[idx, 5] / 2) - u * boxes[idx, 5]
            points = points[~(mask & (points[:, 2] >= float(thr)))]
    return points


def bench_shape(label, kind, n_boxes, iters):
    pts, bx, _ = synth_cloud(kind, 1, n_boxes=n_boxes)
    pts, bx = np.ascontiguousarray(pts.astype(np.float32)), bx[:, :7].astype(np.float32)
    p = torch.from_numpy(pts).cuda()
    n, c = p.shape
    rows = {}
    fused = {
        "random_local_translation_x": (lambda: U.random_local_translation_along_x(bx.copy(), p.clone(), [0.95, 1.05]), "translation", [0.95, 1.05]),
        "local_rotation": (lambda: U.local_rotation(bx.copy(), p.clone(), [-0.157, 0.157]), "rotation", [-0.157, 0.157]),
        "local_scaling": (lambda: U.local_scaling(bx.copy(), p.clone(), [0.95, 1.05]), "scaling", [0.95, 1.05]),
        "local_frustum_dropout_top": (lambda: U.local_frustum_dropout_top(bx.copy(), p.clone(), [0, 0.2]), "dropout", [0, 0.2]),
    }
    for name, (fn, what, arg) in fused.items():
        t_fused = wall(fn, iters)
        t_comp = wall(lambda: composed(what, bx, p.clone(), arg), iters)
        rows[name] = {"fused_ms": round(t_fused, 4), "composed_ms": round(t_comp, 4), "ratio": round(t_comp / t_fused, 2)}
    rows["random_world_translation_xyz"] = {"fused_ms": round(wall(lambda: U._run_steps(p, np.concatenate(
        [U.world_translation_steps(bx.copy(), 0.2, a) for a in "xyz"])), iters), 4)}
    rows["global_frustum_dropout_top"] = {"fused_ms": round(wall(lambda: U.global_frustum_dropout_top(bx.copy(), p, [0, 0.2]), iters), 4)}
    host_iters = max(1, iters // 10)
    for name, fn in [("local_pyramid_dropout", lambda q: U.local_pyramid_dropout(bx.copy(), q, 0.25)),
                     ("local_pyramid_sparsify", lambda q: U.local_pyramid_sparsify(bx.copy(), q, 0.05, 50)),
                     ("local_pyramid_swap", lambda q: U.local_pyramid_swap(bx.copy(), q, 0.1, 50))]:
        if c != 4 and name.endswith("swap"):
            continue
        t_dev = wall(lambda: fn(p.clone()), iters)
        t_host = wall(lambda: fn(pts.copy()), host_iters)
        rows[name] = {"fused_ms": round(t_dev, 4), "numpy_road_ms": round(t_host, 4), "ratio": round(t_host / t_dev, 2)}
    np.random.seed(0)
    steps = torch.from_numpy(U.local_scaling_steps(bx.copy(), [0.95, 1.05])).cuda()
    out = torch.empty_like(p)
    ms = events(lambda: ops.points_box_steps(p, steps, out=out))
    rate = 8.0 * n * c / (ms * 1e-3)
    pyr = torch.from_numpy(U.get_pyramids(bx).reshape(-1, 15).astype(np.float64)).cuda()
    ms_pyr = events(lambda: ops.points_in_pyramids(p, pyr))
    ms_rng = events(lambda: ops.points_column_range(p, 2))
    return {"shape": label, "points": n, "columns": c, "boxes": len(bx), "augmentations": rows,
            "box_steps_kernel": {"steps": int(steps.shape[0]), "us": round(ms * 1e3, 2), "algorithmic_GBps": round(rate / 1e9, 1),
                                 "fraction_of_8TBps_roof": round(rate / HBM_ROOF, 4)},
            "in_pyramids_kernel": {"pyramids": int(pyr.shape[0]), "us_with_zeroing": round(ms_pyr * 1e3, 2)},
            "column_range_kernel": {"us": round(ms_rng * 1e3, 2)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_aug_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=["waymo", "kitti"], default=None)
    args = ap.parse_args()
    shapes = [("waymo 180k x 60", "waymo", 60), ("kitti 20k x 15", "kitti", 15)]
    res = {"bench": "local_aug", "device": torch.cuda.get_device_name(0),
           "shapes": [bench_shape(lb, kind, k, args.iters) for lb, kind, k in shapes if args.only in (None, kind)]}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
