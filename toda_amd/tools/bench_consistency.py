#!/usr/bin/env python
"""Timing of the consistency term of the stage-2 step (get_consistency_loss: ops.consistency_match, csrc/consistency.hip) against
the torch composition it replaces on device tensors (_consistency_loss_torch):
    python -m toda_amd.tools.bench_consistency [--out profiles/consistency_bench.json]
Three shapes, boxes as the filters of the consistency step hand them over (padded lists with masks):
  * c5cl           batch 2, Na = No = 500, all selected: one CenterHead with K = 500, the shape of bench.py --workload c5cl;
  * six_heads      batch 2, Na = No = 3000, all selected: the six-head nuScenes CenterPoint;
  * second_iou     batch 4, Na = No = 500, about 40 % selected: SECOND-IoU's upper bound after the NMS.
Per shape, on the same device inputs, the two routes alternating (kernel, torch, kernel, torch, ...) in rounds of `--iters` calls
timed with device events; the median round of each route is reported with its spread, next to the peak bytes allocated above
the inputs and both routes' results.  Needs a GPU: there is no CPU fallback.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from toda_amd.pcdet import models as M  # noqa: E402

SHAPES = {"c5cl": {"batch": 2, "n": 500, "selected": 1.0},
          "six_heads": {"batch": 2, "n": 3000, "selected": 1.0},
          "second_iou": {"batch": 4, "n": 500, "selected": 0.4}}


def make_lists(shape, seed=0):
    """(adv, org) padded lists: org boxes scattered over a 108 m square, 60 % of the adv boxes within 0.3 m of an org box."""
    rng = np.random.default_rng(seed)
    adv, org = [], []
    for _ in range(shape["batch"]):
        n = shape["n"]
        o = np.concatenate([rng.uniform(-54, 54, (n, 2)), rng.uniform(-2, 0, (n, 1)), rng.uniform(0.5, 5, (n, 3)), rng.uniform(-3, 3, (n, 1))], 1)
        a = np.concatenate([rng.uniform(-54, 54, (n, 2)), rng.uniform(-2, 0, (n, 1)), rng.uniform(0.5, 5, (n, 3)), rng.uniform(-3, 3, (n, 1))], 1)
        near = rng.permutation(n)[:n * 6 // 10]
        a[near, :3] = o[rng.permutation(n)[:len(near)], :3] + rng.uniform(-0.3, 0.3, (len(near), 3))
        for boxes, out in ((a, adv), (o, org)):
            out.append({"pred_boxes": torch.from_numpy(boxes.astype(np.float32)).cuda(), "mask": torch.from_numpy(rng.random(n) < shape["selected"]).cuda()})
    return adv, org


def round_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def bench_shape(shape, iters, rounds):
    adv, org = make_lists(shape)
    routes = {"kernel": lambda: M.get_consistency_loss(adv, org), "torch": lambda: M._consistency_loss_torch(adv, org)}
    res = {"batch": shape["batch"], "na": shape["n"], "no": shape["n"], "selected": float(np.mean([float(d["mask"].float().mean()) for d in adv + org]))}
    for name, fn in routes.items():
        for _ in range(5):
            fn()
        peak, out = peak_bytes(fn)
        res[f"{name}_peak_bytes"], res[f"{name}_centre"], res[f"{name}_size"] = int(peak), float(out[0]), float(out[1])
    times = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():                       # alternating: kernel, torch, kernel, torch, ...
            times[name].append(round_ms(fn, iters))
    for name, t in times.items():
        res[f"{name}_ms"] = round(float(np.median(t)), 5)
        res[f"{name}_ms_min_max"] = [round(float(min(t)), 5), round(float(max(t)), 5)]
    res["torch_over_kernel"] = round(res["torch_ms"] / res["kernel_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_bench.json"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency needs a GPU: the kernel route has no CPU fallback")
    res = {"bench": "consistency", "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds}
    for name, shape in SHAPES.items():
        res[name] = bench_shape(shape, args.iters, args.rounds)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
