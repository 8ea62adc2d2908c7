#!/usr/bin/env python
"""Dynamic voxelisation on Waymo-shape clouds (2 x 180 k points, 0.32 m pillars, 468 x 468): per-kernel time from HIP events,
priced against HBM bytes (these kernels move bytes and do no FLOPs), the whole DynPillarVFE forward + backward, and the same
module composed from torch ops on the GPU (torch.unique + index_add_ / scatter_reduce, the module's CPU restatement run on the
device) for comparison.

    python -m toda_amd.tools.bench_dyn_vfe [--iters 20] [--warmup 5]

Prints one JSON line.  Byte counts are the minimum traffic of each kernel (every input read once, every output written once);
the index build includes its one host read of the voxel count."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from toda_amd import ops  # noqa: E402
from toda_amd.pcdet.config import AttrDict  # noqa: E402
from toda_amd.pcdet.models.backbones_3d.vfe import __all__ as VFES  # noqa: E402

PC_RANGE, VOXEL = [-74.88, -74.88, -2.0, 74.88, 74.88, 4.0], [0.32, 0.32, 6.0]
HBM_GBS = 8000.0      # MI355X peak HBM bandwidth


def clouds(n, bs, seed=0):
    rng = np.random.default_rng(seed)
    parts = []
    for b in range(bs):
        p = np.zeros((n, 6), np.float32)
        p[:, 0] = b
        r = np.abs(rng.normal(0, 25, n)) + 2.0
        a = rng.uniform(-np.pi, np.pi, n)
        p[:, 1], p[:, 2], p[:, 3] = r * np.cos(a), r * np.sin(a), rng.uniform(-2, 4, n)
        p[:, 4:] = rng.uniform(0, 1, (n, 2))
        parts.append(p)
    return torch.from_numpy(np.concatenate(parts)).cuda()


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=180000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    pts = clouds(args.points, args.batch)
    n, w = pts.shape
    cfg = AttrDict({"NAME": "DynPillarVFE", "WITH_DISTANCE": False, "USE_ABSLOTE_XYZ": True, "USE_NORM": True, "NUM_FILTERS": [64, 64]})
    torch.manual_seed(0)
    vfe = VFES["DynPillarVFE"](model_cfg=cfg, num_point_features=w - 1, voxel_size=VOXEL, grid_size=ops.grid_size_xyz(PC_RANGE, VOXEL),
                               point_cloud_range=PC_RANGE).cuda().train()
    idx = ops.dyn_voxel_index(pts, PC_RANGE, VOXEL, args.batch, True)
    k, m, c = idx.K, idx.M, 32
    nwords = (args.batch * 468 * 468 + 31) // 32
    mean = ops.dyn_points_mean(pts, idx, 1, 3)
    offs = [vfe.x_offset, vfe.y_offset, vfe.z_offset]
    deco = ops.dyn_pillar_decorate(pts, idx, mean, VOXEL, offs, True, False)
    f = deco.shape[1]
    x = torch.randn((k, c), device="cuda")
    xmax, arg = ops.dyn_seg_max_raw(x, idx)
    gmax = torch.randn((m, c), device="cuda")
    g2 = torch.randn((k, 2 * c), device="cuda")
    lib = ops.L.load()
    gx = torch.empty((k, c), device="cuda")
    passes = max(1, (max(m - 1, 1).bit_length() + 7) // 8)
    kern = {
        # points read twice, bitmap cleared / marked / scanned / read, keep flags and positions, rows / inv / key per kept point,
        # the radix passes (key + value read and written per pass), segment heads
        "index": (lambda: ops.dyn_voxel_index(pts, PC_RANGE, VOXEL, args.batch, True),
                  2 * n * w * 4 + 5 * nwords * 8 + n * (4 * 3 + 1) + k * (4 * 4 + 8) + passes * k * 16 + k * 12 + m * 24),
        "mean": (lambda: ops.dyn_points_mean(pts, idx, 1, 3), k * (4 + 4 + 12) + m * (8 + 12)),
        "decorate": (lambda: ops.dyn_pillar_decorate(pts, idx, mean, VOXEL, offs, True, False), k * (w * 4 + 8 + 8 + 12 + f * 4)),
        "max_fwd": (lambda: ops.dyn_seg_max_raw(x, idx), k * c * 4 + k * 4 + m * (8 + c * 8)),
        "max_bwd": (lambda: ops.L.check(lib.toda_dynvox_seg_max_bwd(ops.L.ptr(gmax), ops.L.ptr(arg), m, c, k, ops.L.ptr(gx), ops.L.stream()), "bwd"),
                    k * c * 4 + m * c * 8),
        "gather_concat_fwd": (lambda: ops.dyn_gather_concat(x, xmax, idx), k * c * 4 * 2 + k * 4 + k * 2 * c * 4),
        "gather_concat_bwd": (lambda: ops.dyn_seg_sum(g2, idx, col0=c, ncol=c), k * c * 4 + k * 4 + m * (8 + c * 4)),
    }
    res = {"points": n, "batch": args.batch, "kept": k, "pillars": m, "kernels": {}}
    for name, (fn, nbytes) in kern.items():
        us = timed(fn, args.iters, args.warmup)
        gbs = nbytes / (us * 1e-6) / 1e9
        res["kernels"][name] = {"us": round(us, 1), "MB": round(nbytes / 1e6, 2), "GB_s": round(gbs, 1), "hbm_pct": round(100 * gbs / HBM_GBS, 1)}

    def hip_step():
        out = vfe({"points": pts, "batch_size": args.batch})["pillar_features"]
        out.sum().backward()

    def torch_step():
        out = vfe._forward_torch({"points": pts, "batch_size": args.batch})["pillar_features"]
        out.sum().backward()

    res["vfe_fwd_bwd_us"] = round(timed(hip_step, args.iters, args.warmup), 1)
    res["torch_composition_fwd_bwd_us"] = round(timed(torch_step, args.iters, args.warmup), 1)
    res["speedup_vs_torch"] = round(res["torch_composition_fwd_bwd_us"] / res["vfe_fwd_bwd_us"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
