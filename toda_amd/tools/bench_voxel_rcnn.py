#!/usr/bin/env python
"""VoxelRCNNHead's pool at the Waymo training shape (4 samples x 128 rois x 6^3 grid points: M = 110 592, nsample 16, C = 64 per
level, x_conv2..4 at strides 2 / 4 / 8): per level the HIP voxel query, the fused pool forward (moments + kernel + inverse table)
and backward, timed with device events, beside the reference's torch composition on the same inputs ([M, C, nsample] tensors,
Conv2d + BatchNorm2d, max_pool2d) forward + backward; then training samples/s of voxel_rcnn_dyn_voxel_waymo.yaml.

    python -m toda_amd.tools.bench_voxel_rcnn [--iters 20] [--warmup 5] [--train-steps 6]

Prints one JSON line.  Bytes per level, two models: "unique" counts every byte the kernels must touch once (grid points,
coordinates and idx; relative positions from idx and the voxel centres; each neighbour row of the level once, out and arg;
for the backward g, arg, the table and d f) - a floor; "gathered" counts every (grid point, sample) row read of the forward
(M x nsample x C x 4 bytes), what the kernel issues before caches - an upper side.
"""
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
from toda_amd.pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import folded_position_map, pool_torch  # noqa: E402
from toda_amd.pcdet.utils.common_utils import get_voxel_centers  # noqa: E402

HBM_GBS = 8000.0
PC = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
VS = [0.1, 0.1, 0.15]
LEVELS = (("x_conv2", 2, 0.4, [21, 752, 752]), ("x_conv3", 4, 0.8, [11, 376, 376]), ("x_conv4", 8, 1.6, [5, 188, 188]))   # VoxelBackBone8x on [41, 1504, 1504]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out))


def level_inputs(stride, shape, batch, rois, seed):
    """Sites of one level (lattice `shape`): a 40 m x 40 m x full-height block per sample occupied at 30 %, and 6^3 grid points of
    rois around it."""
    g = torch.Generator().manual_seed(seed)
    span = int(40.0 / (VS[0] * stride))
    lo = shape[2] // 2 - span // 2
    coords = []
    for b in range(batch):
        z, y, x = torch.meshgrid(torch.arange(shape[0]), torch.arange(lo, lo + span), torch.arange(lo, lo + span), indexing="ij")
        keep = torch.rand(z.shape, generator=g) < 0.3
        coords.append(torch.stack([torch.full_like(z[keep], b), z[keep], y[keep], x[keep]], 1))
    coords = torch.cat(coords).int().cuda()
    xyz = get_voxel_centers(coords[:, 1:4], stride, VS, PC).contiguous()
    m = rois * 216
    new_xyz = (torch.rand((batch * m, 3), generator=g) * torch.tensor([36.0, 36.0, 4.0]) - torch.tensor([18.0, 18.0, 1.5])).float().cuda()
    bidx = torch.arange(batch).repeat_interleave(m).float().view(-1, 1).cuda()
    c = torch.cat([(new_xyz[:, j:j + 1] - PC[j]) // VS[j] for j in range(3)], 1) // stride
    nc = torch.cat([bidx, c], 1).int()[:, [0, 3, 2, 1]].contiguous()
    gi = ops.GridIndex.from_coords(coords, batch, shape)
    gi.rowof = None
    return coords, xyz, new_xyz, nc, gi


def bench_level(name, stride, radius, shape, iters, warmup):
    coords, xyz, new_xyz, nc, gi = level_inputs(stride, shape, 4, 128, stride)
    n, m, ns, c = coords.shape[0], new_xyz.shape[0], 16, 64
    f = torch.randn((n, c), device="cuda")
    pos = torch.nn.Sequential(torch.nn.Conv2d(3, c, 1, bias=False), torch.nn.BatchNorm2d(c)).cuda().train()
    rng = (3, 3, 2)
    t_query = timed(lambda: ops.voxel_query(new_xyz, nc, xyz, gi, radius, rng, ns), iters, warmup)
    idx, empty = ops.voxel_query(new_xyz, nc, xyz, gi, radius, rng, ns)
    fg = f.clone().requires_grad_(True)
    gout = torch.randn((m, c), device="cuda")
    state = {}

    def fwd():
        a, b = folded_position_map(pos, idx, empty, xyz, new_xyz)
        state["out"] = ops.voxel_neighbor_pool(fg, a, b, idx, empty, xyz, new_xyz)

    def bwd():
        fwd()
        state["out"].backward(gout)

    t_fwd = timed(fwd, iters, warmup)
    t_fb = timed(bwd, iters, warmup)

    def torch_fb():
        out = pool_torch(fg, idx, empty, xyz, new_xyz, pos)
        out.backward(gout)

    t_torch = timed(torch_fb, max(3, iters // 4), 2)
    hits = float((~empty).float().mean())
    b_query = m * (12 + 16 + 4 * ns + 1)
    b_fwd_unique = m * ns * 4 + m + n * 12 + m * 12 + n * c * 4 + m * c * 5
    b_fwd_gathered = b_fwd_unique - n * c * 4 + m * ns * c * 4
    b_bwd = m * c * (4 + 1) * 2 + m * ns * 8 + (n + 1) * 4 + n * c * 4
    us = lambda b: round(b / HBM_GBS / 1e3, 1)      # noqa: E731
    return {"level": name, "stride": stride, "shape": shape, "N": n, "M": m, "C": c, "nsample": ns, "nonempty_frac": round(hits, 3),
            "query_us": round(t_query, 1), "pool_fwd_us": round(t_fwd, 1), "pool_bwd_us": round(t_fb - t_fwd, 1),
            "torch_fwd_bwd_us": round(t_torch, 1), "fused_fwd_bwd_us": round(t_fb, 1),
            "bytes": {"query": b_query, "pool_fwd_unique": b_fwd_unique, "pool_fwd_gathered": b_fwd_gathered, "pool_bwd": b_bwd},
            "hbm_us": {"query": us(b_query), "pool_fwd_unique": us(b_fwd_unique), "pool_fwd_gathered": us(b_fwd_gathered),
                       "pool_bwd": us(b_bwd)}}


def train_rate(steps):
    from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import build_network, prepare_batch_on_gpu

    cfg = AttrDict()
    cfg_from_yaml_file(os.path.join(ROOT, "toda_amd", "tools", "cfgs", "models", "voxel_rcnn_dyn_voxel_waymo.yaml"), cfg)
    bs = cfg.OPTIMIZATION.BATCH_SIZE_PER_GPU
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=True)
    torch.manual_seed(0)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    batches = [ds.collate_batch([ds[(i * bs + k) % 16] for k in range(bs)]) for i in range(steps + 2)]
    t0 = None
    for i, batch in enumerate(batches):
        if i == 2:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        prepare_batch_on_gpu(batch, net)
        opt.zero_grad()
        ret, _, _ = net(batch)
        ret["loss"].backward()
        opt.step()
    torch.cuda.synchronize()
    return bs, steps * bs / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--train-steps", type=int, default=6)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    levels = [bench_level(name, s, r, shp, a.iters, a.warmup) for name, s, r, shp in LEVELS]
    bs, rate = train_rate(a.train_steps) if a.train_steps > 0 else (None, None)
    print(json.dumps({"bench": "voxel_rcnn", "device": torch.cuda.get_device_name(0), "levels": levels,
                      "train_config": "voxel_rcnn_dyn_voxel_waymo", "train_batch": bs,
                      "train_samples_per_s": None if rate is None else round(rate, 2)}))


if __name__ == "__main__":
    main()
