"""PV-RCNN's stack-layer kernels at the Waymo shapes, one JSON line:
  - FPS (2 samples x 180 k points, 4096 keypoints; KITTI: 2 x 20 k, 2048): workgroup groups vs the one-workgroup port of the
    reference's kernel;
  - the ball query, the SA layer (query + pool, forward + backward) and the BEV interpolation at the VSA (x_conv3, raw_points)
    and RoI-grid shapes, each against the torch composition of the reference doing the same work (dense distances, grouping into
    [M, C, nsample] tensors), with algorithmic bytes and the HBM-roof time;
  - PV-RCNN training samples/s of pv_rcnn_centerhead_waymo.yaml.
python -m toda_amd.tools.bench_pv_rcnn [--reps 5] [--no-train]"""
import argparse
import copy
import json
import time

import numpy as np
import torch
import torch.nn.functional as F

from toda_amd import ops
from toda_amd.pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils
from toda_amd.pcdet.ops.pointnet2.pointnet2_stack.pointnet2_modules import StackSAModuleMSG

DEV = torch.device("cuda", 0)
HBM_TBPS = 8.0


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def cloud(n, seed, extent):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand((n, 3), generator=g) - 0.5) * torch.tensor(extent)).float().to(DEV)


def bench_fps(reps):
    out = {}
    for name, n, npoint in (("waymo", 180000, 4096), ("kitti", 20000, 2048), ("n8k", 8192, 2048), ("n4k", 4096, 1024)):
        xyz = torch.cat([cloud(n, 1, (150.0, 150.0, 6.0)), cloud(n, 2, (150.0, 150.0, 6.0))])
        one = timed(lambda: ops.farthest_point_sample(xyz, [n, n], npoint, mode=1), max(1, reps // 2))
        multi = timed(lambda: ops.farthest_point_sample(xyz, [n, n], npoint, mode=2), reps)
        same = torch.equal(ops.farthest_point_sample(xyz, [n, n], npoint, mode=1), ops.farthest_point_sample(xyz, [n, n], npoint, mode=2))
        ops.L.check(ops.L.load().toda_device_fault(), "toda_device_fault")
        out[f"fps_{name}_ms"] = {"one_workgroup": round(one, 3), "workgroup_groups": round(multi, 3), "speedup": round(one / multi, 2),
                                 "identical": same}
    return out


def ball_query_torch(radii, nsamples, xyz, counts, new_xyz, m_counts):
    """The reference's ball query as a torch composition (dense d2 per query chunk, first nsample hits in index order)."""
    xs = [0] + np.cumsum(counts).tolist()
    qs = [0] + np.cumsum(m_counts).tolist()
    out = [(torch.zeros((new_xyz.shape[0], ns), dtype=torch.int32, device=DEV), torch.zeros((new_xyz.shape[0],), dtype=torch.bool, device=DEV))
           for ns in nsamples]
    for b in range(len(counts)):
        pts = xyz[xs[b]:xs[b + 1]]
        for q0 in range(qs[b], qs[b + 1], 1024):
            q1 = min(q0 + 1024, qs[b + 1])
            c = new_xyz[q0:q1]
            d2 = (c[:, 0:1] - pts[None, :, 0]) ** 2 + (c[:, 1:2] - pts[None, :, 1]) ** 2 + (c[:, 2:3] - pts[None, :, 2]) ** 2
            for (idx, empty), r, ns in zip(out, radii, nsamples):
                hit = d2 < r * r
                pos = torch.cumsum(hit.int(), 1) - 1
                cnt = hit.sum(1)
                blk = (torch.argmax(hit.int(), 1) + xs[b]).unsqueeze(1).repeat(1, ns)
                rr, kk = (hit & (pos < ns)).nonzero(as_tuple=True)
                blk[rr, pos[rr, kk]] = kk + xs[b]
                blk[cnt == 0] = 0
                idx[q0:q1] = blk.int()
                empty[q0:q1] = cnt == 0
    return out


def sa_torch(mod, xyz, counts, new_xyz, m_counts, feats, tables):
    """The reference's composition: grouped [M, 3 + C, ns] tensors, Conv2d / BatchNorm2d / ReLU, max_pool2d."""
    outs = []
    for k, (idx, empty) in enumerate(tables):
        grouped = pointnet2_utils.QueryAndGroup.group(xyz, new_xyz, feats, idx, empty, True)
        y = mod.mlps[k](grouped.permute(1, 0, 2).unsqueeze(0))
        outs.append(F.max_pool2d(y, kernel_size=[1, y.size(3)]).squeeze(-1).squeeze(0).permute(1, 0))
    return torch.cat(outs, 1)


def bench_shape(name, n_per, m_per, c_in, radii, nsamples, mlps, reps):
    counts, m_counts = [n_per, n_per], [m_per, m_per]
    xyz = torch.cat([cloud(n_per, 3, (140.0, 140.0, 6.0)), cloud(n_per, 4, (140.0, 140.0, 6.0))])
    new_xyz = torch.cat([cloud(m_per, 5, (140.0, 140.0, 6.0)), cloud(m_per, 6, (140.0, 140.0, 6.0))])
    feats = torch.randn((xyz.shape[0], c_in), device=DEV)
    mod = StackSAModuleMSG(radii=radii, nsamples=nsamples, mlps=[[c_in] + list(m) for m in mlps]).to(DEV).train()
    ref = copy.deepcopy(mod)
    xs, ns_ = ops.batch_starts(counts, DEV), ops.batch_starts(m_counts, DEV)
    bq = timed(lambda: ops.ball_query_stack(radii, nsamples, xyz, xs, new_xyz, ns_), reps)
    bq_torch = timed(lambda: ball_query_torch(radii, nsamples, xyz, counts, new_xyz, m_counts), max(1, reps // 2))

    def ours():                     # query + pool, forward and backward
        f = feats.clone().requires_grad_(True)
        _, out = mod(xyz, counts, new_xyz, m_counts, f)
        out.sum().backward()

    def theirs():                   # the same work as the reference composes it
        f = feats.clone().requires_grad_(True)
        tables = ball_query_torch(radii, nsamples, xyz, counts, new_xyz, m_counts)
        sa_torch(ref, xyz, counts, new_xyz, m_counts, f, tables).sum().backward()

    t_ours, t_torch = timed(ours, reps), timed(theirs, max(1, reps // 2))
    m = 2 * m_per
    e = sum(m * ns for ns in nsamples)
    width = sum(ml[0] for ml in mlps)
    # algorithmic bytes of the pool: features read once per source row, the rows layout of every layer written + read fwd / bwd
    nbytes = xyz.shape[0] * c_in * 4 * 2 + e * width * 4 * 2 * 3 + e * 4 * 2
    return {f"{name}_ball_query_ms": {"hip": round(bq, 3), "torch": round(bq_torch, 3), "speedup": round(bq_torch / bq, 2)},
            f"{name}_sa_fwd_bwd_ms": {"hip": round(t_ours, 3), "torch": round(t_torch, 3), "speedup": round(t_torch / t_ours, 2),
                                      "algorithmic_mb": round(nbytes / 1e6, 1), "hbm_roof_ms": round(nbytes / (HBM_TBPS * 1e9), 3)}}


def bench_bev(reps):
    fmap = torch.randn((2, 256, 188, 188), device=DEV, requires_grad=True)
    k = 8192
    x = torch.rand((k,), device=DEV) * 188
    y = torch.rand((k,), device=DEV) * 188
    b = (torch.arange(k, device=DEV) >= k // 2).int()

    def ours():
        ops.bev_interpolate(fmap, x, y, b).sum().backward()

    def theirs():
        from toda_amd.pcdet.models.backbones_3d.pfe.voxel_set_abstraction import bilinear_interpolate_torch
        out = torch.cat([bilinear_interpolate_torch(fmap[i].permute(1, 2, 0), x[b == i], y[b == i]) for i in range(2)])
        out.sum().backward()

    t_ours, t_torch = timed(ours, reps), timed(theirs, reps)
    nbytes = fmap.numel() * 4 + k * 256 * 4 * 2 + k * 4 * 256 * 4
    return {"bev_interp_fwd_bwd_ms": {"hip": round(t_ours, 3), "torch": round(t_torch, 3), "speedup": round(t_torch / t_ours, 2),
                                      "algorithmic_mb": round(nbytes / 1e6, 1), "hbm_roof_ms": round(nbytes / (HBM_TBPS * 1e9), 3)}}


def bench_train(steps):
    from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import build_network, prepare_batch_on_gpu
    import os

    cfg = AttrDict()
    cfg_from_yaml_file(os.path.join(os.path.dirname(__file__), "cfgs", "models", "pv_rcnn_centerhead_waymo.yaml"), cfg)
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=True)
    torch.manual_seed(0)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    batches = [ds.collate_batch([ds[2 * i], ds[2 * i + 1]]) for i in range(steps + 1)]
    t0 = None
    for i, batch in enumerate(batches):
        if i == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        prepare_batch_on_gpu(batch, net)
        opt.zero_grad()
        ret, _, _ = net(batch)
        ret["loss"].backward()
        opt.step()
    torch.cuda.synchronize()
    return {"train_waymo_samples_per_s": round(2 * steps / (time.perf_counter() - t0), 2),
            "train_steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--train_steps", type=int, default=4)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"bench": "pv_rcnn"}
    res.update(bench_fps(args.reps))
    # VSA x_conv3 (~30 k rows per sample, 64 channels, radii 1.2 / 2.4, nsample 16 / 32), VSA raw points (180 k, 2 features),
    # RoI grid (4096 keypoints per sample, 90 channels, 128 x 216 grid points per sample, radii 0.8 / 1.6, nsample 16 / 16)
    res.update(bench_shape("vsa_x_conv3", 30000, 4096, 64, [1.2, 2.4], [16, 32], [[64, 64], [64, 64]], args.reps))
    res.update(bench_shape("vsa_raw_points", 180000, 4096, 2, [0.4, 0.8], [16, 16], [[16, 16], [16, 16]], args.reps))
    res.update(bench_shape("roi_grid", 4096, 128 * 216, 90, [0.8, 1.6], [16, 16], [[64, 64], [64, 64]], args.reps))
    res.update(bench_bev(args.reps))
    if not args.no_train:
        res.update(bench_train(args.train_steps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
