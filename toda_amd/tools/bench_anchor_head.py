#!/usr/bin/env python
"""The anchor target assigner at the two multi-head shapes - nuScenes (B 4, 128 x 128 map, 10 classes x 2 rotations = 327 680
anchors per sample, 40 gts per sample, 10 box codes) and KITTI (B 4, 200 x 176, 3 classes, 7 codes) - on its two routes in one
process: toda_anchor_assign (HIP, two launches and a workspace clear) beside the torch loop over batch x classes, with the
launch count of each route, the labels' agreement, and one multi-head PointPillars training step.

    python -m toda_amd.tools.bench_anchor_head [--iters 20] [--warmup 3] [--train-steps 5]

Prints one JSON line.  Roof of the HIP route: the target write, B x A x code x 4 bytes, against HBM bandwidth."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file  # noqa: E402
from toda_amd.pcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate  # noqa: E402
from toda_amd.pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner import AxisAlignedTargetAssigner  # noqa: E402
from toda_amd.pcdet.utils import box_coder_utils  # noqa: E402

HBM_GBS = 8000.0      # MI355X peak HBM bandwidth
CFGS = os.path.join(ROOT, "toda_amd", "tools", "cfgs", "models", "{}.yaml")
SHAPES = {   # name: (config whose anchor classes are used, grid (nx, ny) at the head's stride, coder, gts per sample, extra gt columns)
    "nuscenes": ("cbgs_pp_multihead_nuscenes", (128, 128), dict(code_size=9, encode_angle_by_sincos=True), 40, 2),
    "kitti": ("second_multihead_kitti", (176, 200), dict(code_size=7, encode_angle_by_sincos=False), 40, 0),
}


def load_cfg(name):
    cfg = AttrDict()
    cfg_from_yaml_file(CFGS.format(name), cfg)
    return cfg


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


def launches(fn):
    """Device kernels and memsets of one call, counted by the profiler."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return int(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA))


def errors_vs_f64(anchors, gt, hip, ref, sincos):
    """Largest |target - float64 value| over the positive rows, for the HIP route and for the torch route: the best gt of
    every positive anchor is found again (fp32 nearest-axis BEV IoU over the gts of the anchor's class, multi-head row order)
    and ResidualCoder.encode_torch is evaluated in float64 from the fp32 inputs."""
    from toda_amd.pcdet.utils import box_utils

    flat = torch.cat([a.permute(3, 4, 0, 1, 2, 5).reshape(-1, a.shape[-1]) for a in anchors], 0)
    ends = torch.cumsum(torch.tensor([int(np.prod(a.shape[:-1])) for a in anchors], device=flat.device), 0)
    err = {"hip": 0.0, "torch": 0.0}
    for b in range(gt.shape[0]):
        rows = (hip["box_cls_labels"][b] > 0).nonzero().view(-1)
        if rows.numel() == 0:
            continue
        cls = torch.bucketize(rows, ends, right=True)
        a32 = flat[rows]
        iou = box_utils.boxes3d_nearest_bev_iou(a32[:, 0:7].contiguous(), gt[b, :, 0:7].contiguous())
        iou = torch.where(gt[b, :, -1].long()[None, :] == (cls + 1)[:, None], iou, torch.full_like(iou, -1.0))
        g, a = gt[b, iou.argmax(1), :-1].double(), a32.double()
        lo = float(np.float32(1e-5))
        gs, as_ = g[:, 3:6].clamp(min=lo), a[:, 3:6].clamp(min=lo)
        diag = torch.sqrt(as_[:, 0] ** 2 + as_[:, 1] ** 2)
        cols = [(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / as_[:, 2], *torch.log(gs / as_).unbind(1)]
        cols += [torch.cos(g[:, 6]) - torch.cos(a[:, 6]), torch.sin(g[:, 6]) - torch.sin(a[:, 6])] if sincos else [g[:, 6] - a[:, 6]]
        cols += [g[:, 7 + i] - a[:, 7 + i] for i in range(min(g.shape[1], a.shape[1]) - 7)]
        want = torch.stack(cols, 1)
        for route, out in (("hip", hip), ("torch", ref)):
            err[route] = max(err[route], float((out["box_reg_targets"][b, rows].double() - want).abs().max()))
    return err


def assigner_case(name, iters, warmup):
    cfg_name, grid, coder_cfg, n_gt, n_extra = SHAPES[name]
    cfg = load_cfg(cfg_name)
    head = cfg.MODEL.DENSE_HEAD
    head.TARGET_ASSIGNER_CONFIG.BOX_CODER_CONFIG = AttrDict(coder_cfg)
    coder = box_coder_utils.ResidualCoder(**coder_cfg)
    stride = head.ANCHOR_GENERATOR_CONFIG[0]["feature_map_stride"]
    pc_range = np.asarray(cfg.DATA_CONFIG.POINT_CLOUD_RANGE, np.float32)
    anchors, _ = AnchorHeadTemplate.generate_anchors(head.ANCHOR_GENERATOR_CONFIG, grid_size=np.array([grid[0] * stride, grid[1] * stride, 1]),
                                                     point_cloud_range=pc_range, anchor_ndim=coder.code_size)
    anchors = [a.cuda() for a in anchors]
    assigner = AxisAlignedTargetAssigner(head, cfg.CLASS_NAMES, coder, match_height=False)
    rng = np.random.default_rng(0)
    batch, n_cls = 4, len(cfg.CLASS_NAMES)
    gt = np.zeros((batch, n_gt + 8, 8 + n_extra), np.float32)            # 8 rows of trailing padding
    for b in range(batch):
        for m in range(n_gt):
            c = int(rng.integers(0, n_cls))
            size = np.asarray(head.ANCHOR_GENERATOR_CONFIG[c]["anchor_sizes"][0]) * rng.uniform(0.85, 1.15, 3)
            yaw = [0.0, np.pi / 2][int(rng.integers(0, 2))] + rng.uniform(-0.3, 0.3)
            gt[b, m, :7] = [rng.uniform(pc_range[0] + 1, pc_range[3] - 1), rng.uniform(pc_range[1] + 1, pc_range[4] - 1), -1.0, *size, yaw]
            gt[b, m, 7:7 + n_extra] = rng.uniform(-3, 3, n_extra)
            gt[b, m, -1] = c + 1
    gt = torch.from_numpy(gt).cuda()
    hip, ref = assigner.assign_targets_hip(anchors, gt), assigner.assign_targets_torch(anchors, gt.clone())
    labels = hip["box_cls_labels"]
    pos = labels > 0
    err = errors_vs_f64(anchors, gt, hip, ref, coder.encode_angle_by_sincos)
    t_hip = timed(lambda: assigner.assign_targets_hip(anchors, gt), iters, warmup)
    t_torch = timed(lambda: assigner.assign_targets_torch(anchors, gt), max(3, iters // 4), 1)
    a, code = int(labels.shape[1]), int(hip["box_reg_targets"].shape[2])
    write = batch * a * code * 4
    return {
        "batch": batch, "anchors_per_sample": a, "classes": n_cls, "gts_per_sample": n_gt, "code": code,
        "hip_us": round(t_hip, 1), "torch_us": round(t_torch, 1), "torch_over_hip": round(t_torch / t_hip, 1),
        "hip_launches": launches(lambda: assigner.assign_targets_hip(anchors, gt)),
        "torch_launches": launches(lambda: assigner.assign_targets_torch(anchors, gt)),
        "positives": int(pos.sum()), "negatives": int((labels == 0).sum()), "ignored": int((labels < 0).sum()),
        "labels_differ_from_torch": int((labels != ref["box_cls_labels"]).sum()),      # unscreened inputs: reported, not asserted
        "max_abs_target_diff_vs_torch": float((hip["box_reg_targets"] - ref["box_reg_targets"])[pos & (ref["box_cls_labels"] > 0)].abs().max()),
        "max_abs_target_err_vs_f64_hip": err["hip"], "max_abs_target_err_vs_f64_torch": err["torch"],
        "target_bytes": write, "roof_us": round(write / (HBM_GBS * 1e3), 1), "hbm_fraction": round(write / (HBM_GBS * 1e3) / t_hip, 3),
    }


def train_step(steps):
    from toda_amd.pcdet.datasets import SyntheticLidarDataset
    from toda_amd.pcdet.models import build_network, prepare_batch_on_gpu

    cfg = load_cfg("cbgs_pp_multihead_nuscenes")
    ds = SyntheticLidarDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=True)
    torch.manual_seed(0)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    bs = cfg.OPTIMIZATION.BATCH_SIZE_PER_GPU
    out = {}
    for route in ("hip", "torch"):
        os.environ["TODA_ANCHOR_ASSIGN"] = route
        times = []
        for step in range(steps + 2):
            batch = ds.collate_batch([ds[(bs * step + i) % len(ds)] for i in range(bs)])
            prepare_batch_on_gpu(batch, net)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opt.zero_grad()
            ret, _, _ = net(batch)
            ret["loss"].backward()
            opt.step()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out[f"step_ms_{route}"] = round(float(np.median(times[2:])), 2)
    os.environ.pop("TODA_ANCHOR_ASSIGN")
    out["batch"] = bs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=5)
    args = ap.parse_args()
    res = {"bench": "anchor_head", "device": torch.cuda.get_device_name(0)}
    for name in SHAPES:
        res[name] = assigner_case(name, args.iters, args.warmup)
    if args.train_steps > 0:
        res["pointpillars_multihead_train"] = train_step(args.train_steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
