#!/usr/bin/env python
"""SECOND-IoU's RoI head at the TODA shape (4 samples x 128 sampled rois, BEV map 512 x 254 x 254, 7 x 7 grid): the grid-pool
kernel priced against HBM bytes beside the reference's torch composition (per-sample affine_grid + grid_sample on the GPU),
toda_roi_iou3d_max, the head's forward + backward (sampler included), and training samples/s of the targetmix config.

    python -m toda_amd.tools.bench_roi_head [--iters 20] [--warmup 5] [--train-steps 10]

Prints one JSON line.  Pool bytes: the output written once plus at most four taps read per output element (an upper bound:
neighbouring cells share taps); the lower bound is the output alone.  The map (528 MB) exceeds the 256 MiB Infinity Cache,
one sample's plane stack (132 MB) fits."""
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
from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file  # noqa: E402
from toda_amd.pcdet.models.roi_heads.second_head import roi_grid_pool_torch  # noqa: E402

HBM_GBS = 8000.0      # MI355X peak HBM bandwidth
GEOM = (-76.2, -76.2, 0.075, 0.075, 8, 7)
CFG = os.path.join(ROOT, "toda_amd", "tools", "cfgs", "models", "toda_stage1_secondiou_targetmix.yaml")


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


def random_boxes(gen, b, n, extent):
    boxes = torch.zeros((b, n, 7), device="cuda")
    boxes[..., 0:2] = torch.rand((b, n, 2), device="cuda", generator=gen) * 2 * extent - extent
    boxes[..., 2] = -1.0
    boxes[..., 3:6] = torch.rand((b, n, 3), device="cuda", generator=gen) * torch.tensor([2.0, 0.6, 0.4], device="cuda") \
        + torch.tensor([3.6, 1.7, 1.5], device="cuda")
    boxes[..., 6] = torch.rand((b, n), device="cuda", generator=gen) * 2 * np.pi - np.pi
    return boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--train-warmup", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    b, c, h, w, n = 4, 512, 254, 254, 128
    feat = torch.randn((b, c, h, w), device="cuda", generator=gen)
    rois = random_boxes(gen, b, n, 70.0)
    res = {"shape": {"B": b, "C": c, "H": h, "W": w, "rois_per_sample": n, "grid": 7}}

    out_bytes = b * n * c * 49 * 4
    pool_us = timed(lambda: ops.roi_grid_pool(feat, rois, *GEOM), args.iters, args.warmup)
    torch_us = timed(lambda: roi_grid_pool_torch(feat, rois, *GEOM), args.iters, args.warmup)
    hi = out_bytes * 5
    res["pool"] = {"us": round(pool_us, 1), "MB_out": round(out_bytes / 1e6, 1), "MB_upper": round(hi / 1e6, 1),
                   "GB_s_upper": round(hi / (pool_us * 1e-6) / 1e9, 1), "GB_s_out": round(out_bytes / (pool_us * 1e-6) / 1e9, 1),
                   "hbm_pct_upper": round(100 * hi / (pool_us * 1e-6) / 1e9 / HBM_GBS, 1),
                   "torch_composition_us": round(torch_us, 1), "speedup_vs_torch": round(torch_us / pool_us, 2)}

    # 3-D IoU max: the training proposals (512 per sample after NMS) against 40 gts, restricted to the roi's class
    props = random_boxes(gen, b, 512, 70.0)
    gt = torch.zeros((b, 48, 8), device="cuda")
    gt[:, :40, :7] = random_boxes(gen, b, 40, 70.0)
    gt[:, :40, 7] = 1
    props[:, :256] = gt[:, torch.randint(0, 40, (256,), generator=None), :7] + 0.2
    labels = torch.ones((b, 512), dtype=torch.long, device="cuda")
    res["roi_iou3d_max_us"] = round(timed(lambda: ops.roi_iou3d_max(props, labels, gt, True), args.iters, args.warmup), 1)

    # the head's training forward + backward at the config's sizes (sampler with its D2H / H2D included), rois given
    cfg = AttrDict()
    cfg_from_yaml_file(CFG, cfg)
    from toda_amd.pcdet.models.roi_heads import SECONDHead
    torch.manual_seed(0)
    np.random.seed(0)
    head = SECONDHead(input_channels=512, model_cfg=cfg.MODEL.ROI_HEAD, num_class=1).cuda().train()
    feat_g = feat.clone().requires_grad_(True)

    def head_step():
        bd = {"batch_size": b, "rois": props, "roi_scores": torch.rand((b, 512), device="cuda"), "roi_labels": labels,
              "gt_boxes": gt, "spatial_features_2d": feat_g, "dataset_cfg": cfg.DATA_CONFIG}
        head(bd)
        loss, _ = head.get_loss()
        loss.backward()

    res["head_fwd_bwd_us"] = round(timed(head_step, args.iters, args.warmup), 1)

    # training samples/s of the targetmix config (batches mixed and collated up front; voxelisation, rulebooks, forward,
    # backward and the optimizer step timed)
    from toda_amd.pcdet.datasets import SyntheticMixDataset
    from toda_amd.pcdet.models import build_network, prepare_batch_on_gpu
    from toda_amd.tools.train_utils.optimization import build_optimizer
    ds = SyntheticMixDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=True)
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    opt = build_optimizer(net, cfg.OPTIMIZATION)
    bs = cfg.OPTIMIZATION.BATCH_SIZE_PER_GPU
    steps = args.train_steps + args.train_warmup
    batches = [ds.collate_batch([ds[(i * bs + j) % len(ds)] for j in range(bs)]) for i in range(steps)]
    torch.cuda.synchronize()
    t0 = None
    for i, batch in enumerate(batches):
        if i == args.train_warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        prepare_batch_on_gpu(batch, net)
        opt.zero_grad()
        ret, _, _ = net(batch)
        ret["loss"].backward()
        opt.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res["train"] = {"config": "toda_stage1_secondiou_targetmix", "batch": bs, "steps": args.train_steps,
                    "ms_per_step": round(1e3 * dt / args.train_steps, 1), "samples_per_s": round(bs * args.train_steps / dt, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
