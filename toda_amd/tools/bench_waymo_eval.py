"""Time the Waymo LEVEL_1 / LEVEL_2 AP / APH evaluator (eval_metric 'aph', datasets/waymo/waymo_eval.py) on a seeded synthetic
workload; one JSON line, also written to --out.

    python -m toda_amd.tools.bench_waymo_eval [--frames 39987] [--repeats 3] [--host-frames 100] [--out profiles/waymo_eval_bench.json]

The shape is an ASSUMPTION about the Waymo validation set and a CenterPoint-like detector (stated in the output): 39987 frames,
about 60 Vehicle, 25 Pedestrian and 2 Cyclist ground truths and 150 .. 300 predictions a frame.  Measured: the IoU kernel and the
match launch (device events around the calls, summed over the launches of at most MAX_SEGMENTS_PER_LAUNCH segments, median of
--repeats), the whole evaluate() call, and the host route's matching - scipy.optimize.linear_sum_assignment solved at each of the
101 cutoffs of every segment - on the IoU blocks of the first --host-frames frames, scaled to all frames.  No ratio to the official
C++ metric exists: that tool is on no machine this project runs on."""
import argparse
import functools
import json
import os
import time

import numpy as np
import torch

from ..pcdet.datasets.waymo import waymo_eval as ev

CLASS_NAMES = ["Vehicle", "Pedestrian", "Cyclist"]
GT_MEAN = (60, 25, 2)
SIZES = ((4.7, 2.1, 1.7), (0.9, 0.85, 1.7), (1.8, 0.8, 1.7))


def make(frames, seed):
    """(det_annos, gt_annos) of `frames` frames."""
    rng = np.random.default_rng(seed)
    dets, gts = [], []
    for _ in range(frames):
        counts = rng.poisson(GT_MEAN)
        cls = np.repeat(np.arange(3), counts)
        n = len(cls)
        size = np.array(SIZES)[cls] * rng.uniform(0.8, 1.25, (n, 3))
        boxes = np.concatenate([rng.uniform(-75, 75, (n, 2)), rng.uniform(-1, 2, (n, 1)), size, rng.uniform(-np.pi, np.pi, (n, 1))], 1)
        gts.append({"name": np.array(CLASS_NAMES)[cls], "difficulty": np.zeros(n, np.int64), "num_points_in_gt": rng.integers(0, 200, n) // rng.integers(1, 20, n),
                    "gt_boxes_lidar": boxes.astype(np.float32)})
        found = rng.random(n) < 0.85
        tp = boxes[found] + np.concatenate([rng.normal(0, 0.08, (int(found.sum()), 3)), rng.normal(0, 0.04, (int(found.sum()), 3)),
                                            rng.normal(0, 0.05, (int(found.sum()), 1))], 1)
        n_fp = int(rng.integers(100, 220))
        near = boxes[rng.integers(0, max(n, 1), n_fp)] if n else np.zeros((n_fp, 7))
        fp = near + np.concatenate([rng.normal(0, 1.5, (n_fp, 2)), rng.normal(0, 0.2, (n_fp, 4)), rng.normal(0, 0.5, (n_fp, 1))], 1)
        fp_cls = cls[rng.integers(0, max(n, 1), n_fp)] if n else np.zeros(n_fp, np.int64)
        dets.append({"name": np.concatenate([np.array(CLASS_NAMES)[cls[found]], np.array(CLASS_NAMES)[fp_cls]]),
                     "score": np.concatenate([rng.uniform(0.3, 1.0, len(tp)), rng.uniform(0.1, 0.6, n_fp)]), "boxes_lidar": np.concatenate([tp, fp])})
    return dets, gts


def device_pass(seg):
    """Both kernels over every launch slice -> (iou ms, match ms, counts, the IoU blocks of the first slice on the host)."""
    from .. import ops
    dev = torch.device("cuda")
    iou_ms = match_ms = 0.0
    up = functools.partial(ops.eval_upload, dev=dev)
    counts, first = ev.empty_counts(), None
    for part in ev.launch_slices(seg, ev.MAX_SEGMENTS_PER_LAUNCH):
        pred, gt, score, level = up(part["pred_boxes"], np.float64), up(part["gt_boxes"], np.float64), up(part["pred_score"], np.float32), up(part["gt_level"], np.int32)
        ph, gh = pred[:, 6].contiguous(), gt[:, 6].contiguous()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        iou = ops.waymo_eval_iou(pred, gt, part["pred_off"], part["gt_off"])
        e[1].record()
        out = ops.waymo_eval_match(iou, score, ph, gh, level, part["pred_off"], part["gt_off"], part["seg_type"])
        e[2].record()
        torch.cuda.synchronize()
        iou_ms += e[0].elapsed_time(e[1])
        match_ms += e[1].elapsed_time(e[2])
        counts = tuple(c + o.cpu().numpy() for c, o in zip(counts, out[:4]))
        if first is None:
            first = iou.cpu().numpy()
    return iou_ms, match_ms, counts, first


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=39987)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "waymo_eval_bench.json"))
    args = ap.parse_args(argv)
    dets, gts = make(args.frames, args.seed)
    walls = []
    for _ in range(2):                                      # the first call also loads the library and warms the allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        text, res = ev.evaluate(dets, gts, CLASS_NAMES)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    seg = ev.segment(ev.prepare(dets, gts, CLASS_NAMES))
    prepare_s = time.perf_counter() - t0
    runs = [device_pass(seg) for _ in range(args.repeats + 1)][1:]
    n_host = min(args.host_frames, args.frames)
    head = ev.segment(ev.prepare(dets[:n_host], gts[:n_host], CLASS_NAMES))
    n_head = len(head["seg_type"])                          # the first frames' segments open the CSR order, and so the first launch slice
    blocks = runs[0][3][:int((np.diff(head["pred_off"]).astype(np.int64) * np.diff(head["gt_off"])).sum())]
    t0 = time.perf_counter()
    host_counts = ev.counts_host(head, iou=blocks)
    host_s = time.perf_counter() - t0
    head_dev = ev.counts_device(head)
    same = bool(all(np.array_equal(a, b) for a, b in zip(host_counts[:3], head_dev[:3])))
    n_pred, n_gt = len(seg["pred_score"]), len(seg["gt_level"])
    out = {"bench": "waymo_eval", "device": torch.cuda.get_device_name(0),
           "assumed_shape": {"frames": args.frames, "gts_per_frame": round(n_gt / args.frames, 1), "preds_per_frame": round(n_pred / args.frames, 1),
                             "types": 3, "segments": int(len(seg["seg_type"])), "pairs": int((np.diff(seg["pred_off"]).astype(np.int64) * np.diff(seg["gt_off"])).sum()),
                             "launches": -(-len(seg["seg_type"]) // ev.MAX_SEGMENTS_PER_LAUNCH)},
           "iou_kernel_ms_median": round(float(np.median([r[0] for r in runs])), 3), "match_launch_ms_median": round(float(np.median([r[1] for r in runs])), 3),
           "match_launch_ms_all": [round(r[1], 3) for r in runs], "prepare_and_order_host_s": round(prepare_s, 3),
           "evaluate_wall_s": [round(w, 3) for w in walls],
           "host_scipy_per_cutoff_matching": {"frames": n_host, "segments": n_head, "seconds": round(host_s, 3), "seconds_per_frame": round(host_s / max(n_host, 1), 5),
                                              "scaled_to_all_frames_s": round(host_s / max(n_host, 1) * args.frames, 1), "counts_equal_device": same},
           "VEHICLE_L2_APH": round(float(res["OBJECT_TYPE_TYPE_VEHICLE_LEVEL_2/APH"]), 4), "PEDESTRIAN_L2_APH": round(float(res["OBJECT_TYPE_TYPE_PEDESTRIAN_LEVEL_2/APH"]), 4),
           "note": "the shape is an assumption; the launches include the copy of the host offsets into the workspace; the host route is scipy's "
                   "linear_sum_assignment at each of the 101 cutoffs on the device's IoU blocks (where an optimum is not unique the counts may differ); "
                   "no ratio to the official C++ metric exists"}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
