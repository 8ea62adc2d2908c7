"""Time the Lyft mAP evaluator (eval_metric 'lyft', datasets/lyft/lyft_eval.py) on a seeded synthetic workload; one JSON line,
also written to --out.

    python -m toda_amd.tools.bench_lyft_eval [--samples 3780] [--repeats 3] [--host-samples 40] [--out profiles/lyft_eval_bench.json]

The shape is an ASSUMPTION about the Lyft validation split and a CenterPoint-like detector (stated in the output): 3780 samples,
nine classes, 30 .. 150 ground truths a sample (two thirds of them cars) and up to 500 predictions: one near most ground truths,
the rest scattered around them.  Measured: each kernel (device events around the call, which includes the copy of the host
offsets into the workspace; median of --repeats), the torch curves, the whole evaluate() from the loaded tables, and the numpy
route (lyft_eval.flags_host: the same IoU in numpy and the reference's sequential walk) on the first --host-samples samples,
scaled to all samples.  The reference's own evaluator needs shapely, pyquaternion and the Lyft SDK, which are on no machine this
project runs on: no ratio to it exists."""
import argparse
import json
import os
import time

import numpy as np
import torch

from ..pcdet.datasets.lyft import lyft_eval as ev
from ..pcdet.datasets.nuscenes.nuscenes_eval import matrices_to_quats

CLASS_NAMES = ["car", "truck", "bus", "emergency_vehicle", "other_vehicle", "motorcycle", "bicycle", "pedestrian", "animal"]
CLASS_SHARE = (0.66, 0.04, 0.03, 0.002, 0.1, 0.008, 0.05, 0.1, 0.01)
SIZES = ((4.6, 1.9, 1.7), (8.0, 2.6, 3.2), (11.0, 2.9, 3.4), (6.0, 2.3, 2.4), (7.5, 2.6, 3.0), (2.2, 0.9, 1.5), (1.8, 0.6, 1.4), (0.8, 0.7, 1.75), (0.9, 0.4, 0.6))
THRESHOLDS = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]


def rot_zyx(yaw, pitch, roll):
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def make(samples, seed):
    """(infos, det_annos, tables) of `samples` samples."""
    rng = np.random.default_rng(seed)
    infos, dets, anns, instances = [], [], [], []
    categories = [{"token": f"cat{k}", "name": name} for k, name in enumerate(CLASS_NAMES)]
    names = np.array(CLASS_NAMES)
    for s in range(samples):
        tok = f"sample{s:05d}"
        ref_to_car, car_to_global = np.eye(4), np.eye(4)
        ref_to_car[:3, :3], ref_to_car[:3, 3] = rot_zyx(rng.uniform(-0.02, 0.02), rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)), [1.2, 0.0, 1.8]
        car_to_global[:3, :3] = rot_zyx(rng.uniform(-np.pi, np.pi), rng.uniform(-0.04, 0.04), rng.uniform(-0.04, 0.04))
        car_to_global[:3, 3] = [rng.uniform(500, 2500), rng.uniform(500, 2500), rng.uniform(-30, 10)]
        infos.append({"token": tok, "ref_to_car": ref_to_car, "car_to_global": car_to_global})
        G = car_to_global @ ref_to_car
        n = int(rng.integers(30, 151))
        cls = rng.choice(len(CLASS_NAMES), n, p=np.array(CLASS_SHARE) / sum(CLASS_SHARE))
        size = np.array(SIZES)[cls] * rng.uniform(0.8, 1.25, (n, 3))
        boxes = np.concatenate([rng.uniform(-75, 75, (n, 2)), rng.uniform(-1.5, 0.5, (n, 1)), size, rng.uniform(-np.pi, np.pi, (n, 1))], 1)
        centres = boxes[:, :3] @ G[:3, :3].T + G[:3, 3]
        quats = matrices_to_quats(np.stack([G[:3, :3] @ rot_zyx(h, 0.0, 0.0) for h in boxes[:, 6]]))
        for i in range(n):
            instances.append({"token": f"i{s}_{i}", "category_token": f"cat{cls[i]}"})
            anns.append({"token": f"a{s}_{i}", "sample_token": tok, "instance_token": f"i{s}_{i}", "translation": centres[i].tolist(),
                         "size": [boxes[i, 4], boxes[i, 3], boxes[i, 5]], "rotation": quats[i].tolist()})
        found = rng.random(n) < 0.85
        k = int(found.sum())
        tp = boxes[found] + np.concatenate([rng.normal(0, 0.1, (k, 3)), rng.normal(0, 0.05, (k, 3)), rng.normal(0, 0.05, (k, 1))], 1)
        n_fp = min(500 - k, int(rng.integers(150, 450)))
        pick = rng.integers(0, n, n_fp)
        fp = boxes[pick] + np.concatenate([rng.normal(0, 1.5, (n_fp, 2)), rng.normal(0, 0.2, (n_fp, 1)), np.zeros((n_fp, 3)), rng.normal(0, 0.5, (n_fp, 1))], 1)
        fp[:, 3:6] *= rng.uniform(0.8, 1.25, (n_fp, 3))
        dets.append({"name": np.concatenate([names[cls[found]], names[cls[pick]]]), "boxes_lidar": np.concatenate([tp, fp]).astype(np.float32),
                     "score": np.concatenate([rng.uniform(0.3, 1.0, k), rng.uniform(0.1, 0.6, n_fp)]).astype(np.float32), "metadata": {"token": tok}})
    return infos, dets, {"sample_annotation": anns, "instance": instances, "category": categories}


def device_pass(seg):
    """Both kernels and the curves -> (best ms, flags ms, curves ms, aps)."""
    from .. import ops
    dev = torch.device("cuda")
    pred, gt, score = ops.eval_upload(seg["pred"], np.float64, dev), ops.eval_upload(seg["gt"], np.float64, dev), ops.eval_upload(seg["pred_score"], np.float64, dev)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    e[0].record()
    best_iou, best_gt = ops.lyft_eval_best(pred, gt, seg["pred_off"], seg["gt_off"])
    e[1].record()
    tp = ops.lyft_eval_flags(score, best_iou, best_gt, seg["pred_off"], THRESHOLDS)
    e[2].record()
    aps = ev.average_precisions(tp, seg["pred_score"], seg["pred_cls"], seg["n_gt"], len(CLASS_NAMES))
    e[3].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3]), aps, tp


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3780)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-samples", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "lyft_eval_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lyft_eval times the device route: it needs an MI355X (there is no CPU fallback)")
    infos, dets, tables = make(args.samples, args.seed)
    walls = []
    for _ in range(2):                                      # the first call also loads the library and warms the allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        text, res = ev.evaluate(infos, dets, CLASS_NAMES, None, THRESHOLDS, tables=tables)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    gt_rows = ev.ground_truth_rows(tables, [d["metadata"]["token"] for d in dets])
    rows_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    seg = ev.segment(infos, dets, CLASS_NAMES, gt_rows)
    order_s = time.perf_counter() - t0
    runs = [device_pass(seg) for _ in range(args.repeats + 1)][1:]
    n_host = min(args.host_samples, args.samples)
    head = ev.segment(infos, dets[:n_host], CLASS_NAMES, gt_rows)
    t0 = time.perf_counter()
    host_tp, _, _ = ev.flags_host(head, THRESHOLDS)
    host_s = time.perf_counter() - t0
    same = bool(np.array_equal(host_tp, runs[0][4][:, :len(head["pred"])].cpu().numpy()))        # the first samples open the CSR order
    pairs = int((np.diff(seg["pred_off"]).astype(np.int64) * np.diff(seg["gt_off"])).sum())
    out = {"bench": "lyft_eval", "device": torch.cuda.get_device_name(0),
           "assumed_shape": {"samples": args.samples, "classes": len(CLASS_NAMES), "cutoffs": len(THRESHOLDS), "gts_per_sample": round(len(tables["sample_annotation"]) / args.samples, 1),
                             "preds_per_sample": round(len(seg["pred"]) / args.samples, 1), "segments": int(len(seg["pred_off"]) - 1), "pairs": pairs,
                             "largest_segment": [int(np.diff(seg["pred_off"]).max()), int(np.diff(seg["gt_off"]).max())]},
           "best_kernel_ms_median": round(float(np.median([r[0] for r in runs])), 3), "flags_kernel_ms_median": round(float(np.median([r[1] for r in runs])), 3),
           "curves_torch_ms_median": round(float(np.median([r[2] for r in runs])), 3), "best_kernel_ms_all": [round(r[0], 3) for r in runs],
           "ground_truth_rows_host_s": round(rows_s, 3), "prediction_rows_and_order_host_s": round(order_s, 3), "evaluate_wall_s": [round(w, 3) for w in walls],
           "host_numpy_route": {"samples": n_host, "seconds": round(host_s, 3), "seconds_per_sample": round(host_s / max(n_host, 1), 5),
                                "scaled_to_all_samples_s": round(host_s / max(n_host, 1) * args.samples, 1), "flags_equal_device": same},
           "car_AP": round(float(res["car"]), 4), "mAP": round(float(res["mAP"]), 4),
           "note": "the shape is an assumption; the kernel times include the copy of the host offsets into the workspace; the host route is the "
                   "vectorised numpy IoU of this project plus the reference's sequential walk, not the reference's shapely loop, which is on no "
                   "machine this project runs on: no ratio to it exists"}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
