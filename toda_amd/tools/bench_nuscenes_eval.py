"""Time the nuScenes mAP / NDS evaluator (eval_metric 'nds', datasets/nuscenes/nuscenes_eval.py) on a seeded synthetic workload;
one JSON line, also written to --out.

    python -m toda_amd.tools.bench_nuscenes_eval [--samples 6019] [--repeats 5] [--host-samples 200] [--out profiles/nuscenes_eval_bench.json]

The shape is an ASSUMPTION about the nuScenes validation set (stated in the output): 6019 samples, about 30 ground truths and
100 .. 500 predictions each, ten classes.  Measured: the two kernels alone (device events, median of --repeats), the whole
evaluate() call (tables, both kernels, orders, curves, both JSON files), and the matching in numpy on the host - per (sample,
class) one vectorised distance matrix and the greedy walk over the predictions, for the first --host-samples samples, checked
against the kernel's match table."""
import argparse
import functools
import json
import os
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

from ..pcdet.datasets.nuscenes import nuscenes_eval as ev

CLASS_SHARE = (0.43, 0.07, 0.02, 0.02, 0.01, 0.20, 0.01, 0.01, 0.08, 0.15)        # roughly the validation set's class mix
ATTRIBUTE_OF = {"car": "vehicle.parked", "truck": "vehicle.parked", "bus": "vehicle.moving", "trailer": "vehicle.parked",
                "construction_vehicle": "vehicle.parked", "pedestrian": "pedestrian.moving", "motorcycle": "cycle.without_rider",
                "bicycle": "cycle.without_rider", "traffic_cone": "", "barrier": ""}


def make(samples, seed, root, version):
    """(infos, det_annos) and the four tables under root / version."""
    rng = np.random.default_rng(seed)
    infos, dets = [], []
    tables = {"attribute": [{"token": f"attr_{a}", "name": a} for a in sorted(set(ATTRIBUTE_OF.values())) if a],
              "category": [{"token": f"cat_{c}", "name": c} for c in ev.CLASSES], "instance": [{"token": f"inst_{c}", "category_token": f"cat_{c}"} for c in ev.CLASSES],
              "sample_annotation": []}
    for s in range(samples):
        yaw = rng.uniform(-np.pi, np.pi)
        car_to_global = np.eye(4)
        car_to_global[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        car_to_global[:3, 3] = [rng.uniform(0, 2000), rng.uniform(0, 2000), 0.0]
        lidar_to_car = np.eye(4)
        lidar_to_car[:3, 3] = [0.94, 0.0, 1.84]
        n_gt = int(rng.integers(10, 51))
        cls = rng.choice(10, n_gt, p=CLASS_SHARE)
        boxes = np.concatenate([rng.uniform(-45, 45, (n_gt, 2)), rng.uniform(-2, 0, (n_gt, 1)), rng.uniform(0.4, 5, (n_gt, 3)),
                                rng.uniform(-np.pi, np.pi, (n_gt, 1)), rng.uniform(-2, 2, (n_gt, 2))], 1).astype(np.float32)
        names = np.array(ev.CLASSES)[cls]
        tokens = np.array([f"a{s}_{i}" for i in range(n_gt)])
        infos.append({"token": f"s{s}", "ref_from_car": np.linalg.inv(lidar_to_car), "car_from_global": np.linalg.inv(car_to_global), "gt_boxes": boxes,
                      "gt_boxes_velocity": np.concatenate([boxes[:, 7:9], np.zeros((n_gt, 1), np.float32)], 1), "gt_names": names, "gt_boxes_token": tokens})
        for tok, name in zip(tokens, names):
            attr = ATTRIBUTE_OF[str(name)]
            tables["sample_annotation"].append({"token": str(tok), "sample_token": f"s{s}", "instance_token": f"inst_{name}",
                                                "attribute_tokens": [f"attr_{attr}"] if attr else [], "translation": [0.0, 0.0, 0.0],
                                                "size": [1.0, 1.0, 1.0], "rotation": [1.0, 0.0, 0.0, 0.0]})
        found = rng.random(n_gt) < 0.8
        n_pred = int(rng.integers(100, 501))
        n_fp = max(n_pred - int(found.sum()), 0)
        tp = boxes[found].astype(np.float64)
        tp[:, :2] += rng.normal(0, 0.6, (len(tp), 2))
        tp[:, 6] += rng.normal(0, 0.2, len(tp))
        fp = np.concatenate([rng.uniform(-55, 55, (n_fp, 2)), rng.uniform(-2, 0, (n_fp, 1)), rng.uniform(0.4, 5, (n_fp, 3)),
                             rng.uniform(-np.pi, np.pi, (n_fp, 1)), rng.uniform(-2, 2, (n_fp, 2))], 1)
        dets.append({"name": np.concatenate([names[found], np.array(ev.CLASSES)[rng.choice(10, n_fp, p=CLASS_SHARE)]]),
                     "score": np.concatenate([rng.uniform(0.3, 1.0, len(tp)), rng.uniform(0.05, 0.6, n_fp)]), "boxes_lidar": np.concatenate([tp, fp], 0),
                     "metadata": {"token": f"s{s}"}})
    (Path(root) / version).mkdir(parents=True)
    for name, rows in tables.items():
        with open(Path(root) / version / f"{name}.json", "w") as f:
            json.dump(rows, f)
    return infos, dets


def match_numpy(pred, score, gt, pred_off, gt_off, n_seg):
    """The match table [4, pred_off[n_seg]] of the first n_seg segments on the host: one distance matrix per segment, then the
    greedy walk."""
    out = np.full((4, int(pred_off[n_seg])), -1, np.int32)
    for s in range(n_seg):
        p0, p1, g0, g1 = pred_off[s], pred_off[s + 1], gt_off[s], gt_off[s + 1]
        if p1 == p0 or g1 == g0:
            continue
        d = np.sqrt(((pred[p0:p1, None, :2] - gt[None, g0:g1, :2]) ** 2).sum(-1))
        order = np.lexsort((-np.arange(p1 - p0), -score[p0:p1]))
        for t, th in enumerate(ev.DIST_THS):
            free = np.ones(g1 - g0, bool)
            for i in order:
                row = np.where(free, d[i], np.inf)
                j = int(np.argmin(row))
                if row[j] < th:
                    free[j] = False
                    out[t, p0 + i] = g0 + j
    return out


def main(argv=None):
    from .. import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=6019)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-samples", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "nuscenes_eval_bench.json"))
    args = ap.parse_args(argv)
    version = "v1.0-trainval"
    with tempfile.TemporaryDirectory() as tmp:
        infos, dets = make(args.samples, args.seed, tmp, version)
        held = {}

        def recording(*a):
            held["args"] = a
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ev.match_on_device(*a)
            held["match_call_s"] = time.perf_counter() - t0
            return res

        walls = []
        for _ in range(2):                                  # the first call also loads the library and warms the allocator
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            text, res = ev.evaluate(infos, dets, list(ev.CLASSES), tmp, version, os.path.join(tmp, "out"), match_fn=recording)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        pred, score, p_attr, gt, g_attr, p_off, g_off, seg_cls = held["args"]
        dev = torch.device("cuda")
        up = functools.partial(ops.eval_upload, dev=dev)
        d_args = (up(pred, np.float64), up(score, np.float64), up(p_attr, np.int32), up(gt, np.float64), up(g_attr, np.int32))
        rows = up(np.random.default_rng(0).uniform(-40, 40, (len(pred) + len(gt), 10)), np.float64)
        sample = up(np.random.default_rng(0).integers(0, len(infos), len(pred) + len(gt)), np.int32)
        cls = up(np.random.default_rng(1).integers(0, 10, len(pred) + len(gt)), np.int32)
        G, _, ego = ev.sample_transforms(infos)
        G, ego = up(G, np.float64), up(ego, np.float64)
        prep_ms, match_ms = [], []
        for i in range(args.repeats + 1):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            ops.nusc_eval_prepare(rows, sample, cls, G, ego)
            e[1].record()
            match, err = ops.nusc_eval_match(*d_args, p_off, g_off, seg_cls)
            e[2].record()
            torch.cuda.synchronize()
            if i:
                prep_ms.append(e[0].elapsed_time(e[1]))
                match_ms.append(e[1].elapsed_time(e[2]))
        n_host = min(args.host_samples, len(infos))
        t0 = time.perf_counter()
        host = match_numpy(pred, score, gt, p_off, g_off, n_host * 10)
        host_s = time.perf_counter() - t0
        same = bool(np.array_equal(host, match.cpu().numpy()[:, :host.shape[1]]))
    out = {"bench": "nuscenes_eval", "device": torch.cuda.get_device_name(0),
           "assumed_shape": {"samples": len(infos), "gts_per_sample": round(float(np.mean([len(i["gt_names"]) for i in infos])), 1),
                             "preds_per_sample": round(float(np.mean([len(d["name"]) for d in dets])), 1), "classes": 10,
                             "kept_preds": int(len(pred)), "kept_gts": int(len(gt)), "segments": int(len(seg_cls))},
           "prepare_kernel_ms_median": round(float(np.median(prep_ms)), 3), "match_launch_ms_median": round(float(np.median(match_ms)), 3),
           "match_launch_ms_all": [round(v, 3) for v in match_ms],
           "match_call_with_transfers_s": round(held["match_call_s"], 4),
           "evaluate_wall_s": [round(w, 3) for w in walls],
           "host_numpy_matching": {"samples": n_host, "seconds": round(host_s, 3), "seconds_per_sample": round(host_s / max(n_host, 1), 5),
                                   "scaled_to_all_samples_s": round(host_s / max(n_host, 1) * len(infos), 2), "equals_kernel": same},
           "mAP": round(float(res["mAP"]), 4), "NDS": round(float(res["NDS"]), 4),
           "note": "the shape is an assumption; match_launch includes the copy of the host offsets into the workspace; the host route is "
                   "the tool's own numpy matching, not the devkit"}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
