"""Time the KITTI AP evaluator (datasets/kitti/kitti_object_eval_python) on seeded synthetic annotations; one JSON line.

    python -m toda_amd.tools.bench_kitti_eval [--repeats 7] [--warmup 1] [--host-frames 40]

Two shapes, both ASSUMPTIONS about the real validation sets (stated in the output): KITTI-val-like (3769 frames, about 8
ground truths and 20 detections per frame, 3 classes) and nuScenes-val-like (6019 frames, about 35 and 100).  The annotations
are LiDAR-frame boxes through transform_annotations_to_kitti_format, the route of the camera-less datasets, so every image
box is the placeholder.  Per shape: the median wall time of get_official_eval_result (device synchronised only where the
evaluator reads back), one more run with every step bracketed by synchronisations for the split into overlap kernels,
matching kernels, transfers and host work, the number of launches, and the time of the pure-Python fp32 restatement
(tests/kitti_eval_cases.py, run from the repository root) on the first --host-frames frames."""
import argparse
import copy
import json
import time

import numpy as np
import torch

SHAPES = {
    "kitti_val_like": {"frames": 3769, "mean_gt": 8, "max_fp": 28, "names": ("car", "pedestrian", "bicycle"), "seed": 1},
    "nuscenes_val_like": {"frames": 6019, "mean_gt": 35, "max_fp": 145, "names": ("car", "pedestrian", "bicycle"), "seed": 2},
}
MAPPING = {"car": "Car", "pedestrian": "Pedestrian", "bicycle": "Cyclist"}


def make(shape):
    from tests import kitti_eval_cases as cases

    from ..pcdet.datasets.kitti.kitti_utils import transform_annotations_to_kitti_format
    infos, dets = cases.lidar_frames(shape["seed"], shape["frames"], shape["names"], shape["mean_gt"], shape["max_fp"])
    transform_annotations_to_kitti_format(infos, map_name_to_kitti=MAPPING)
    transform_annotations_to_kitti_format(dets, map_name_to_kitti=MAPPING)
    return infos, dets


def case(shape, repeats, warmup, host_frames):
    from tests import kitti_eval_cases as cases

    from ..pcdet.datasets.kitti.kitti_object_eval_python import eval as ev
    gts, dts = make(shape)
    classes = ["Car", "Pedestrian", "Cyclist"]
    held = {}

    def backend(timed):
        def build(prep):
            held["be"] = ev.DeviceBackend(prep, timed=timed)
            return held["be"]
        return build

    walls = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        text, res = ev.get_official_eval_result(gts, dts, classes, backend=backend(False))
        torch.cuda.synchronize()
        if i >= warmup:
            walls.append(time.perf_counter() - t0)
    launches, transfers = held["be"].stats["launches"], held["be"].stats["transfers"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.get_official_eval_result(gts, dts, classes, backend=backend(True))
    torch.cuda.synchronize()
    timed_wall = time.perf_counter() - t0
    st = held["be"].stats
    n = min(host_frames, len(gts))
    t0 = time.perf_counter()
    ev.get_official_eval_result(copy.deepcopy(gts[:n]), copy.deepcopy(dts[:n]), classes, backend=cases.HostBackend)
    host = time.perf_counter() - t0
    return {
        "assumed_shape": {"frames": len(gts), "gts_per_frame": round(float(np.mean([len(g["name"]) for g in gts])), 1),
                          "dets_per_frame": round(float(np.mean([len(d["name"]) for d in dts])), 1), "classes": len(classes)},
        "pairs": int(sum(len(g["name"]) * len(d["name"]) for g, d in zip(gts, dts))),
        "wall_s_median": round(float(np.median(walls)), 4), "wall_s_min_max": [round(min(walls), 4), round(max(walls), 4)],
        "wall_s_all": [round(w, 4) for w in walls],
        "launches": launches, "transfers": transfers,
        "split_s_synchronised_run": {"overlap_kernels": round(st["overlap_s"], 4), "matching_kernels": round(st["match_s"], 4),
                                     "transfers": round(st["transfer_s"], 4),
                                     "host": round(timed_wall - st["overlap_s"] - st["match_s"] - st["transfer_s"], 4),
                                     "wall": round(timed_wall, 4)},
        "host_restatement_fp32": {"frames": n, "seconds": round(host, 3), "seconds_per_frame": round(host / max(n, 1), 4)},
        "Car_3d_moderate_R40": round(float(res["Car_3d/moderate_R40"]), 4),
    }


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-frames", type=int, default=40)
    args = ap.parse_args(argv)
    out = {"bench": "kitti_eval", "device": torch.cuda.get_device_name(0),
           "note": "both shapes are assumptions; the reference's numba path runs on neither machine, so there is no ratio"}
    for name, shape in SHAPES.items():
        out[name] = case(shape, args.repeats, args.warmup, args.host_frames)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
