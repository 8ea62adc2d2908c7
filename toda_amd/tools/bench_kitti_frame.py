#!/usr/bin/env python
"""Timing of KittiDataset's per-frame point work:
    python -m toda_amd.tools.bench_kitti_frame [--out profiles/kitti_frame_bench.json]
A synthetic 120 000-point, 4-column frame (a KITTI sweep's size) under a KITTI-like calibration:
  * the device chain of KittiDataset.fov_points - one H2D copy, toda_points_fov_flags, the stable compaction (its row-count read
    included) - against the reference's host route: numpy lidar_to_rect + rect_to_img + boolean indexing, then the H2D copy of
    the cropped cloud.  Wall time, device idle at both ends.  The flag kernel alone is also timed with HIP events; its rate is
    given at its 4 c + 4 bytes per point as a fraction of the 8 TB/s HBM roof.
  * the info builder's point count for 15 boxes (points_in_boxes mode 2 + bincount on the cropped cloud, read-back included)
    against one Delaunay hull test per box (scipy; left out when scipy is not importable).
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from toda_amd import ops  # noqa: E402
from toda_amd.pcdet.datasets.kitti.kitti_dataset import KittiDataset  # noqa: E402
from toda_amd.pcdet.utils import box_utils, calibration_kitti  # noqa: E402
from toda_amd.tools.bench_local_aug import HBM_ROOF, events, wall  # noqa: E402

N_POINTS, N_BOXES, SHAPE = 120_000, 15, (375, 1242)


def make_frame(seed=0):
    rng = np.random.default_rng(seed)
    calib = calibration_kitti.Calibration({
        "P2": np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]], np.float32),
        "R0": np.array([[0.9999, 0.0098, -0.0074], [-0.0099, 0.9999, -0.0043], [0.0074, 0.0044, 0.9999]], np.float32),
        "Tr_velo2cam": np.array([[0.0075, -0.9999, -0.0006, -0.0041], [0.0148, 0.0007, -0.9998, -0.0763], [0.9998, 0.0075, 0.0148, -0.2718]], np.float32)})
    theta, r = rng.uniform(-np.pi, np.pi, N_POINTS), 2.0 + 68.0 * rng.uniform(0, 1, N_POINTS) ** 1.5
    points = np.stack([r * np.cos(theta), r * np.sin(theta), rng.uniform(-2.0, 0.5, N_POINTS), rng.uniform(0, 1, N_POINTS)], 1).astype(np.float32)
    boxes = np.stack([rng.uniform(6, 60, N_BOXES), rng.uniform(-10, 10, N_BOXES), rng.uniform(-1.2, -0.6, N_BOXES), rng.uniform(3.5, 4.5, N_BOXES),
                      rng.uniform(1.5, 1.9, N_BOXES), rng.uniform(1.4, 1.8, N_BOXES), rng.uniform(-np.pi, np.pi, N_BOXES)], 1).astype(np.float32)
    return calib, points, boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kitti_frame_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    calib, points, boxes = make_frame()
    shape = np.array(SHAPE, np.int32)
    m, p2 = calib.fov_matrices()
    ds = KittiDataset.__new__(KittiDataset)            # fov_points reads no attribute of the instance

    def host_route():
        keep = KittiDataset.get_fov_flag(calib.lidar_to_rect(points[:, 0:3]), shape, calib)
        return torch.from_numpy(points[keep]).cuda()

    t_dev = wall(lambda: ds.fov_points(points, calib, shape), args.iters)
    t_host = wall(host_route, args.iters)
    cropped_dev, cropped_host = ds.fov_points(points, calib, shape), host_route()
    pts_dev = torch.from_numpy(points).cuda()
    ms_flags = events(lambda: ops.points_fov_flags(pts_dev, m, p2, shape))
    rate = N_POINTS * (4 * points.shape[1] + 4) / (ms_flags * 1e-3)
    res = {"bench": "kitti_frame", "device": torch.cuda.get_device_name(0), "points": N_POINTS, "columns": int(points.shape[1]),
           "rows_in_view": int(cropped_dev.shape[0]), "rows_in_view_numpy": int(cropped_host.shape[0]),
           "fov_crop": {"device_chain_ms": round(t_dev, 4), "numpy_route_ms": round(t_host, 4), "ratio": round(t_host / t_dev, 2)},
           "fov_flags_kernel": {"us_with_flag_zeroing": round(ms_flags * 1e3, 2), "bytes_per_point": 4 * points.shape[1] + 4,
                                "algorithmic_GBps": round(rate / 1e9, 1), "fraction_of_8TBps_roof": round(rate / HBM_ROOF, 4)}}
    bx_dev = torch.from_numpy(boxes).cuda()

    def count_dev():
        owner = ops.points_in_boxes(cropped_dev, bx_dev, mode=2)
        return torch.bincount(owner[owner >= 0].long(), minlength=N_BOXES).cpu().numpy()

    count = {"boxes": N_BOXES, "device_ms": round(wall(count_dev, args.iters), 4)}
    try:
        from scipy.spatial import Delaunay
    except ImportError:
        Delaunay = None
    if Delaunay is not None:
        kept, corners = cropped_host.cpu().numpy(), box_utils.boxes_to_corners_3d(boxes)

        def count_hull():
            return np.array([(Delaunay(corners[k]).find_simplex(kept[:, 0:3]) >= 0).sum() for k in range(N_BOXES)])

        count["hull_per_box_ms"] = round(wall(count_hull, max(1, args.iters // 4)), 4)
        count["ratio"] = round(count["hull_per_box_ms"] / count["device_ms"], 2)
        count["counts_agree"] = bool(np.array_equal(count_dev(), count_hull()))
    res["num_points_in_gt"] = count
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
