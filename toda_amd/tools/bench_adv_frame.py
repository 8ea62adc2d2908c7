#!/usr/bin/env python
"""Timing of the adversarial edit of a pseudo-labelled frame (NuScenesMixUpAdvDataset.adversarial_points, csrc/adv_frame.hip):
    python -m toda_amd.tools.bench_adv_frame [--out profiles/adv_frame_bench.json]
Two synthetic frames in the stage-2 nuScenes geometry (range +-54 m / [-5, 4.8], voxels 0.075 x 0.075 x 0.2 m, the frame's own
voxels with random gradients):
  * one sweep:   about 35 000 rows, 20 pseudo boxes of some hundred rows each;
  * ten sweeps:  about 260 000 rows, 40 pseudo boxes, one of them (a truck next to the sensor) with more than 40 000 rows.
Per frame, with the same draws for both routes and the cloud resident on the device at the start and at the end:
  * device_chain_ms  adversarial_points: the voxel keys sorted and uploaded with the gradients, the box table uploaded,
                     toda_adv_edit, the row-count read - wall time, device idle at both ends;
  * host_route_ms    the cloud copied to the host, adversarial_points_host (numpy, one pass over the cloud per box), the
                     edited cloud copied back - the route a host edit would take on a device-resident frame;
  * kernels_us       toda_adv_edit alone (one memset and 14 kernels, and the reset of the output cursor) with HIP events,
                     buffers and tables allocated once;
  * the rate of that time at the bytes the edit needs - every row read once and every output row written once, 4 c bytes
    each - as a fraction of the 8 TB/s HBM roof.  The kernels move more than that: the membership pass and the two walks read
    the rows three times, and the membership words are written once and read five times - by the three histogram passes and
    the two walks.
Prints one JSON line and writes it to --out.  No ratio is asked: the baseline is the reference's algorithm on the host."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from toda_amd import lib as L  # noqa: E402
from toda_amd import ops  # noqa: E402
from toda_amd.pcdet.datasets.nuscenes.nuscenes_mixup_adv_dataset import NuScenesMixUpAdvDataset  # noqa: E402
from toda_amd.tools.bench_local_aug import HBM_ROOF, events, wall  # noqa: E402

RANGE = np.array([-54.0, -54.0, -5.0, 54.0, 54.0, 4.8], np.float32)
VOXEL = np.array([0.075, 0.075, 0.2], np.float32)
SHAPES = {"one_sweep": {"rows": 35_000, "boxes": 20, "rows_per_box": 300, "truck_rows": 0},
          "ten_sweeps": {"rows": 260_000, "boxes": 40, "rows_per_box": 1500, "truck_rows": 45_000}}


def make_frame(shape, seed=0):
    """(cloud [n, 5], pseudo info) of one shape: ground returns on rings round the sensor, one cluster per box."""
    rng = np.random.default_rng(seed)
    k, per_box, truck = shape["boxes"], shape["rows_per_box"], shape["truck_rows"]
    boxes, parts = [], []
    for j in range(k):
        big = truck and j == 0
        size = np.array([12.0, 3.0, 4.0] if big else [4.6, 1.9, 1.7])
        centre = np.array([8.0, 0.0, -0.5]) if big else np.array([rng.uniform(-45, 45), rng.uniform(-45, 45), rng.uniform(-1.5, -0.5)])
        boxes.append(list(centre) + list(size) + [rng.uniform(-np.pi, np.pi) if not big else 0.1])
        parts.append(centre + rng.uniform(-0.45, 0.45, (truck if big else per_box, 3)) * size * 0.6)
    n_ground = shape["rows"] - sum(len(p) for p in parts)
    theta, r = rng.uniform(-np.pi, np.pi, n_ground), 2.0 + 50.0 * rng.uniform(0, 1, n_ground) ** 1.5
    parts.append(np.stack([r * np.cos(theta), r * np.sin(theta), rng.uniform(-2.2, -1.6, n_ground)], 1))
    xyz = np.concatenate(parts, 0)[rng.permutation(shape["rows"])]
    cloud = np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1)), rng.integers(0, 10, (len(xyz), 1)) * 0.05], 1).astype(np.float32)
    cell = np.floor((cloud[:, :3] - RANGE[:3]) / VOXEL)
    grid = ops.grid_size_xyz(RANGE, VOXEL)
    inside = ((cell >= 0) & (cell < grid)).all(1)
    coords = np.unique(cell[inside].astype(np.int32)[:, ::-1], axis=0)
    info = {"token": f"bench{seed}", "lidar_path": "bench", "gt_boxes": np.asarray(boxes, np.float32), "gt_names": np.array(["car"] * k),
            "p_score": np.full(k, 0.9, np.float32), "p_voxel_coords": coords, "p_voxel_perturb": (rng.standard_normal((len(coords), 3)) * 30).astype(np.float32)}
    return cloud, info


def bench_shape(ds, name, shape, iters):
    cloud, info = make_frame(shape)
    np.random.seed(1)
    draws = ds.draw_edits(len(info["gt_boxes"]))
    dev = torch.from_numpy(cloud).cuda()

    def device_route():
        return ds.adversarial_points(dev, info, draws)

    def host_route():
        return torch.from_numpy(ds.adversarial_points_host(dev.cpu().numpy(), info, draws)).cuda()

    got, want = device_route().cpu().numpy(), host_route().cpu().numpy()
    t_dev, t_host = wall(device_route, iters), wall(host_route, max(3, iters // 4))

    # the entry point alone: tables and buffers allocated once
    lib = L.load()
    n, c = cloud.shape
    boxes = ds.adversarial_boxes(info)
    k = len(boxes)
    table = ops.adv_table(boxes, draws["op"], draws["frac"], draws["seed"])
    keys, grads = (torch.from_numpy(t).cuda() for t in ds.voxel_table(info))
    th, td = L.host_f64(table.reshape(-1)), torch.from_numpy(table).cuda()
    lo, vs, gs = L.host_f32(RANGE[:3]), L.host_f32(VOXEL), L.host_i32(ds.grid_size)
    cap = len(got) + 16
    dst = torch.empty((cap, c), dtype=torch.float32, device="cuda")
    cursor, counts = torch.zeros((1,), dtype=torch.int32, device="cuda"), torch.zeros((k,), dtype=torch.int32, device="cuda")
    ws_bytes = lib.toda_adv_edit_workspace_bytes(n, k)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")

    def launch():
        cursor.zero_()
        L.check(lib.toda_adv_edit(L.ptr(dev), n, c, L.hptr(th), L.ptr(td), k, L.ptr(keys), L.ptr(grads), len(keys), L.hptr(lo), L.hptr(vs), L.hptr(gs),
                                  ds.adv_eps, L.ptr(dst), cap, L.ptr(cursor), L.ptr(counts), L.ptr(ws), ws_bytes, L.stream()), "toda_adv_edit")

    ms = events(launch, iters=max(iters, 50))
    need = 4 * c * (n + len(got))
    rate = need / (ms * 1e-3)
    return {"rows": n, "boxes": k, "voxels": int(len(keys)), "rows_in_largest_box": int(counts.max().item()), "rows_out": int(len(got)),
            "rows_out_numpy": int(len(want)), "rows_differing_from_numpy": int((got != want).any(1).sum()) if got.shape == want.shape else -1,
            "device_chain_ms": round(t_dev, 4), "host_route_ms": round(t_host, 4), "ratio": round(t_host / t_dev, 2), "kernels_us": round(ms * 1e3, 2),
            "algorithmic_bytes": need, "algorithmic_GBps": round(rate / 1e9, 1), "fraction_of_8TBps_roof": round(rate / HBM_ROOF, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adv_frame_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    ds = NuScenesMixUpAdvDataset.__new__(NuScenesMixUpAdvDataset)          # the two routes read the voxel geometry and the edit's settings only
    ds.point_cloud_range, ds.voxel_size, ds.grid_size = RANGE, VOXEL, ops.grid_size_xyz(RANGE, VOXEL)
    ds.pseudo_thresh, ds.adv_eps, ds.shift_coor = 0.3, 1e-3, None
    res = {"bench": "adv_frame", "device": torch.cuda.get_device_name(0)}
    for name, shape in SHAPES.items():
        res[name] = bench_shape(ds, name, shape, args.iters)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
