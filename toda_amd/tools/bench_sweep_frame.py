#!/usr/bin/env python
"""Timing of the per-sample point work of the sweep datasets (NuScenesDataset, LyftDataset):
    python -m toda_amd.tools.bench_sweep_frame --dataset {nuscenes,lyft} [--out profiles/<dataset>_frame_bench.json]
A synthetic sample written to a temporary directory, key frame + sweeps with rigid matrices whose translations are metres:
    nuscenes   10 files x 34 720 rows (a nuScenes LiDAR_TOP sweep's size), SHIFT_COOR [0, 0, 1.8], entry point toda_sweeps_merge
    lyft       5 files x 69 120 rows (an ASSUMPTION about a Lyft 64-beam LIDAR_TOP sweep), one file with trailing bytes, entry
               point toda_sweeps_merge_rect
  * the device chain of get_lidar_with_sweeps - the files read into one host buffer, one H2D copy, the merge kernel, the stable
    compaction (its row-count read included) - against get_lidar_with_sweeps_host, the reference's numpy route (per sweep:
    boolean index, transpose, vstack with ones, float64 dot, concatenations), followed by the shift and the H2D copy of the
    merged cloud.  Wall time, device idle at both ends, the same files (in the page cache) for both.
  * the merge kernel alone with HIP events; its rate at 20 bytes in + 24 bytes out per row as a fraction of the 8 TB/s HBM roof.
    At ~346 000 rows the kernel moves 15 MB and lasts a few microseconds, so that figure is mostly the wrapper's launch pace
    (output allocation and flag zeroing included); the kernel is therefore also timed on 16 x 1 048 576 rows (738 MB, past the
    256 MiB Infinity Cache) through the C entry point with buffers allocated once.
Prints one JSON line and writes it to --out.  No ratio is asked of the chain: the baseline is the reference's algorithm."""
import argparse
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from toda_amd import ops  # noqa: E402
from toda_amd.pcdet.datasets.lyft.lyft_dataset import LyftDataset  # noqa: E402
from toda_amd.pcdet.datasets.nuscenes.nuscenes_dataset import NuScenesDataset  # noqa: E402
from toda_amd.tools.bench_local_aug import HBM_ROOF, events, wall  # noqa: E402

BYTES_PER_ROW = 20 + 24
LARGE_SWEEPS, LARGE_ROWS = 16, 1 << 20
# per dataset: class, ops wrapper and C entry point (nuScenes' own take one radius), files, rows per file, largest range, rings,
# file suffix, bytes after the rows of file 2, yaw / translation / time lag per sweep index, shift, extra fields of the JSON line
WORKLOADS = {
    "nuscenes": dict(cls=NuScenesDataset, op="sweeps_merge", files=10, rows=34_720, reach=60.0, rings=32, suffix=".pcd.bin", tail=b"",
                     yaw=0.002, step=(0.45, 0.03, 0.002), lag=0.05, shift=np.array([0.0, 0.0, 1.8], np.float32), extra={}),
    "lyft": dict(cls=LyftDataset, op="sweeps_merge_rect", files=5, rows=69_120, reach=80.0, rings=64, suffix=".bin", tail=b"\x00" * 12,
                 yaw=0.004, step=(1.8, 0.06, 0.004), lag=0.2, shift=None,
                 extra={"assumed_shape": "5 files x 69 120 rows: an assumption about a Lyft 64-beam LIDAR_TOP sweep"}),
}


def make_sample(root, w, seed=0):
    """w["files"] files under root and the info that lists all but the first as sweeps."""
    rng = np.random.default_rng(seed)
    n, sweeps = w["rows"], []
    for k in range(w["files"]):
        theta, r = rng.uniform(-np.pi, np.pi, n), 0.5 + w["reach"] * rng.uniform(0, 1, n) ** 1.5         # ~1 % inside the ego rectangle
        rows = np.stack([r * np.cos(theta), r * np.sin(theta), rng.uniform(-3.0, 2.0, n), rng.uniform(0, 255, n),
                         rng.integers(0, w["rings"], n)], 1).astype(np.float32)
        with open(root / f"{k}{w['suffix']}", "wb") as f:
            f.write(rows.tobytes() + (w["tail"] if k == 2 else b""))
        if k:
            yaw = w["yaw"] * k
            m = np.eye(4)
            m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
            m[:3, 3] = [s * k for s in w["step"]]
            sweeps.append({"lidar_path": f"{k}{w['suffix']}", "transform_matrix": m, "time_lag": w["lag"] * k})
    return {"lidar_path": f"0{w['suffix']}", "token": "bench", "sweeps": sweeps}


def radii(w):
    """The radius arguments of the workload's own wrapper and entry point: one for the square, two for the rectangle."""
    sides = w["cls"].EGO_HALF_SIDES
    return sides if w["op"] == "sweeps_merge_rect" else sides[:1]


def large_kernel_ms(w):
    """The C entry point on LARGE_SWEEPS x LARGE_ROWS rows, every sweep with a matrix and the ego cut, HIP events over 50 launches."""
    from toda_amd import lib as L
    name = "toda_" + w["op"]
    entry = getattr(L.load(), name)
    n = LARGE_SWEEPS * LARGE_ROWS
    rows = torch.rand((n, 5), dtype=torch.float32, device="cuda") * 100.0 - 50.0
    out, flags = torch.empty_like(rows), torch.empty((n,), dtype=torch.int32, device="cuda")
    m = np.eye(4)[:3]
    off, mats = L.host_i32([k * LARGE_ROWS for k in range(LARGE_SWEEPS + 1)]), L.host_f64(np.tile(m.reshape(-1), LARGE_SWEEPS) * 0.999)
    ones, lags = L.host_i32([1] * LARGE_SWEEPS), L.host_f64([0.05 * k for k in range(LARGE_SWEEPS)])
    shift = L.host_f32(w["shift"]) if w["shift"] is not None else None

    def launch():
        L.check(entry(L.ptr(rows), n, LARGE_SWEEPS, L.hptr(off), L.hptr(mats), L.hptr(ones), L.hptr(ones), L.hptr(lags), *radii(w),
                      L.hptr(shift) if shift is not None else None, L.ptr(out), L.ptr(flags), L.stream()), name)

    return events(launch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", choices=sorted(WORKLOADS), required=True)
    ap.add_argument("--out", default=None, help="default: profiles/<dataset>_frame_bench.json")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    w, shift = WORKLOADS[args.dataset], WORKLOADS[args.dataset]["shift"]
    out_path = args.out if args.out is not None else os.path.join(ROOT, "profiles", f"{args.dataset}_frame_bench.json")
    with tempfile.TemporaryDirectory() as tmp:
        ds = w["cls"].__new__(w["cls"])          # the two routes read root_path and infos only
        ds.root_path, ds.infos = Path(tmp), [make_sample(Path(tmp), w)]

        def device_route():
            return ds.get_lidar_with_sweeps(0, w["files"], shift=shift)

        def host_route():
            points = ds.get_lidar_with_sweeps_host(0, w["files"])
            if shift is not None:
                points[:, 0:3] += shift
            return torch.from_numpy(points).cuda()

        t_dev, t_host = wall(device_route, args.iters), wall(host_route, args.iters)      # wall() seeds numpy alike: the same draw
        np.random.seed(0)
        got = device_route().cpu().numpy()
        np.random.seed(0)
        want = host_route().cpu().numpy()
        np.random.seed(0)
        paths, mats, lags, ego = ds._sweep_table(ds.infos[0], w["files"])
        rows, offsets = ds.read_rows(paths)
    dev = torch.from_numpy(rows).cuda()
    ms_kernel = events(lambda: getattr(ops, w["op"])(dev, offsets, mats, lags, ego, *radii(w), shift=shift))
    rate = len(rows) * BYTES_PER_ROW / (ms_kernel * 1e-3)
    ms_large = large_kernel_ms(w)
    rate_large = LARGE_SWEEPS * LARGE_ROWS * BYTES_PER_ROW / (ms_large * 1e-3)
    res = {"bench": f"{args.dataset}_frame", "device": torch.cuda.get_device_name(0), "files": w["files"], "rows": int(len(rows)), "rows_kept": int(got.shape[0]),
           "rows_kept_numpy": int(want.shape[0]), "rows_differing_from_numpy": int((got != want).any(1).sum()) if got.shape == want.shape else -1,
           **w["extra"],
           w["op"]: {"device_chain_ms": round(t_dev, 4), "numpy_route_ms": round(t_host, 4), "ratio": round(t_host / t_dev, 2)},
           w["op"] + "_kernel": {"us_with_output_allocation_and_flag_zeroing": round(ms_kernel * 1e3, 2), "bytes_per_row": BYTES_PER_ROW,
                                 "algorithmic_GBps": round(rate / 1e9, 1), "fraction_of_8TBps_roof": round(rate / HBM_ROOF, 4)},
           w["op"] + "_kernel_large": {"sweeps": LARGE_SWEEPS, "rows": LARGE_SWEEPS * LARGE_ROWS, "us": round(ms_large * 1e3, 2),
                                       "algorithmic_GBps": round(rate_large / 1e9, 1), "fraction_of_8TBps_roof": round(rate_large / HBM_ROOF, 4)}}
    line = json.dumps(res)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
