#!/usr/bin/env python
"""Timing of LyftDataset's per-sample point work:
    python -m toda_amd.tools.bench_lyft_frame [--out profiles/lyft_frame_bench.json]
A synthetic sample of 5 files x 69 120 rows (an ASSUMPTION about a Lyft 64-beam LIDAR_TOP sweep; key frame + 4 sweeps, rigid
matrices with translations of metres, one file with trailing bytes) written to a temporary directory:
  * the device chain of LyftDataset.get_lidar_with_sweeps - the files read into one host buffer, one H2D copy,
    toda_sweeps_merge_rect, the stable compaction (its row-count read included) - against get_lidar_with_sweeps_host, the
    reference's numpy route (per sweep: boolean index, transpose, vstack with ones, float64 dot, concatenations), followed by the
    H2D copy of the merged cloud.  Wall time, device idle at both ends, the same files (in the page cache) for both.
  * the merge kernel alone with HIP events; its rate at 20 bytes in + 24 bytes out per row as a fraction of the 8 TB/s HBM roof.
    At 345 600 rows the kernel moves 15 MB and lasts a few microseconds, so that figure is mostly the wrapper's launch pace
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
from toda_amd.pcdet.datasets.lyft.lyft_dataset import EGO_RADIUS_X, EGO_RADIUS_Y, LyftDataset  # noqa: E402
from toda_amd.tools.bench_local_aug import HBM_ROOF, events, wall  # noqa: E402

N_FILES, N_ROWS = 5, 69_120
BYTES_PER_ROW = 20 + 24
LARGE_SWEEPS, LARGE_ROWS = 16, 1 << 20


def make_sample(root, seed=0):
    """N_FILES files under root and the info that lists the last N_FILES - 1 as sweeps."""
    rng = np.random.default_rng(seed)
    sweeps = []
    for k in range(N_FILES):
        theta, r = rng.uniform(-np.pi, np.pi, N_ROWS), 0.5 + 80.0 * rng.uniform(0, 1, N_ROWS) ** 1.5         # ~1 % inside the ego rectangle
        rows = np.stack([r * np.cos(theta), r * np.sin(theta), rng.uniform(-3.0, 2.0, N_ROWS), rng.uniform(0, 255, N_ROWS),
                         rng.integers(0, 64, N_ROWS)], 1).astype(np.float32)
        with open(root / f"{k}.bin", "wb") as f:
            f.write(rows.tobytes() + (b"\x00" * 12 if k == 2 else b""))
        if k:
            yaw = 0.004 * k
            m = np.eye(4)
            m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
            m[:3, 3] = [1.8 * k, 0.06 * k, 0.004 * k]
            sweeps.append({"lidar_path": f"{k}.bin", "transform_matrix": m, "time_lag": 0.2 * k})
    return {"lidar_path": "0.bin", "token": "bench", "sweeps": sweeps}


def large_kernel_ms():
    """toda_sweeps_merge_rect on LARGE_SWEEPS x LARGE_ROWS rows, every sweep with a matrix and the ego cut, HIP events over 50 launches."""
    from toda_amd import lib as L
    lib = L.load()
    n = LARGE_SWEEPS * LARGE_ROWS
    rows = torch.rand((n, 5), dtype=torch.float32, device="cuda") * 100.0 - 50.0
    out, flags = torch.empty_like(rows), torch.empty((n,), dtype=torch.int32, device="cuda")
    m = np.eye(4)[:3]
    off, mats = L.host_i32([k * LARGE_ROWS for k in range(LARGE_SWEEPS + 1)]), L.host_f64(np.tile(m.reshape(-1), LARGE_SWEEPS) * 0.999)
    ones, lags = L.host_i32([1] * LARGE_SWEEPS), L.host_f64([0.05 * k for k in range(LARGE_SWEEPS)])

    def launch():
        L.check(lib.toda_sweeps_merge_rect(L.ptr(rows), n, LARGE_SWEEPS, L.hptr(off), L.hptr(mats), L.hptr(ones), L.hptr(ones), L.hptr(lags), EGO_RADIUS_X,
                                           EGO_RADIUS_Y, None, L.ptr(out), L.ptr(flags), L.stream()), "toda_sweeps_merge_rect")

    return events(launch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lyft_frame_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ds = LyftDataset.__new__(LyftDataset)          # the two routes read root_path and infos only
        ds.root_path, ds.infos = Path(tmp), [make_sample(Path(tmp))]

        def device_route():
            return ds.get_lidar_with_sweeps(0, N_FILES)

        def host_route():
            return torch.from_numpy(ds.get_lidar_with_sweeps_host(0, N_FILES)).cuda()

        t_dev, t_host = wall(device_route, args.iters), wall(host_route, args.iters)      # wall() seeds numpy alike: the same draw
        np.random.seed(0)
        got = device_route().cpu().numpy()
        np.random.seed(0)
        want = host_route().cpu().numpy()
        np.random.seed(0)
        paths, mats, lags, ego = ds._sweep_table(ds.infos[0], N_FILES)
        rows, offsets = ds.read_rows(paths)
    dev = torch.from_numpy(rows).cuda()
    ms_kernel = events(lambda: ops.sweeps_merge_rect(dev, offsets, mats, lags, ego, EGO_RADIUS_X, EGO_RADIUS_Y))
    rate = len(rows) * BYTES_PER_ROW / (ms_kernel * 1e-3)
    ms_large = large_kernel_ms()
    rate_large = LARGE_SWEEPS * LARGE_ROWS * BYTES_PER_ROW / (ms_large * 1e-3)
    res = {"bench": "lyft_frame", "device": torch.cuda.get_device_name(0), "files": N_FILES, "rows": int(len(rows)), "rows_kept": int(got.shape[0]),
           "rows_kept_numpy": int(want.shape[0]), "rows_differing_from_numpy": int((got != want).any(1).sum()) if got.shape == want.shape else -1,
           "assumed_shape": "5 files x 69 120 rows: an assumption about a Lyft 64-beam LIDAR_TOP sweep",
           "sweeps_merge_rect": {"device_chain_ms": round(t_dev, 4), "numpy_route_ms": round(t_host, 4), "ratio": round(t_host / t_dev, 2)},
           "sweeps_merge_rect_kernel": {"us_with_output_allocation_and_flag_zeroing": round(ms_kernel * 1e3, 2), "bytes_per_row": BYTES_PER_ROW,
                                        "algorithmic_GBps": round(rate / 1e9, 1), "fraction_of_8TBps_roof": round(rate / HBM_ROOF, 4)},
           "sweeps_merge_rect_kernel_large": {"sweeps": LARGE_SWEEPS, "rows": LARGE_SWEEPS * LARGE_ROWS, "us": round(ms_large * 1e3, 2),
                                              "algorithmic_GBps": round(rate_large / 1e9, 1), "fraction_of_8TBps_roof": round(rate_large / HBM_ROOF, 4)}}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
