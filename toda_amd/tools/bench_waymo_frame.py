#!/usr/bin/env python
"""Timing of WaymoDataset's per-frame point work:
    python -m toda_amd.tools.bench_waymo_frame [--out profiles/waymo_frame_bench.json]
A synthetic processed frame of 180 000 rows x 6 columns (one Waymo frame's size; a sixth of the rows inside a no-label zone)
written as .npy to a temporary directory:
  * the device chain of WaymoDataset.get_lidar - np.load, one H2D copy, toda_waymo_frame and, with the NLZ filter on, the stable
    compaction (its row-count read included) - against get_lidar_host, the reference's numpy statements (boolean index, fp32
    tanh), followed by the H2D copy of the result.  Wall time, device idle at both ends, the same file (in the page cache) for
    both, with the NLZ filter on and off (DISABLE_NLZ_FLAG_ON_POINTS).
  * the frame kernel alone with HIP events; its rate at 24 bytes in + 20 + 4 bytes out per row as a fraction of the 8 TB/s HBM
    roof.  At 180 000 rows the kernel moves 8.6 MB and lasts a few microseconds, so that figure is mostly the wrapper's launch pace
    (output allocation included); the kernel is therefore also timed on 16 777 216 rows (805 MB, past the 256 MiB Infinity Cache)
    through the C entry point with buffers allocated once.
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
from toda_amd.pcdet.datasets.waymo.waymo_dataset import WaymoDataset  # noqa: E402
from toda_amd.tools.bench_local_aug import HBM_ROOF, events, wall  # noqa: E402

N_ROWS, C_IN = 180_000, 6
BYTES_PER_ROW = 4 * C_IN + 20 + 4
LARGE_ROWS = 1 << 24
SEQUENCE = "segment-bench_with_camera_labels"


def make_frame(root, seed=0):
    rng = np.random.default_rng(seed)
    r, theta = 75.0 * rng.uniform(0, 1, N_ROWS) ** 0.75, rng.uniform(-np.pi, np.pi, N_ROWS)
    rows = np.stack([r * np.cos(theta), r * np.sin(theta), rng.uniform(-2.0, 4.0, N_ROWS), np.exp(rng.normal(-1.5, 1.5, N_ROWS)),
                     rng.uniform(0, 1.5, N_ROWS), rng.choice([-1.0, 0.0, 1.0], N_ROWS, p=[5 / 6, 1 / 12, 1 / 12])], 1).astype(np.float32)
    (root / SEQUENCE).mkdir()
    np.save(str(root / SEQUENCE / "0000.npy"), rows)
    return rows


def dataset(root, use_nlz):
    ds = WaymoDataset.__new__(WaymoDataset)                    # the two routes read frame_path and use_nlz only
    ds.frame_path, ds.use_nlz = root, use_nlz
    return ds


def large_kernel_ms():
    """toda_waymo_frame on LARGE_ROWS rows with the NLZ test on, HIP events over 50 launches."""
    from toda_amd import lib as L
    lib = L.load()
    rows = torch.rand((LARGE_ROWS, C_IN), dtype=torch.float32, device="cuda") * 4.0 - 2.0
    out, flags = torch.empty((LARGE_ROWS, 5), dtype=torch.float32, device="cuda"), torch.empty((LARGE_ROWS,), dtype=torch.int32, device="cuda")

    def launch():
        L.check(lib.toda_waymo_frame(L.ptr(rows), LARGE_ROWS, C_IN, 1, L.ptr(out), L.ptr(flags), L.stream()), "toda_waymo_frame")

    return events(launch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waymo_frame_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    chains = {}
    with tempfile.TemporaryDirectory() as tmp:
        rows = make_frame(Path(tmp))
        for tag, use_nlz in (("nlz_filter_on", True), ("nlz_filter_off", False)):
            ds = dataset(Path(tmp), use_nlz)
            t_dev = wall(lambda: ds.get_lidar(SEQUENCE, 0), args.iters)
            t_host = wall(lambda: torch.from_numpy(ds.get_lidar_host(SEQUENCE, 0)).cuda(), args.iters)
            got, want = ds.get_lidar(SEQUENCE, 0).cpu().numpy(), ds.get_lidar_host(SEQUENCE, 0)
            same_rows = got.shape == want.shape and bool((got[:, [0, 1, 2, 4]] == want[:, [0, 1, 2, 4]]).all())
            ulps = np.abs(got[:, 3].view(np.int32).astype(np.int64) - want[:, 3].view(np.int32).astype(np.int64)) if same_rows else np.array([-1])
            chains[tag] = {"device_chain_ms": round(t_dev, 4), "numpy_route_ms": round(t_host, 4), "ratio": round(t_host / t_dev, 2),
                           "rows_kept": int(got.shape[0]), "same_rows_as_numpy": same_rows, "intensity_max_ulp_from_numpy_fp32_tanh": int(ulps.max())}
    dev = torch.from_numpy(rows).cuda()
    ms_kernel = events(lambda: ops.waymo_frame(dev, use_nlz=True))
    rate = N_ROWS * BYTES_PER_ROW / (ms_kernel * 1e-3)
    ms_large = large_kernel_ms()
    rate_large = LARGE_ROWS * BYTES_PER_ROW / (ms_large * 1e-3)
    res = {"bench": "waymo_frame", "device": torch.cuda.get_device_name(0), "rows": N_ROWS, "columns": C_IN, "get_lidar": chains,
           "waymo_frame_kernel": {"us_with_output_allocation": round(ms_kernel * 1e3, 2), "bytes_per_row": BYTES_PER_ROW,
                                  "algorithmic_GBps": round(rate / 1e9, 1), "fraction_of_8TBps_roof": round(rate / HBM_ROOF, 4)},
           "waymo_frame_kernel_large": {"rows": LARGE_ROWS, "megabytes": round(LARGE_ROWS * BYTES_PER_ROW / 1e6, 1), "us": round(ms_large * 1e3, 2),
                                        "algorithmic_GBps": round(rate_large / 1e9, 1), "fraction_of_8TBps_roof": round(rate_large / HBM_ROOF, 4)}}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
