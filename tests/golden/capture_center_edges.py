#!/usr/bin/env python
"""Capture the edge cases of CenterHead target assignment from the REFERENCE's own Python (build container only, CPU).

    python tests/golden/capture_center_edges.py
writes tests/golden/center_edges.npz: for every case of tests/center_edge_cases.ASSIGN_CASES the gt boxes, the settings
[H, W, code, NUM_MAX_OBJS, MIN_RADIUS, heads] and, per head, what the reference's CenterHead.assign_targets(gt, (H, W))
returns (heat-map, target boxes, inds, masks).  pcdet/models/dense_heads/center_head.py is loaded by path
(capture_reference.setup()); the head is built on capture_reference.HEAD_CFG with the case's overrides.
Only inputs, settings and outputs are stored - no reference source.  The file is byte-stable: seeds, no time stamps.
"""
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import capture_reference as CR  # noqa: E402
from capture_reference import EasyDict  # noqa: E402
from tests import center_edge_cases as E  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def capture(L, case):
    c = E.ASSIGN_CASES[case]
    cfg = EasyDict(CR.HEAD_CFG)
    for k, v in E.head_cfg(case).items():
        cfg[k] = v
    if c["code"] > 8:
        cfg.SEPARATE_HEAD_CFG.HEAD_ORDER = ["center", "center_z", "dim", "rot", "vel"]
        cfg.SEPARATE_HEAD_CFG.HEAD_DICT["vel"] = dict(out_channels=c["code"] - 8, num_conv=2)
    pc_range, vs, grid = E.assign_geometry(case)
    head = L["center_head"].CenterHead(cfg, 24, 3, CR.CLASSES, grid, pc_range, vs, predict_boxes_when_training=False)
    gt = E.assign_gt(case)
    td = head.assign_targets(torch.from_numpy(gt.copy()), feature_map_size=(c["h"], c["w"]))     # (it writes into its argument)
    out = {f"{case}.gt": gt, f"{case}.settings": np.array([c["h"], c["w"], c["code"], c["max_objs"], c["min_radius"], len(c["heads"])], np.int64)}
    for i in range(len(c["heads"])):
        out[f"{case}.heatmap{i}"] = td["heatmaps"][i].numpy()
        out[f"{case}.target_boxes{i}"] = td["target_boxes"][i].numpy()
        out[f"{case}.inds{i}"] = td["inds"][i].numpy()
        out[f"{case}.masks{i}"] = td["masks"][i].numpy()
        print(case, i, "hm", tuple(out[f"{case}.heatmap{i}"].shape), "slots", out[f"{case}.masks{i}"].sum(1).tolist(),
              "cells == 1:", int((out[f"{case}.heatmap{i}"] == 1).sum()))
    return out


def save_stable(path, arrays):
    """np.savez_compressed with a fixed member date, so that the same arrays give the same bytes."""
    import io

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    L = CR.setup()
    arrays = {}
    for case in E.ASSIGN_CASES:
        arrays.update(capture(L, case))
    path = os.path.join(OUT, "center_edges.npz")
    save_stable(path, arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
