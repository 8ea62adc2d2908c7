#!/usr/bin/env python
"""Capture the WaymoDataset fixture from the REFERENCE's own Python (build container only).

    python tests/golden/capture_waymo_dataset.py        # writes tests/golden/waymo_dataset.npz

The reference's pcdet/datasets/waymo/waymo_dataset.py is loaded by path under the alias-package scheme of capture_reference.py
(the dataset template and tqdm are stubs, SharedArray and roiaware_pool3d_utils are those capture_reference sets up; waymo_utils,
which imports TensorFlow, is never reached) and its include_waymo_data, get_lidar, __getitem__ and generate_prediction_dicts are
called as they are.  Nothing of the reference is copied: the file holds inputs made up here and the reference's outputs for them.

Inputs: one sequence of N_INFOS frames whose .npy files alternate between two made-up [n, 6] tables (x, y, z, intensity,
elongation, NLZ flag; the elongation column holds a row id, so the reference's output names the rows it kept):
    frame0 300 rows, NLZ flags drawn from -1, 0, 1      frame1 257 rows, the same, the first rows with the edge intensities
The intensities are filtered by waymo_dataset_cases.tanh_tie_free: the fp64 tanh of each lies farther than 2^-40 (relative) from
every midpoint between two fp32 values, so (float)tanh((double)x) has one answer and a test may ask a kernel for it bit for bit.
Frame 0 carries annotations with two `unknown` objects and two boxes without points.

Outputs: get_lidar with the NLZ filter on and off, the frame ids the info list holds after SAMPLED_INTERVAL 1, 2 and 3, names and
boxes of __getitem__ in training (FILTER_EMPTY_BOXES_FOR_TRAIN) and in test mode, generate_prediction_dicts for a frame with
detections and one without, and tanh_ulp_ref: the largest distance in fp32 ulps between the reference's intensity column (numpy's
fp32 tanh of this machine) and the fp64 criterion."""
import os
import pickle
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import capture_reference as CR  # noqa: E402
from tests import waymo_dataset_cases as cases  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SEQ = "segment-4242424242424242424_with_camera_labels"
N_INFOS = 7
CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]
EDGE_INTENSITY = [0.0, -0.0, 1e-40, 9.0, 9.1, 100.0, -0.75, 0.5, 1.0, 3.0e4]


class Template:
    def __init__(self, dataset_cfg=None, class_names=None, training=True, root_path=None, logger=None):
        self.dataset_cfg, self.class_names, self.training, self.root_path, self.logger = dataset_cfg, class_names, training, root_path, logger
        self._merge_all_iters_to_one_epoch = False

    @property
    def mode(self):
        return "train" if self.training else "test"

    def prepare_data(self, data_dict):          # the frame as __getitem__ hands it to the template
        return data_dict


class Quiet:
    def info(self, *a, **k):
        pass


def setup():
    CR.ALIAS = "pcdet"
    CR.setup()
    A = CR.ALIAS
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    sys.modules["tqdm"] = tq
    CR._pkg(f"{A}.datasets.waymo")
    mod = types.ModuleType(f"{A}.datasets.dataset")
    mod.DatasetTemplate = Template
    sys.modules[f"{A}.datasets.dataset"] = mod
    sys.modules[f"{A}.datasets"].dataset = mod
    return CR._load(f"{A}.datasets.waymo.waymo_dataset", "pcdet/datasets/waymo/waymo_dataset.py")


def make_frames(seed):
    rng = np.random.default_rng(seed)
    frames = []
    for k, n in enumerate((300, 257)):
        rows = cases.random_frame(rng, n)
        if k == 1:
            rows[:len(EDGE_INTENSITY), 3] = np.array(EDGE_INTENSITY, np.float32)
            rows[:len(EDGE_INTENSITY), 5] = -1.0
        rows[:, 4] = np.arange(1000 * k, 1000 * k + n, dtype=np.float32)
        assert cases.tanh_tie_free(rows[:, 3]).all()
        frames.append(rows)
    return frames


def make_annos(seed):
    rng = np.random.default_rng(seed + 1)
    names = np.array(["Vehicle", "unknown", "Pedestrian", "Vehicle", "Cyclist", "unknown", "Vehicle", "Sign"])
    n = len(names)
    boxes = np.concatenate([rng.uniform(-60, 60, (n, 2)), rng.uniform(-1, 2, (n, 1)), rng.uniform(0.5, 5, (n, 3)), rng.uniform(-3, 3, (n, 1))], 1).astype(np.float32)
    return {"name": names, "difficulty": np.array([1, 1, 2, 2, 1, 2, 1, 1], np.int64), "gt_boxes_lidar": boxes,
            "num_points_in_gt": np.array([25, 3, 0, 7, 1, 0, 0, 4], np.int64)}


def dataset(W, root, training, interval=1, **extra):
    cfg = CR.EasyDict(PROCESSED_DATA_TAG=cases.TAG, DATA_SPLIT={"train": "train", "test": "val"}, SAMPLED_INTERVAL={"train": interval, "test": interval}, **extra)
    return W.WaymoDataset(dataset_cfg=cfg, class_names=CLASSES, training=training, root_path=root, logger=Quiet())


def capture(W, seed):
    frames, annos = make_frames(seed), make_annos(seed)
    out = {"seed": np.array(seed), "sequence": np.array(SEQ), "n_infos": np.array(N_INFOS), "frame0": frames[0], "frame1": frames[1],
           "anno_name": annos["name"], "anno_difficulty": annos["difficulty"], "anno_boxes": annos["gt_boxes_lidar"], "anno_num_points": annos["num_points_in_gt"]}
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        assert cases.write_golden_tree(root, out) == SEQ
        worst = 0
        for tag, extra in (("nlz", {}), ("all", {"DISABLE_NLZ_FLAG_ON_POINTS": True})):
            ds = dataset(W, root, False, **extra)
            for k in range(2):
                points = ds.get_lidar(SEQ, k)
                assert points.dtype == np.float32 and points.shape[1] == 5
                src = frames[k][np.isin(frames[k][:, 4], points[:, 4])]
                assert len(src) == len(points)
                worst = max(worst, int(cases.ulp_distance(points[:, 3], cases.tanh_fp64(src[:, 3])).max()))
                out[f"points_{tag}_{k}"] = points
        assert len(out["points_nlz_0"]) < len(out["points_all_0"]) == 300                                   # the filter acted
        out["tanh_ulp_ref"] = np.array(worst)
        for interval in (1, 2, 3):
            out[f"frame_ids_interval_{interval}"] = np.array([info["frame_id"] for info in dataset(W, root, True, interval=interval).infos])
        for tag, training in (("train", True), ("test", False)):
            item = dataset(W, root, training, FILTER_EMPTY_BOXES_FOR_TRAIN=True)[0]
            assert "num_points_in_gt" not in item and item["metadata"] == item["frame_id"]
            out[f"item_{tag}_names"], out[f"item_{tag}_boxes"] = np.array(item["gt_names"]), item["gt_boxes"]
        assert "unknown" not in out["item_train_names"] and len(out["item_train_names"]) < len(out["item_test_names"]) < len(annos["name"])
    return out


def capture_predictions(W, seed):
    rng = np.random.default_rng(seed + 2)
    boxes = np.concatenate([rng.uniform(-70, 70, (6, 3)), rng.uniform(0.5, 5, (6, 3)), rng.uniform(-3, 3, (6, 1))], 1).astype(np.float32)
    scores, labels = rng.uniform(0.1, 1, 6).astype(np.float32), rng.integers(1, len(CLASSES) + 1, 6).astype(np.int64)
    batch = {"frame_id": [f"{SEQ}_000", f"{SEQ}_001"], "metadata": [{"context_name": SEQ, "timestamp_micros": 1}, f"{SEQ}_001"]}
    preds = [{"pred_boxes": torch.from_numpy(boxes.copy()), "pred_scores": torch.from_numpy(scores), "pred_labels": torch.from_numpy(labels)},
             {"pred_boxes": torch.zeros((0, 7)), "pred_scores": torch.zeros(0), "pred_labels": torch.zeros(0, dtype=torch.long)}]
    full, empty = W.WaymoDataset.generate_prediction_dicts(batch, preds, CLASSES)
    assert full["frame_id"] == f"{SEQ}_000" and full["metadata"] == batch["metadata"][0] and empty["metadata"] == f"{SEQ}_001"
    assert sorted(full) == sorted(empty) == ["boxes_lidar", "frame_id", "metadata", "name", "score"]
    assert empty["boxes_lidar"].shape == (0, 7) and empty["name"].shape == (0,) and empty["name"].dtype == np.float64
    return {"pred_boxes": boxes, "pred_scores": scores, "pred_labels": labels, "pred_name": np.array(full["name"]), "pred_score": full["score"],
            "pred_boxes_lidar": full["boxes_lidar"]}


def main():
    W = setup()
    seed = 20261019
    out = capture(W, seed)
    out.update(capture_predictions(W, seed))
    path = os.path.join(OUT, "waymo_dataset.npz")
    np.savez_compressed(path, **out)
    print("waymo_dataset.npz:", os.path.getsize(path), "bytes; tanh_ulp_ref", int(out["tanh_ulp_ref"]))


if __name__ == "__main__":
    main()
