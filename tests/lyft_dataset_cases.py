"""Inputs of the LyftDataset tests (tests/test_lyft_dataset_host.py, tests/test_gpu_lyft_dataset.py):
  * the committed fixture tests/golden/lyft_dataset.npz (capture_lyft_dataset.py: the reference's own clouds, prediction dicts
    and get_ap values) written back to .bin files, trailing bytes included, with the infos that produced it;
  * a mini Lyft tree: VERSION/lidar/*.bin, the info pickles in the wire format of a stock OpenPCDet preparation and the three JSON
    tables under VERSION/data.  Two training frames and one validation frame, each the key frame and four sweep entries: one with
    a matrix, one without, that one once more (the reference repeats the last sweep of a short history) and one with a matrix;
    15 cars, a pedestrian and a truck per frame, axis-parallel in the LiDAR frame.  One sweep file carries 7 trailing bytes, one
    key frame 19, and one sweep of frame 1 is an empty file.  Each box holds 12 known points of the key frame, the first car 6
    more from every non-empty sweep file; the random points keep clear of every box by 1 m and of the ego rectangle.  Every sweep
    also holds points placed for the ego cut."""
import json
import os
import pickle

import numpy as np

from tests import lyft_eval_cases as E
from tests.nuscenes_dataset_cases import tie_free
from toda_amd.pcdet.config import AttrDict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lyft_dataset.npz")
VERSION = "trainval"
CLASSES = E.CLASSES
RANGE = [-25.6, -25.6, -5.0, 25.6, 25.6, 3.0]
N_KEY, N_SWEEP, N_IN_BOX, N_IN_FIRST = 1500, 500, 12, 6
TREE_SWEEPS = 5                 # MAX_SWEEPS of the mini tree: every frame lists exactly four sweeps, so all of them are drawn
TRAIN, VAL = (0, 1), (2,)

X15, ONE = np.float32(1.5), np.float32(1.0)
XB, YB = np.nextafter(X15, np.float32(0)), np.nextafter(ONE, np.float32(0))
# (x, y) placed for the ego cut and whether a SWEEP keeps the row; the key frame keeps all of them
EGO_ROWS = [((1.5, 0.5), 1), ((-1.5, -0.3), 1), ((0.5, 1.0), 1), ((0.2, -1.0), 1), ((1.5, 1.0), 1), ((XB, YB), 0), ((-XB, -YB), 0), ((XB, 0.0), 0),
            ((0.0, YB), 0), ((0.0, 0.0), 0), ((1.2, 0.4), 0), ((-1.4, -0.9), 0), ((1.2, 1.2), 1), ((np.nan, 0.1), 1), ((0.3, np.nan), 1),
            ((np.nan, np.nan), 1)]


def load_golden():
    return dict(np.load(GOLDEN))


# ---- the fixture as files
def write_golden_files(root, gold):
    """The fixture's five files under root, byte for byte; returns the info list of the capture's two samples."""
    k = 0
    while f"file{k}" in gold:
        gold[f"file{k}"].tofile(str(root / f"f{k}.bin"))
        k += 1
    infos = []
    for s in range(2):
        sweeps = [{"lidar_path": f"f{int(f)}.bin", "transform_matrix": None if m < 0 else gold["matrices"][int(m)], "time_lag": float(lag)}
                  for f, m, lag in zip(gold[f"sample{s}_files"], gold[f"sample{s}_matrix"], gold[f"sample{s}_lag"])]
        infos.append({"lidar_path": f"f{int(gold[f'sample{s}_key'])}.bin", "token": f"tok{s}", "sweeps": sweeps})
    return infos


def golden_rows(gold, f):
    """The whole rows of fixture file f as [n, 5] fp32."""
    raw = gold[f"file{f}"]
    return raw[:len(raw) // 20 * 20].view(np.float32).reshape(-1, 5)


def golden_table(gold, sample, max_sweeps):
    """The sweep table of one captured run in the drawn order: (raw rows [n, 5], offsets, matrices, lags, drop_ego)."""
    picks = gold[f"picks_{sample}_{max_sweeps}"]
    files = [int(gold[f"sample{sample}_key"])] + [int(gold[f"sample{sample}_files"][p]) for p in picks]
    mats = [None] + [None if gold[f"sample{sample}_matrix"][p] < 0 else gold["matrices"][int(gold[f"sample{sample}_matrix"][p])] for p in picks]
    lags = [0.0] + [float(gold[f"sample{sample}_lag"][p]) for p in picks]
    rows = np.concatenate([golden_rows(gold, f) for f in files], 0)
    offsets = np.concatenate([[0], np.cumsum([len(golden_rows(gold, f)) for f in files])]).tolist()
    return rows, offsets, mats, lags, [False] + [True] * len(picks)


def same_bits_nan_aware(a, b):
    """Bit equality where neither side is NaN, and NaN in the same places (a NaN's payload is no part of the contract)."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(na, nb) and np.where(na, np.float32(0), a).tobytes() == np.where(nb, np.float32(0), b).tobytes()


# ---- the mini tree
def frame_boxes(k):
    """[17, 7] fp32 boxes (x y z dx dy dz heading) and names of frame k."""
    cars = [[x, y + 0.3 * k, -1.0, 4.0, 1.8, 1.6, 0.0] for x in (-20.0, -12.0, 8.0, 16.0, 22.0) for y in (-14.0, -3.0, 10.0)]
    boxes = np.array(cars + [[4.0, 6.0 + 0.3 * k, -0.9, 0.8, 0.6, 1.75, 0.0], [-5.0, 18.0, -0.5, 7.0, 2.5, 3.0, 0.0]], np.float32)
    return boxes, np.array(["car"] * 15 + ["pedestrian", "truck"])


def sweep_matrix(k, j):
    """Sweep j of frame k into the key frame: a few centimetres and a milliradian."""
    a = 0.001 * (1 + j + k)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    m[:3, 3] = [0.05 * (j + 1), -0.02 * (k + 1), 0.01]
    return m


def _free_points(rng, n, boxes, margin):
    pts = np.stack([rng.uniform(-25, 25, 2 * n), rng.uniform(-25, 25, 2 * n), rng.uniform(-3, 1, 2 * n)], 1)
    clear = np.ones(len(pts), bool)
    for b in boxes:
        clear &= ~(np.abs(pts - b[:3]) <= b[3:6] / 2 + margin).all(1)
    clear &= ~((np.abs(pts[:, 0]) < 2.5) & (np.abs(pts[:, 1]) < 2.0))          # nothing of the scene inside or near the ego rectangle
    return pts[clear][:n]


def _inside(rng, box, n, frac):
    return box[:3] + rng.uniform(-frac, frac, (n, 3)) * box[3:6] / 2


def _rows(rng, xyz):
    return np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1)), rng.integers(0, 32, (len(xyz), 1))], 1).astype(np.float32)


def _settle(rows, matrix, keep_from):
    """Rows whose transformed coordinates are clear of every fp32 rounding midpoint (the first keep_from rows are checked, not dropped)."""
    if matrix is None:
        return rows
    ok = tie_free(rows, matrix) | np.isnan(rows[:, :3]).any(1)
    assert ok[:keep_from].all()
    return np.ascontiguousarray(rows[ok])


def frame_files(k):
    """(key rows, [rows of sweep files 0, 1, 2], matrices [m0, None, m2]) of frame k; sweep file 2 of frame 1 is empty.  Sweep points
    of the first car are placed in the key frame's coordinates and carried back through the sweep's matrix."""
    rng = np.random.default_rng(300 + k)
    boxes = frame_boxes(k)[0].astype(np.float64)
    ego = np.array([[x, y, -1.0] for (x, y), _ in EGO_ROWS], np.float32)
    key = np.concatenate([_rows(rng, np.concatenate([_inside(rng, b, N_IN_BOX, 0.4) for b in boxes], 0)), _rows(rng, ego), _rows(rng, _free_points(rng, N_KEY, boxes, 1.0))], 0)
    mats = [sweep_matrix(k, 0), None, sweep_matrix(k, 2)]
    sweeps = []
    for j, m in enumerate(mats):
        if k == 1 and j == 2:
            sweeps.append(np.zeros((0, 5), np.float32))
            continue
        in_key = _inside(rng, boxes[0], N_IN_FIRST, 0.3)
        first = in_key if m is None else in_key @ np.linalg.inv(m)[:3, :3].T + np.linalg.inv(m)[:3, 3]
        free = _free_points(rng, N_SWEEP, boxes, 1.0)
        rows = np.concatenate([_rows(rng, first), _rows(rng, ego), _rows(rng, free)], 0)
        sweeps.append(_settle(rows, m, N_IN_FIRST + len(ego)))
    return key, sweeps, mats


def world():
    """The tree's samples as lyft_eval_cases worlds (pose, ground truths, no predictions): what the JSON tables are built from."""
    rng = np.random.default_rng(41)
    out = []
    for k in TRAIN + VAL:
        boxes, names = frame_boxes(k)
        out.append({"token": f"token{k}", "pose": E.pose(rng, 0.02), "gt_boxes": boxes.astype(np.float64), "gt_names": names.tolist(),
                    "pred_boxes": np.zeros((0, 7)), "pred_names": [], "scores": np.zeros(0, np.float32)})
    return out


def write_tree(data_path, tables=True):
    """The mini tree under data_path / VERSION; returns that directory."""
    root = data_path / VERSION
    (root / "lidar").mkdir(parents=True)
    built = E.build(world())
    for split, ks in (("train", TRAIN), ("val", VAL)):
        infos = []
        for k in ks:
            key, sweeps, mats = frame_files(k)
            stem = f"host-a101_lidar1_12000000{k:02d}"
            with open(root / "lidar" / f"{stem}.bin", "wb") as f:
                f.write(key.tobytes() + (b"\x07" * 19 if k == 1 else b""))
            entries = []
            for j, (rows, m) in enumerate(zip(sweeps, mats)):
                rel = f"lidar/{stem}_{j}.bin"
                with open(root / rel, "wb") as f:
                    f.write(rows.tobytes() + (b"\x01\x02\x03\x04\x05\x06\x07" if j == 0 else b""))
                entries.append({"lidar_path": rel, "sample_data_token": f"sd{k}{j}", "transform_matrix": m, "time_lag": 0.0 if m is None else 0.1 * (j + 1)})
            entries = [entries[0], entries[1], entries[1], entries[2]]                     # the sweep without a matrix is listed twice
            boxes, names = frame_boxes(k)
            base = built["infos"][k]
            infos.append({"lidar_path": f"lidar/{stem}.bin", "token": f"token{k}", "ref_from_car": np.linalg.inv(base["ref_to_car"]),
                          "ref_to_car": base["ref_to_car"], "car_from_global": np.linalg.inv(base["car_to_global"]), "car_to_global": base["car_to_global"],
                          "timestamp": 1.5e9 + k, "sweeps": entries, "gt_boxes": boxes.astype(np.float64), "gt_boxes_velocity": np.zeros((len(boxes), 3)),
                          "gt_names": names, "gt_boxes_token": np.array([f"ann_{k}_{i}" for i in range(len(boxes))]).reshape(-1, 1)})
        with open(root / f"lyft_infos_{split}.pkl", "wb") as f:
            pickle.dump(infos, f)
    if tables:
        (root / "data").mkdir()
        for name, records in built["tables"].items():
            with open(root / "data" / f"{name}.json", "w") as f:
                json.dump(records, f)
    return root


def dataset_cfg(data_path, **extra):
    cfg = {"DATASET": "LyftDataset", "DATA_PATH": str(data_path), "VERSION": VERSION, "MAX_SWEEPS": TREE_SWEEPS, "POINT_CLOUD_RANGE": RANGE,
           "EVAL_LYFT_IOU_LIST": list(E.THRESHOLDS), "DATA_SPLIT": {"train": "train", "test": "val"},
           "INFO_PATH": {"train": ["lyft_infos_train.pkl"], "test": ["lyft_infos_val.pkl"]},
           "POINT_FEATURE_ENCODING": {"encoding_type": "absolute_coordinates_encoding", "used_feature_list": ["x", "y", "z", "intensity", "timestamp"],
                                      "src_feature_list": ["x", "y", "z", "intensity", "timestamp"]},
           "DATA_PROCESSOR": [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
                              {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}},
                              {"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.1, 0.1, 0.2], "MAX_POINTS_PER_VOXEL": 10,
                               "MAX_NUMBER_OF_VOXELS": {"train": 60000, "test": 60000}}]}
    cfg.update(extra)
    return AttrDict(cfg)
