"""Inputs of the NuScenesDataset tests (tests/test_nuscenes_dataset_host.py, tests/test_gpu_nuscenes_dataset.py):
  * the committed fixture tests/golden/nuscenes_dataset.npz (capture_nuscenes_dataset.py) written back to .pcd.bin files with
    the infos that produced it;
  * tie_free: the capture's own condition for asking bit equality of an fp64 product rounded to fp32;
  * a mini nuScenes tree: VERSION/samples/LIDAR_TOP, VERSION/sweeps/LIDAR_TOP and info pickles in the wire format of a stock
    OpenPCDet preparation.  Three training frames and one validation frame, each the key frame and two sweeps, 15 cars, a
    pedestrian and a truck.  The KITTI evaluator takes one score threshold per ground truth, so a precision curve reaches all
    41 recall samples (and an AP of 100 is possible at all) only with 41 or more ground truths: the training frames carry 45
    cars.  Every box is axis-parallel (heading 0), so a box and its copy overlap exactly.  Each box holds 12 known points of the
    key frame, the first car 6 more from each sweep; the random points keep clear of every box by 1 m."""
import os
import pickle

import numpy as np

from toda_amd.pcdet.config import AttrDict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nuscenes_dataset.npz")
VERSION = "v1.0-mini"
CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]
RANGE = [-25.6, -25.6, -5.0, 25.6, 25.6, 3.0]
N_KEY, N_SWEEP, N_EGO, N_IN_BOX, N_IN_FIRST = 1500, 700, 20, 12, 6
TREE_SWEEPS = 3                 # MAX_SWEEPS of the mini tree: every frame lists exactly two sweeps, so all of them are drawn


def load_golden():
    return dict(np.load(GOLDEN))


# ---- the fixture as files
def write_golden_files(root, gold):
    """The fixture's six files under root; returns the info list of the capture's two samples."""
    k = 0
    while f"file{k}" in gold:
        gold[f"file{k}"].tofile(str(root / f"f{k}.pcd.bin"))
        k += 1
    infos = []
    for s in range(2):
        sweeps = [{"lidar_path": f"f{int(f)}.pcd.bin", "transform_matrix": None if m < 0 else gold["matrices"][int(m)], "time_lag": float(lag)}
                  for f, m, lag in zip(gold[f"sample{s}_files"], gold[f"sample{s}_matrix"], gold[f"sample{s}_lag"])]
        infos.append({"lidar_path": f"f{int(gold[f'sample{s}_key'])}.pcd.bin", "token": f"tok{s}", "sweeps": sweeps})
    return infos


def golden_table(gold, sample, max_sweeps):
    """The sweep table of one captured run in the drawn order: (raw rows [n, 5], offsets, matrices, lags, drop_ego)."""
    picks = gold[f"picks_{sample}_{max_sweeps}"]
    files = [int(gold[f"sample{sample}_key"])] + [int(gold[f"sample{sample}_files"][p]) for p in picks]
    mats = [None] + [None if gold[f"sample{sample}_matrix"][p] < 0 else gold["matrices"][int(gold[f"sample{sample}_matrix"][p])] for p in picks]
    lags = [0.0] + [float(gold[f"sample{sample}_lag"][p]) for p in picks]
    rows = np.concatenate([gold[f"file{f}"] for f in files], 0)
    offsets = np.concatenate([[0], np.cumsum([len(gold[f"file{f}"]) for f in files])]).tolist()
    return rows, offsets, mats, lags, [False] + [True] * len(picks)


def tie_free(rows, matrix):
    """True where the fp64 sums ((x m0 + y m1) + z m2) + m3 of all three output coordinates lie farther than 2^-40 (relative)
    from a midpoint between two fp32 values: there every summation order or fused form rounds to the same fp32."""
    x, y, z = (rows[:, c].astype(np.float64) for c in range(3))
    ok = np.ones(len(rows), bool)
    for row in np.asarray(matrix, np.float64)[:3]:
        v = ((x * row[0] + y * row[1]) + z * row[2]) + row[3]
        near = v.astype(np.float32)
        for other in (np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))):
            mid = (near.astype(np.float64) + other.astype(np.float64)) / 2
            with np.errstate(all="ignore"):
                ok &= np.abs(v - mid) / np.abs(v) > 2.0 ** -40
    return ok


# ---- the mini tree
def frame_boxes(k):
    """[17, 9] fp32 boxes (x y z dx dy dz heading vx vy) and names of frame k; the pedestrian's velocity is NaN."""
    cars = [[x, y + 0.3 * k, -1.0, 4.0, 1.8, 1.6, 0.0, 0.5 * k, 0.0] for x in (-20.0, -12.0, 8.0, 16.0, 22.0) for y in (-14.0, -3.0, 10.0)]
    boxes = np.array(cars + [[4.0, 6.0 + 0.3 * k, -0.9, 0.8, 0.6, 1.75, 0.0, np.nan, np.nan], [-5.0, 18.0, -0.5, 7.0, 2.5, 3.0, 0.0, 1.0, -1.0]], np.float32)
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
    clear &= ~((np.abs(pts[:, 0]) < 2.0) & (np.abs(pts[:, 1]) < 2.0))          # nothing of the scene inside the ego square
    return pts[clear][:n]


def _inside(rng, box, n, frac):
    return box[:3] + rng.uniform(-frac, frac, (n, 3)) * box[3:6] / 2


def _rows(rng, xyz):
    return np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1)), rng.integers(0, 32, (len(xyz), 1))], 1).astype(np.float32)


def frame_files(k):
    """(key rows, [sweep rows] * 2) of frame k.  Sweep points of the first car are placed in the key frame's coordinates and
    carried back through the sweep's matrix, so they land well inside it (30 % of the half extents, moved by micrometres)."""
    rng = np.random.default_rng(100 + k)
    boxes = frame_boxes(k)[0].astype(np.float64)
    key = np.concatenate([_free_points(rng, N_KEY, boxes, 1.0)] + [_inside(rng, b, N_IN_BOX, 0.4) for b in boxes], 0)
    sweeps = []
    for j in range(2):
        inv = np.linalg.inv(sweep_matrix(k, j))
        in_key = np.concatenate([_free_points(rng, N_SWEEP, boxes, 1.0), _inside(rng, boxes[0], N_IN_FIRST, 0.3)], 0)
        raw = in_key @ inv[:3, :3].T + inv[:3, 3]
        ego = np.concatenate([rng.uniform(-0.95, 0.95, (N_EGO, 2)), rng.uniform(-1.5, 0.0, (N_EGO, 1))], 1)
        sweeps.append(_rows(rng, np.concatenate([raw, ego], 0)))
    return _rows(rng, key), sweeps


def write_tree(data_path, frames=(("train", (0, 1, 2)), ("val", (3,)))):
    """The mini tree under data_path / VERSION; returns that directory."""
    root = data_path / VERSION
    for sub in ("samples", "sweeps"):
        (root / sub / "LIDAR_TOP").mkdir(parents=True)
    for split, ks in frames:
        infos = []
        for k in ks:
            key, sweeps = frame_files(k)
            stem = f"n008-2018-08-01-15-16-36-0400__LIDAR_TOP__153315{k:04d}"
            key.tofile(str(root / "samples" / "LIDAR_TOP" / f"{stem}.pcd.bin"))
            entries = []
            for j, rows in enumerate(sweeps):
                rel = f"sweeps/LIDAR_TOP/{stem}_{j}.pcd.bin"
                rows.tofile(str(root / rel))
                entries.append({"lidar_path": rel, "sample_data_token": f"sd{k}{j}", "transform_matrix": sweep_matrix(k, j), "time_lag": 0.05 * (j + 1)})
            boxes, names = frame_boxes(k)
            counts = np.full(len(boxes), N_IN_BOX, np.int64)
            counts[0] += 2 * N_IN_FIRST
            infos.append({"lidar_path": f"samples/LIDAR_TOP/{stem}.pcd.bin", "cam_front_path": "", "token": f"token{k}", "sweeps": entries,
                          "gt_boxes": boxes, "gt_boxes_velocity": boxes[:, 7:9].copy(), "gt_names": names, "gt_boxes_token": np.array([f"b{k}_{i}" for i in range(len(boxes))]),
                          "num_lidar_pts": counts, "num_radar_pts": np.zeros(len(boxes), np.int64)})
        with open(root / f"nuscenes_infos_10sweeps_{split}.pkl", "wb") as f:
            pickle.dump(infos, f)
    return root


def dataset_cfg(data_path, **extra):
    cfg = {"DATASET": "NuScenesDataset", "DATA_PATH": str(data_path), "VERSION": VERSION, "MAX_SWEEPS": TREE_SWEEPS, "PRED_VELOCITY": False,
           "SET_NAN_VELOCITY_TO_ZEROS": True, "POINT_CLOUD_RANGE": RANGE, "DATA_SPLIT": {"train": "train", "test": "val"},
           "INFO_PATH": {"train": ["nuscenes_infos_10sweeps_train.pkl"], "test": ["nuscenes_infos_10sweeps_val.pkl"]},
           "POINT_FEATURE_ENCODING": {"encoding_type": "absolute_coordinates_encoding", "used_feature_list": ["x", "y", "z", "intensity", "timestamp"],
                                      "src_feature_list": ["x", "y", "z", "intensity", "timestamp"]},
           "DATA_PROCESSOR": [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
                              {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}},
                              {"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.1, 0.1, 0.2], "MAX_POINTS_PER_VOXEL": 10,
                               "MAX_NUMBER_OF_VOXELS": {"train": 60000, "test": 60000}}]}
    cfg.update(extra)
    return AttrDict(cfg)
