"""Inputs of the WaymoDataset tests (tests/test_waymo_dataset_host.py, tests/test_gpu_waymo_dataset.py):
  * the committed fixture tests/golden/waymo_dataset.npz (capture_waymo_dataset.py) written back to a processed-data tree;
  * tanh_tie_free / tanh_fp64 / ulp_distance: the fp64 criterion of the frame kernel's intensity and the capture's own condition
    for asking bit equality with it;
  * a mini Waymo tree in the wire format of a stock OpenPCDet preparation: ImageSets, two sequences of four frames with their
    info pickles and [n, 6] .npy frames.  A frame has about 2 000 points and three kinds of labelled boxes: six Vehicles, a
    Pedestrian and a Cyclist, plus one `unknown` object.  The KITTI evaluator takes one score threshold per ground truth, so a
    precision curve reaches all 41 recall samples (and an AP of 100 is possible at all) only with 41 or more ground truths:
    the eight frames carry 48 Vehicles.  Every box is axis-parallel (heading 0), so a box and its copy overlap exactly, and
    the boxes move from frame to frame by more than their width, so no object of one frame touches a box of another.  Each
    box holds 12 known points outside the no-label zones, the first Vehicle 4 more inside one (NLZ flag 1), the last Vehicle
    none at all; the random points keep clear of every box by 1 m and a sixth of them lie in a no-label zone."""
import os
import pickle

import numpy as np

from toda_amd.pcdet.config import AttrDict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "waymo_dataset.npz")
TAG = "waymo_processed_data_v0_5_0"
CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]
RANGE = [-25.6, -25.6, -2.0, 25.6, 25.6, 4.0]
SEQUENCES = ["segment-1000000000000000001_with_camera_labels", "segment-2000000000000000002_with_camera_labels"]
MISSING = "segment-3000000000000000003_with_camera_labels"
FRAMES_PER_SEQUENCE = 4
N_FREE, N_IN_BOX, N_NLZ_IN_FIRST = 1900, 12, 4


def load_golden():
    return dict(np.load(GOLDEN))


# ---- the intensity criterion
def tanh_fp64(x):
    """(float)tanh((double)x): the fp64 routine rounded once."""
    with np.errstate(all="ignore"):
        return np.tanh(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def tanh_tie_free(x):
    """True where the fp64 tanh of the fp32 value lies farther than 2^-40 (relative) from every midpoint between two fp32
    values: there every fp64 tanh routine that is good to a few fp64 ulps rounds to the same fp32.  Zeros, NaN, infinities and
    values whose fp64 tanh is exactly +-1 have one answer and pass."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        v = np.tanh(x.astype(np.float64))
        near = v.astype(np.float32)
        ok = np.ones(x.shape, bool)
        for other in (np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))):
            mid = (near.astype(np.float64) + other.astype(np.float64)) / 2
            ok &= np.abs(v - mid) / np.abs(v) > 2.0 ** -40
    return ok | ~np.isfinite(x) | (x == 0) | (np.abs(v) == 1.0)


def ulp_distance(a, b):
    """Distance in fp32 ulps between two finite fp32 arrays (0 for equal values, +0 and -0 included)."""
    def ordered(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def random_intensity(rng, n):
    """n tie-free intensities with the spread of the sensor's: most below 1, a tail into the saturation of tanh."""
    x = np.exp(rng.normal(-1.5, 1.5, 2 * n + 16)).astype(np.float32)
    x = x[tanh_tie_free(x)]
    assert len(x) >= n
    return x[:n]


def random_frame(rng, n, c_in=6, nlz=(-1.0, 0.0, 1.0)):
    """[n, c_in] fp32 rows: x y z, a tie-free intensity, elongation, an NLZ flag drawn from `nlz`, further columns random."""
    rows = rng.uniform(-70, 70, (n, c_in)).astype(np.float32)
    rows[:, 2] = rng.uniform(-2, 4, n)
    rows[:, 3] = random_intensity(rng, n)
    rows[:, 4] = rng.uniform(0, 1.5, n)
    rows[:, 5] = rng.choice(np.asarray(nlz, np.float32), n)
    return np.ascontiguousarray(rows)


def host_route(rows, use_nlz=True):
    """The reference's three numpy statements on a copy of the rows: [n', 5] fp32."""
    point_features = rows.copy()
    points_all, nlz_flag = point_features[:, 0:5], point_features[:, 5]
    if use_nlz:
        points_all = points_all[nlz_flag == -1]
    points_all[:, 3] = np.tanh(points_all[:, 3])
    return points_all


# ---- the fixture as files
def write_golden_tree(root, gold):
    """The fixture's two frames and its infos as one sequence under root / TAG; returns the sequence's name."""
    seq = str(gold["sequence"])
    (root / TAG / seq).mkdir(parents=True)
    (root / "ImageSets").mkdir()
    for split in ("train", "val"):
        (root / "ImageSets" / f"{split}.txt").write_text(seq + ".tfrecord\n")
    infos = []
    for k in range(int(gold["n_infos"])):
        np.save(str(root / TAG / seq / ("%04d.npy" % k)), gold[f"frame{k % 2}"])
        info = {"point_cloud": {"lidar_sequence": seq, "sample_idx": k, "num_features": 5}, "frame_id": f"{seq}_{k:03d}"}
        if k == 0:
            info["annos"] = {"name": gold["anno_name"].copy(), "difficulty": gold["anno_difficulty"].copy(), "gt_boxes_lidar": gold["anno_boxes"].copy(),
                             "num_points_in_gt": gold["anno_num_points"].copy()}
        infos.append(info)
    with open(root / TAG / seq / f"{seq}.pkl", "wb") as f:
        pickle.dump(infos, f)
    return seq


# ---- the mini tree
def frame_boxes(k):
    """[9, 7] fp32 boxes (x y z dx dy dz heading), names and difficulties of frame k (0 .. 7 over both sequences)."""
    vehicles = [[x, y + 2.5 * k, 0.0, 4.2, 1.9, 1.6, 0.0] for x in (-18.0, 2.0, 17.0) for y in (-22.0, 0.0)]
    boxes = np.array(vehicles + [[9.0, -2.0 + k, 0.1, 0.8, 0.7, 1.8, 0.0], [-8.0, -4.0 + k, 0.0, 1.8, 0.7, 1.7, 0.0],
                                 [-22.5, 21.0, 0.5, 1.0, 1.0, 2.5, 0.0]], np.float32)
    return boxes, np.array(["Vehicle"] * 6 + ["Pedestrian", "Cyclist", "unknown"]), np.array([1, 2, 1, 1, 2, 2, 1, 2, 1], np.int64)


def points_in_boxes_count(k):
    """num_points_in_gt of frame k: the known points outside the no-label zones."""
    counts = np.full(9, N_IN_BOX, np.int64)
    counts[5] = 0
    return counts


def frame_rows(k):
    """[n, 6] fp32 rows of frame k: the free points, then the boxes' points."""
    rng = np.random.default_rng(300 + k)
    boxes = frame_boxes(k)[0].astype(np.float64)
    free = np.stack([rng.uniform(-25, 25, 3 * N_FREE), rng.uniform(-25, 25, 3 * N_FREE), rng.uniform(-1.5, 3.0, 3 * N_FREE)], 1)
    clear = np.ones(len(free), bool)
    for b in boxes:
        clear &= ~(np.abs(free - b[:3]) <= b[3:6] / 2 + 1.0).all(1)
    free = free[clear][:N_FREE]
    assert len(free) == N_FREE
    nlz = [rng.choice([-1.0, 0.0, 1.0], N_FREE, p=[5 / 6, 1 / 12, 1 / 12])]
    inside = []
    for i, b in enumerate(boxes):
        if i == 5:
            continue
        n = N_IN_BOX + (N_NLZ_IN_FIRST if i == 0 else 0)
        inside.append(b[:3] + rng.uniform(-0.4, 0.4, (n, 3)) * b[3:6] / 2)
        nlz.append(np.array([-1.0] * N_IN_BOX + [1.0] * (n - N_IN_BOX)))
    xyz = np.concatenate([free] + inside, 0)
    rows = np.concatenate([xyz, np.zeros((len(xyz), 2)), np.concatenate(nlz)[:, None]], 1).astype(np.float32)
    rows[:, 3] = random_intensity(rng, len(rows))
    rows[:, 4] = rng.uniform(0, 1.5, len(rows))
    return np.ascontiguousarray(rows)


def write_tree(data_path, other_channel=None):
    """The mini tree under data_path: ImageSets/train.txt names both sequences and one that is not on disk, val.txt the second
    sequence.  other_channel: the .npy frames go under data_path / other_channel instead of the processed-data directory."""
    (data_path / "ImageSets").mkdir(parents=True)
    (data_path / "ImageSets" / "train.txt").write_text("".join(s + ".tfrecord\n" for s in (SEQUENCES[0], MISSING, SEQUENCES[1])))
    (data_path / "ImageSets" / "val.txt").write_text(SEQUENCES[1] + ".tfrecord\n")
    frames_root = data_path / other_channel if other_channel else data_path / TAG
    for s, seq in enumerate(SEQUENCES):
        (data_path / TAG / seq).mkdir(parents=True)
        (frames_root / seq).mkdir(parents=True, exist_ok=True)
        infos = []
        for idx in range(FRAMES_PER_SEQUENCE):
            k = s * FRAMES_PER_SEQUENCE + idx
            np.save(str(frames_root / seq / ("%04d.npy" % idx)), frame_rows(k))
            boxes, names, difficulty = frame_boxes(k)
            infos.append({"point_cloud": {"num_features": 5, "lidar_sequence": seq, "sample_idx": idx}, "frame_id": f"{seq}_{idx:03d}",
                          "metadata": {"context_name": seq, "timestamp_micros": 1_550_000_000_000_000 + 100_000 * k},
                          "annos": {"name": names, "difficulty": difficulty, "gt_boxes_lidar": boxes, "dimensions": boxes[:, 3:6].copy(),
                                    "location": boxes[:, 0:3].copy(), "heading_angles": boxes[:, 6].copy(), "obj_ids": np.array([f"o{k}_{i}" for i in range(len(boxes))]),
                                    "tracking_difficulty": difficulty.copy(), "num_points_in_gt": points_in_boxes_count(k)}})
        with open(data_path / TAG / seq / f"{seq}.pkl", "wb") as f:
            pickle.dump(infos, f)
    return data_path


def all_infos(data_path):
    """Every frame's info of the tree in list order (what create_waymo_infos leaves as <tag>_infos_train.pkl)."""
    infos = []
    for seq in SEQUENCES:
        with open(data_path / TAG / seq / f"{seq}.pkl", "rb") as f:
            infos.extend(pickle.load(f))
    return infos


def dataset_cfg(data_path, **extra):
    cfg = {"DATASET": "WaymoDataset", "DATA_PATH": str(data_path), "PROCESSED_DATA_TAG": TAG, "POINT_CLOUD_RANGE": RANGE,
           "DATA_SPLIT": {"train": "train", "test": "val"}, "SAMPLED_INTERVAL": {"train": 1, "test": 1}, "FILTER_EMPTY_BOXES_FOR_TRAIN": True,
           "DISABLE_NLZ_FLAG_ON_POINTS": False,
           "POINT_FEATURE_ENCODING": {"encoding_type": "absolute_coordinates_encoding", "used_feature_list": ["x", "y", "z", "intensity", "elongation"],
                                      "src_feature_list": ["x", "y", "z", "intensity", "elongation"]},
           "DATA_PROCESSOR": [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
                              {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}},
                              {"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.1, 0.1, 0.15], "MAX_POINTS_PER_VOXEL": 5,
                               "MAX_NUMBER_OF_VOXELS": {"train": 60000, "test": 60000}}]}
    cfg.update(extra)
    return AttrDict(cfg)
