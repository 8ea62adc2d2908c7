"""A mini KITTI tree for the KittiDataset tests (tests/test_kitti_dataset_host.py, tests/test_gpu_kitti_dataset.py), written
from the committed fixture tests/golden/kitti_dataset.npz: 3 labelled frames (train: 000000, 000001; val: 000002) and one
unlabelled (testing/000000), each with the fixture's calibration, a 375 x 1242 PNG that is a header and one empty row, and
the fixture's non-borderline points with the neighbourhood of the frame's boxes cleared and 10 known points put well inside
the first Car.  Frame 000000 has a road-plane file.  Labels are written through the project's own box conversions (which
test_kitti_dataset_host.py checks against the reference's) with the benchmark's two decimals."""
import os
import struct
import zlib

import numpy as np

from toda_amd.pcdet.config import AttrDict
from toda_amd.pcdet.utils import box_utils, calibration_kitti

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_dataset.npz")
N_KNOWN = 10
# per frame: (class, LiDAR box x y z dx dy dz heading, truncated, occluded); the first is the Car that holds the known points.
# * The KITTI evaluator takes at most one score threshold per ground truth, so a precision curve reaches all 41 recall samples
#   (and an AP of 100 is possible at all) only with 41 or more ground truths of a difficulty: every frame carries a lattice of 15
#   unoccluded Cars, 14 to 24 m ahead and more than 40 px tall (Easy), next to one Moderate or Hard Car and a Pedestrian.
# * Every heading is -pi / 2, i.e. rotation_y = 0.00 in the label: the angle then survives label -> LiDAR -> camera bit for bit and
#   the bird's-eye rectangles of a box and of its round-tripped copy are axis-parallel and a micrometre apart, which the rotated
#   overlap (the reference's included) handles exactly; at a general angle two nearly coincident rectangles are left to the signs
#   of rounded dot products.
SIDEWAYS = -np.pi / 2


def _car(x, y, z=-0.9, length=4.0, width=1.8, height=1.6):
    return [x, y, z, length, width, height, SIDEWAYS]


def _lattice(k):
    cars = [_car(14.5 + 0.5 * k, y + 0.3 * k) for y in (-7.5, -2.5, 2.5, 7.5)]
    cars += [_car(18.5 + 0.5 * k, y - 0.3 * k, length=3.9, width=1.7, height=1.5) for y in (-10.0, -5.0, 0.0, 5.0, 10.0)]
    cars += [_car(22.5 + 0.5 * k, y + 0.3 * k, length=3.8, width=1.6, height=1.5) for y in (-12.5, -7.5, -2.5, 2.5, 7.5, 12.5)]
    return [("Car", box, 0.0, 0) for box in cars]


FRAMES = {
    "000000": [("Car", _car(9.0, 1.5), 0.0, 0), ("Car", _car(35.0, -6.0, -0.8, 3.8, 1.7, 1.5), 0.0, 2)] + _lattice(0),
    "000001": [("Car", _car(9.5, -2.0, -1.0, 4.2, 1.8, 1.5), 0.0, 0), ("Pedestrian", _car(9.0, 5.5, -0.8, 0.8, 0.6, 1.75), 0.0, 0)] + _lattice(1),
    "000002": [("Car", _car(10.0, 0.5), 0.0, 0), ("Car", _car(30.0, 5.0, -0.9, 3.9, 1.6, 1.5), 0.0, 1)] + _lattice(2),
}


def extents(box):
    """World-axis extents of a box turned by -pi / 2: its length lies along y."""
    return np.array([box[4], box[3], box[5]], np.float32)


SPLITS = {"train": ["000000", "000001"], "val": ["000002"], "test": ["000000"]}
DONTCARE = "DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10"
PLANE = "# Plane\nWidth 4\nHeight 1\n-1.851372e-02 -9.998285e-01 -2.533805e-04 1.678761e+00\n"


def load_golden():
    return dict(np.load(GOLDEN))


def golden_calib(gold):
    return calibration_kitti.Calibration({"P2": gold["P2"], "R0": gold["R0"], "Tr_velo2cam": gold["Tr_velo2cam"]})


def tiny_png(height, width):
    """A PNG whose IHDR says height x width (8-bit RGB) and whose data is one empty deflate stream: enough for the header reader."""
    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(b"\x00")) + chunk(b"IEND", b"")


def known_points(box):
    """N_KNOWN points within 40 % of the half extents of an axis-parallel box: clear of every face by more than 0.2 m."""
    rng = np.random.default_rng(7)
    xyz = np.asarray(box[:3]) + rng.uniform(-0.4, 0.4, (N_KNOWN, 3)) * extents(box) / 2
    return np.concatenate([xyz, rng.uniform(0, 1, (N_KNOWN, 1))], 1).astype(np.float32)


def frame_points(gold, frame):
    """(points of the frame's .bin, bool mask of the rows the reference's field-of-view test keeps)."""
    keep = ~gold["borderline"]
    pts = gold["points"]
    for _, box, _, _ in FRAMES[frame]:
        near = (np.abs(pts[:, :3] - np.asarray(box[:3], np.float32)) <= extents(box) / 2 + 0.5).all(1)
        keep &= ~near
    known = known_points(FRAMES[frame][0][1])
    points = np.ascontiguousarray(np.concatenate([pts[keep], known], 0))
    in_fov = np.concatenate([gold["fov_flags"][keep], np.ones(N_KNOWN, bool)])       # the known points sit mid-image, 8-12 m ahead
    return points, in_fov


def label_lines(gold, frame):
    calib, shape = golden_calib(gold), gold["image_shape"]
    lines = []
    for name, box, trunc, occ in FRAMES[frame]:
        lidar = np.asarray([box], np.float32)
        cam = box_utils.boxes3d_lidar_to_kitti_camera(lidar, calib)
        bbox = box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=shape)[0]
        alpha = -np.arctan2(-lidar[0, 1], lidar[0, 0]) + cam[0, 6]
        x, y, z, l, h, w, ry = cam[0]
        lines.append("%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (name, trunc, occ, alpha, *bbox, h, w, l, x, y, z, ry))
    return lines + [DONTCARE]


def write_tree(root, gold):
    (root / "ImageSets").mkdir(parents=True)
    for split, frames in SPLITS.items():
        (root / "ImageSets" / f"{split}.txt").write_text("\n".join(frames) + "\n")
        top = root / ("testing" if split == "test" else "training")
        for sub in ("velodyne", "calib", "image_2", "label_2", "planes"):
            (top / sub).mkdir(parents=True, exist_ok=True)
        for frame in frames:
            frame_points(gold, frame)[0].tofile(str(top / "velodyne" / f"{frame}.bin"))
            (top / "calib" / f"{frame}.txt").write_text(str(gold["calib_text"]))
            (top / "image_2" / f"{frame}.png").write_bytes(tiny_png(int(gold["image_shape"][0]), int(gold["image_shape"][1])))
            if split != "test":
                (top / "label_2" / f"{frame}.txt").write_text("\n".join(label_lines(gold, frame)) + "\n")
    (root / "training" / "planes" / "000000.txt").write_text(PLANE)
    return root


def dataset_cfg(root, processors=("mask", "shuffle", "voxel"), **extra):
    steps = {"mask": {"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
             "shuffle": {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}},
             "voxel": {"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.05, 0.05, 0.1], "MAX_POINTS_PER_VOXEL": 5,
                       "MAX_NUMBER_OF_VOXELS": {"train": 16000, "test": 40000}}}
    cfg = {"DATASET": "KittiDataset", "DATA_PATH": str(root), "POINT_CLOUD_RANGE": [0, -40, -3, 70.4, 40, 1],
           "DATA_SPLIT": {"train": "train", "test": "val"},
           "INFO_PATH": {"train": ["kitti_infos_train.pkl"], "test": ["kitti_infos_val.pkl"]},
           "GET_ITEM_LIST": ["points"], "FOV_POINTS_ONLY": True,
           "POINT_FEATURE_ENCODING": {"encoding_type": "absolute_coordinates_encoding", "used_feature_list": ["x", "y", "z", "intensity"],
                                      "src_feature_list": ["x", "y", "z", "intensity"]},
           "DATA_PROCESSOR": [steps[p] for p in processors]}
    cfg.update(extra)
    return AttrDict(cfg)
