"""The mini KITTI tree of tests/kitti_dataset_cases.py dressed for KittiMixUpAdvDataset: infos of its three labelled frames in one
pickle, a labelled-split file and hand-written pseudo infos (tests/test_kitti_mixup_adv_host.py, tests/test_gpu_kitti_mixup_adv.py)."""
import pickle

import numpy as np

from tests import kitti_dataset_cases as K
from toda_amd.pcdet.datasets.kitti.kitti_dataset import KittiDataset

CLASSES = ["Car"]
SHIFT = [0.0, 0.0, 1.6]
FRAMES = ["000000", "000001", "000002"]
INFOS = "kitti_infos_trainval.pkl"
VOXEL = np.array([0.05, 0.05, 0.1], np.float32)
RANGE = [0, -40, -3, 70.4, 40, 1]
GRAD = np.array([30.0, -20.0, 10.0], np.float32)            # the stored gradient of every voxel of the hand-written pseudo infos
EXTRA = np.array([[30.0, 20.0, -0.9, 4.0, 1.8, 1.6, 0.3]], np.float32)         # a pseudo box in free space


def cfg(root, **extra):
    base = dict(DATASET="KittiMixUpAdvDataset", SHIFT_COOR=SHIFT, INFO_PATH={"train": [INFOS], "test": [INFOS]},
                DATA_SPLIT={"train": "train", "test": "val"})
    base.update(extra)
    return K.dataset_cfg(root, **base)


def frame_voxels(points):
    """(z, y, x) cells of the voxels the shifted rows of a frame occupy inside RANGE."""
    lo, hi = np.array(RANGE[:3], np.float32), np.array(RANGE[3:], np.float32)
    xyz = points[:, :3] + np.array(SHIFT, np.float32)
    cell = np.floor((xyz - lo) / VOXEL)
    grid = np.round((hi.astype(np.float64) - lo) / VOXEL).astype(np.int64)
    inside = ((cell >= 0) & (cell < grid)).all(1)
    return np.unique(cell[inside].astype(np.int32)[:, ::-1], axis=0)


def write(root, gold, listed=((1, "000001"),)):
    """The tree, the infos of all three labelled frames (host only: no point counts), the split file with `listed`
    (index, frame id) lines and pseudo.pkl: every frame's own objects as pseudo boxes, a little off, plus EXTRA; scores 0.9 / 0.25 /
    0.15 in turn; the frame's own voxels, all with the gradient GRAD."""
    K.write_tree(root, gold)
    ds = KittiDataset(K.dataset_cfg(root), ["Car", "Pedestrian", "Cyclist"], training=False, root_path=root)
    ds.set_split("train")
    infos = ds.get_infos(has_label=True, count_inside_pts=False, sample_id_list=FRAMES)
    with open(root / INFOS, "wb") as f:
        pickle.dump(infos, f)
    write_split(root, listed)
    rng = np.random.default_rng(23)
    pseudo = []
    for info in infos:
        p = {k: v for k, v in info.items() if k != "annos"}
        own = info["annos"]["gt_boxes_lidar"].astype(np.float32)
        boxes = np.concatenate([own + rng.normal(0, 0.03, own.shape).astype(np.float32), EXTRA], 0)
        boxes[0] = own[0]                                           # the Car that holds the known points, exactly
        p["gt_boxes"], p["gt_names"] = boxes, np.array(["Car"] * len(boxes))
        p["p_score"] = np.array([0.9, 0.25, 0.15], np.float32)[np.arange(len(boxes)) % 3]
        pts = np.fromfile(str(root / "training" / "velodyne" / f"{info['point_cloud']['lidar_idx']}.bin"), np.float32).reshape(-1, 4)
        p["p_voxel_coords"] = frame_voxels(pts)
        p["p_voxel_perturb"] = np.tile(GRAD, (len(p["p_voxel_coords"]), 1))
        pseudo.append(p)
    with open(root / "pseudo.pkl", "wb") as f:
        pickle.dump(pseudo, f)
    return root


def write_split(root, listed, name="train_0.01_1.txt"):
    (root / "ImageSets" / name).write_text("".join(f"{frame} {index}\n" for index, frame in listed))
