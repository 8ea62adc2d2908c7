#!/usr/bin/env python
"""Capture the KittiDataset fixture from the REFERENCE's own Python (build container only).

    python tests/golden/capture_kitti_dataset.py        # writes tests/golden/kitti_dataset.npz

The reference's pcdet/utils/calibration_kitti.py, object3d_kitti.py, box_utils.py and the static KittiDataset.get_fov_flag
of pcdet/datasets/kitti/kitti_dataset.py are loaded by path under the alias-package scheme of capture_reference.py (skimage,
the dataset template and kitti_utils are stubs: get_fov_flag reads none of them) and called as they are.  Nothing of the
reference is copied: the file holds inputs made up here and the reference's outputs for them.

Inputs: a made-up, KITTI-like calibration (fu = fv = 721.5377, image 375 x 1242, R0 and V2C turned by a few hundredths of a
radian off the identity and the axis permutation), 4096 points in x [-20, 70] y [-40, 40] z [-3, 1] without the slab
|rect_z| < 0.3 m, 16 LiDAR boxes, 8 label lines (the last two DontCare).
Outputs: lidar_to_rect / rect_to_img (fp32) and the field-of-view flags; the parsed label fields and levels; camera <->
LiDAR boxes, corners, image boxes with and without the clip, alpha.

tau_px / tau_depth: 4 x the largest difference between the reference's fp32 pixel / depth and a float64 evaluation of the
same formula on the same fp32 inputs (points, M = fp32(V2C^T . R0^T), P2); the factor 4 covers another summation order and
fused multiply-adds.  A point is borderline when its float64 pixel lies within tau_px of an image edge or its float64 depth
within tau_depth of 0.  Asserted here: at most 2 % of the points are borderline and the reference's own flags agree with
float64 on all others; the seed is advanced until that holds.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import capture_reference as CR  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
IMG_H, IMG_W = 375, 1242
N_POINTS, N_BOXES = 4096, 16

LABELS = [
    "Car 0.00 0 -1.58 587.01 173.33 614.12 200.12 1.65 1.67 3.64 -0.65 1.71 46.70 -1.59",       # 27.8 px tall: Moderate
    "Car 0.00 0 1.85 387.63 181.54 423.81 233.96 1.67 1.87 3.69 -16.53 2.39 58.49 1.57",        # Easy
    "Pedestrian 0.00 1 0.21 712.40 143.00 810.73 307.92 1.89 0.48 1.20 1.84 1.47 8.41 0.01",    # Moderate (occluded 1)
    "Cyclist 0.40 2 -1.55 676.60 163.95 688.98 193.93 1.86 0.60 2.02 4.59 1.32 45.84 -1.55",    # Hard (truncated, occluded 2)
    "Van 0.80 3 -2.44 0.00 217.12 85.92 374.00 2.47 1.59 3.26 -6.31 1.73 5.56 2.95",            # unknown level
    "Car 0.10 0 1.71 298.00 190.00 340.00 210.00 1.50 1.62 3.88 -12.54 1.64 40.11 1.40 0.87",   # 21 px: unknown level; with a score
    "DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10",
    "DontCare -1 -1 -10 511.35 174.96 527.81 187.45 -1 -1 -1 -1000 -1000 -1000 -10",
]


def setup():
    CR.ALIAS = "pcdet"
    L = CR.setup()
    A = CR.ALIAS
    sys.modules["skimage"].io = types.ModuleType("skimage.io")
    sys.modules["skimage.io"] = sys.modules["skimage"].io
    CR._pkg(f"{A}.datasets.kitti")
    for stub in (f"{A}.datasets.dataset", f"{A}.datasets.kitti.kitti_utils"):
        mod = types.ModuleType(stub)
        sys.modules[stub] = mod
        parent, _, leaf = stub.rpartition(".")
        setattr(sys.modules[parent], leaf, mod)
    sys.modules[f"{A}.datasets.dataset"].DatasetTemplate = object
    C = CR._load(f"{A}.utils.calibration_kitti", "pcdet/utils/calibration_kitti.py")
    O = CR._load(f"{A}.utils.object3d_kitti", "pcdet/utils/object3d_kitti.py")
    K = CR._load(f"{A}.datasets.kitti.kitti_dataset", "pcdet/datasets/kitti/kitti_dataset.py")
    return C, O, L["box_utils"], K


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def make_calib():
    p2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
    r0 = rot(0.011, -0.017, 0.009)
    v2c = np.concatenate([rot(-0.013, 0.021, 0.007) @ np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]]),
                          np.array([[-0.004069766], [-0.07631618], [-0.2717806]])], axis=1)
    return {"P2": p2.astype(np.float32), "P3": p2.astype(np.float32), "R0": r0.astype(np.float32), "Tr_velo2cam": v2c.astype(np.float32)}


def calib_text(calib):
    """The six lines of a KITTI calib file; %.9e round-trips fp32."""
    def line(tag, arr):
        return tag + ": " + " ".join("%.9e" % v for v in np.asarray(arr, np.float32).reshape(-1))
    eye = np.eye(3, 4, dtype=np.float32)
    return "\n".join([line("P0", eye), line("P1", eye), line("P2", calib["P2"]), line("P3", calib["P3"]), line("R0_rect", calib["R0"]),
                      line("Tr_velo_to_cam", calib["Tr_velo2cam"]), line("Tr_imu_to_velo", eye)]) + "\n"


def fp64_projection(points, calib):
    m = np.dot(calib.V2C.T, calib.R0.T).astype(np.float64)          # the fp32 matrix the reference forms, widened
    p2 = calib.P2.astype(np.float64)
    hom = np.concatenate([points[:, :3].astype(np.float64), np.ones((len(points), 1))], 1)
    rect = hom @ m
    proj = np.concatenate([rect, np.ones((len(points), 1))], 1) @ p2.T
    with np.errstate(all="ignore"):
        return proj[:, :2] / rect[:, 2:3], proj[:, 2] - p2[2, 3]


def capture_points(C, K, calib, seed):
    rng = np.random.default_rng(seed)
    raw = np.stack([rng.uniform(-20, 70, 3 * N_POINTS), rng.uniform(-40, 40, 3 * N_POINTS), rng.uniform(-3, 1, 3 * N_POINTS),
                    rng.uniform(0, 1, 3 * N_POINTS)], 1).astype(np.float32)
    rect_all = calib.lidar_to_rect(raw[:, :3])
    points = np.ascontiguousarray(raw[np.abs(rect_all[:, 2]) >= 0.3][:N_POINTS])
    assert len(points) == N_POINTS
    rect = calib.lidar_to_rect(points[:, :3])
    img, depth = calib.rect_to_img(rect)
    flags = K.KittiDataset.get_fov_flag(rect, np.array([IMG_H, IMG_W], np.int32), calib)
    assert rect.dtype == np.float32 and img.dtype == np.float32 and depth.dtype == np.float32
    img64, depth64 = fp64_projection(points, calib)
    tau_px = 4.0 * float(np.abs(img.astype(np.float64) - img64).max())
    tau_depth = 4.0 * float(np.abs(depth.astype(np.float64) - depth64).max())
    edge = np.minimum.reduce([np.abs(img64[:, 0]), np.abs(img64[:, 0] - IMG_W), np.abs(img64[:, 1]), np.abs(img64[:, 1] - IMG_H)])
    borderline = (edge <= tau_px) | (np.abs(depth64) <= tau_depth)
    flags64 = (img64[:, 0] >= 0) & (img64[:, 0] < IMG_W) & (img64[:, 1] >= 0) & (img64[:, 1] < IMG_H) & (depth64 >= 0)
    ok = borderline.mean() <= 0.02 and np.array_equal(flags[~borderline], flags64[~borderline])
    print(f"seed {seed}: tau_px {tau_px:.3e} tau_depth {tau_depth:.3e} borderline {int(borderline.sum())} in fov {int(flags.sum())} ok {ok}")
    return ok, {"points": points, "rect": rect, "img": img, "depth": depth, "fov_flags": flags, "fov_flags64": flags64, "borderline": borderline,
                "tau_px": np.array(tau_px), "tau_depth": np.array(tau_depth), "seed": np.array(seed)}


def capture_labels(O):
    objs = [O.Object3d(line) for line in LABELS]
    return {"label_lines": np.array(LABELS), "label_cls_type": np.array([o.cls_type for o in objs]),
            "label_cls_id": np.array([o.cls_id for o in objs], np.int64),
            "label_truncation": np.array([o.truncation for o in objs]), "label_occlusion": np.array([o.occlusion for o in objs]),
            "label_alpha": np.array([o.alpha for o in objs]), "label_box2d": np.stack([o.box2d for o in objs]),
            "label_hwl": np.array([[o.h, o.w, o.l] for o in objs]), "label_loc": np.stack([o.loc for o in objs]),
            "label_ry": np.array([o.ry for o in objs]), "label_score": np.array([o.score for o in objs]),
            "label_level": np.array([o.level for o in objs], np.int64), "label_level_str": np.array([o.level_str for o in objs]),
            "label_dis_to_cam": np.array([o.dis_to_cam for o in objs]),
            "label_corners3d": np.stack([o.generate_corners3d() for o in objs[:6]])}


def capture_boxes(B, calib, seed):
    rng = np.random.default_rng(seed + 1)
    k = N_BOXES
    boxes = np.stack([rng.uniform(4, 60, k), rng.uniform(-15, 15, k), rng.uniform(-1.6, -0.4, k), rng.uniform(0.6, 5, k),
                      rng.uniform(0.5, 2.2, k), rng.uniform(1.3, 2.2, k), rng.uniform(-np.pi, np.pi, k)], 1).astype(np.float32)
    boxes[0, 1], boxes[0, 0] = -14.0, 5.0        # leaves the image on the right: the clip acts
    cam = B.boxes3d_lidar_to_kitti_camera(boxes, calib)
    back = B.boxes3d_kitti_camera_to_lidar(cam, calib)
    shape = np.array([IMG_H, IMG_W], np.int32)
    out = {"boxes_lidar": boxes, "boxes_camera": cam, "boxes_lidar_back": back,
           "corners_camera": B.boxes3d_to_corners3d_kitti_camera(cam), "corners_camera_center": B.boxes3d_to_corners3d_kitti_camera(cam, bottom_center=False),
           "image_boxes": B.boxes3d_kitti_camera_to_imageboxes(cam, calib), "image_boxes_clipped": B.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=shape),
           "alpha": -np.arctan2(-boxes[:, 1], boxes[:, 0]) + cam[:, 6]}         # kitti_dataset.py generate_prediction_dicts
    corners = out["corners_camera"]
    out["img_boxes_from_corners"], out["img_corners_from_corners"] = calib.corners3d_to_img_boxes(corners)
    assert (out["image_boxes"] != out["image_boxes_clipped"]).any()
    return out


def main():
    C, O, B, K = setup()
    cd = make_calib()
    calib = C.Calibration(cd)
    seed = 20261018
    while True:
        ok, out = capture_points(C, K, calib, seed)
        if ok:
            break
        seed += 1
    out.update({"P2": cd["P2"], "R0": cd["R0"], "Tr_velo2cam": cd["Tr_velo2cam"], "calib_text": np.array(calib_text(cd)),
                "image_shape": np.array([IMG_H, IMG_W], np.int32), "lidar_to_rect_matrix": np.dot(calib.V2C.T, calib.R0.T)})
    out["rect_to_lidar"] = calib.rect_to_lidar(out["rect"][:256])
    out["lidar_to_img"], out["lidar_to_img_depth"] = calib.lidar_to_img(out["points"][:256, :3])
    out.update(capture_labels(O))
    out.update(capture_boxes(B, calib, seed))
    np.savez_compressed(os.path.join(OUT, "kitti_dataset.npz"), **out)
    print("kitti_dataset.npz:", os.path.getsize(os.path.join(OUT, "kitti_dataset.npz")), "bytes")


if __name__ == "__main__":
    main()
