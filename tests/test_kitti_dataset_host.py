"""KittiDataset, host side: calibration, label and box arithmetic against the reference's outputs in
tests/golden/kitti_dataset.npz (capture_kitti_dataset.py), and the file-level behaviour on a mini KITTI tree.  No GPU.

Tolerances: the conversions are fp32 numpy as the reference's, so a few fp32 ulp at the magnitudes involved - 1e-5 m on
metres (coordinates below 100 m: ulp 7.6e-6), 1e-3 px on pixels (image-sized values, below 2^11 px: ulp 1.2e-4)."""
import pickle

import numpy as np
import pytest
import torch

from tests import kitti_dataset_cases as cases
from toda_amd.pcdet.datasets import __all__ as registry
from toda_amd.pcdet.datasets.dataset import DatasetTemplate
from toda_amd.pcdet.datasets.kitti.kitti_dataset import KittiDataset, png_image_shape
from toda_amd.pcdet.utils import box_utils, calibration_kitti, common_utils, object3d_kitti

TOL_M, TOL_PX = 1e-5, 1e-3
CLASSES = ["Car", "Pedestrian", "Cyclist"]


@pytest.fixture(scope="module")
def gold():
    return cases.load_golden()


@pytest.fixture(scope="module")
def tree(tmp_path_factory, gold):
    return cases.write_tree(tmp_path_factory.mktemp("kitti"), gold)


def test_registry_and_calibration_file(tmp_path, gold):
    assert registry["KittiDataset"] is KittiDataset
    path = tmp_path / "calib.txt"
    path.write_text(str(gold["calib_text"]))
    calib = calibration_kitti.Calibration(path)
    for key, attr in (("P2", "P2"), ("R0", "R0"), ("Tr_velo2cam", "V2C")):
        got = getattr(calib, attr)
        assert got.dtype == np.float32 and np.array_equal(got, gold[key])
    assert calib.fu == gold["P2"][0, 0] and calib.cv == gold["P2"][1, 2] and calib.tx == gold["P2"][0, 3] / -gold["P2"][0, 0]
    m, p2 = calib.fov_matrices()
    assert m.shape == (4, 3) and m.dtype == np.float32 and m.flags.c_contiguous and np.array_equal(m, gold["lidar_to_rect_matrix"])
    assert p2.shape == (3, 4) and np.array_equal(p2, gold["P2"])


def test_point_maps_match_the_reference(gold):
    calib = cases.golden_calib(gold)
    rect = calib.lidar_to_rect(gold["points"][:, :3])
    assert rect.dtype == np.float32 and np.abs(rect - gold["rect"]).max() <= TOL_M
    img, depth = calib.rect_to_img(gold["rect"])
    assert img.dtype == np.float32 and np.abs(img - gold["img"]).max() <= TOL_PX
    assert np.abs(depth - gold["depth"]).max() <= TOL_M
    back = calib.rect_to_lidar(gold["rect"][:256])
    assert np.abs(back - gold["rect_to_lidar"]).max() <= TOL_M
    assert np.abs(back - gold["points"][:256, :3]).max() <= 1e-4          # the round trip itself: an fp32 inverse
    img2, depth2 = calib.lidar_to_img(gold["points"][:256, :3])
    assert np.abs(img2 - gold["lidar_to_img"]).max() <= TOL_PX and np.abs(depth2 - gold["lidar_to_img_depth"]).max() <= TOL_M
    flags = KittiDataset.get_fov_flag(gold["rect"], gold["image_shape"], calib)
    assert np.array_equal(flags[~gold["borderline"]], gold["fov_flags"][~gold["borderline"]])


def test_box_conversions_match_the_reference(gold):
    calib = cases.golden_calib(gold)
    cam = box_utils.boxes3d_lidar_to_kitti_camera(gold["boxes_lidar"], calib)
    assert cam.shape == (16, 7) and np.abs(cam - gold["boxes_camera"]).max() <= TOL_M
    back = box_utils.boxes3d_kitti_camera_to_lidar(gold["boxes_camera"], calib)
    assert np.abs(back - gold["boxes_lidar_back"]).max() <= TOL_M
    assert np.abs(back[:, :6] - gold["boxes_lidar"][:, :6]).max() <= 1e-4
    for flag, key in ((True, "corners_camera"), (False, "corners_camera_center")):
        corners = box_utils.boxes3d_to_corners3d_kitti_camera(gold["boxes_camera"], bottom_center=flag)
        assert corners.dtype == np.float32 and corners.shape == (16, 8, 3) and np.abs(corners - gold[key]).max() <= TOL_M
    free = box_utils.boxes3d_kitti_camera_to_imageboxes(gold["boxes_camera"], calib)
    assert np.abs(free - gold["image_boxes"]).max() <= TOL_PX
    clipped = box_utils.boxes3d_kitti_camera_to_imageboxes(gold["boxes_camera"], calib, image_shape=gold["image_shape"])
    assert np.abs(clipped - gold["image_boxes_clipped"]).max() <= TOL_PX
    assert clipped[:, 0::2].max() <= 1241 and clipped[:, 1::2].max() <= 374 and clipped.min() >= 0 and (clipped != free).any()
    boxes, corner_px = calib.corners3d_to_img_boxes(gold["corners_camera"])
    assert np.abs(boxes - gold["img_boxes_from_corners"]).max() <= TOL_PX
    assert corner_px.shape == (16, 8, 2)
    alpha = -np.arctan2(-gold["boxes_lidar"][:, 1], gold["boxes_lidar"][:, 0]) + cam[:, 6]
    assert np.abs(alpha - gold["alpha"]).max() <= 1e-5
    before = gold["boxes_lidar"].copy()
    box_utils.boxes3d_lidar_to_kitti_camera(before, calib)
    assert np.array_equal(before, gold["boxes_lidar"])                  # the conversions leave their argument alone


def test_label_parsing_levels_and_dontcare_drop(tmp_path, gold):
    path = tmp_path / "label.txt"
    path.write_text("\n".join(str(s) for s in gold["label_lines"]) + "\n")
    objs = object3d_kitti.get_objects_from_label(path)
    assert len(objs) == 8
    assert [o.cls_type for o in objs] == [str(s) for s in gold["label_cls_type"]]
    assert [o.cls_id for o in objs] == list(gold["label_cls_id"])
    for attr, key in (("truncation", "label_truncation"), ("occlusion", "label_occlusion"), ("alpha", "label_alpha"), ("ry", "label_ry"),
                      ("score", "label_score"), ("dis_to_cam", "label_dis_to_cam")):
        assert np.array_equal(np.array([getattr(o, attr) for o in objs]), gold[key]), attr
    assert np.array_equal(np.stack([o.box2d for o in objs]), gold["label_box2d"]) and objs[0].box2d.dtype == np.float32
    assert np.array_equal(np.array([[o.h, o.w, o.l] for o in objs]), gold["label_hwl"])
    assert np.array_equal(np.stack([o.loc for o in objs]), gold["label_loc"])
    assert [o.level for o in objs] == list(gold["label_level"]) and sorted(set(gold["label_level"])) == [-1, 0, 1, 2]
    assert [o.level_str for o in objs] == [str(s) for s in gold["label_level_str"]]
    assert np.abs(np.stack([o.generate_corners3d() for o in objs[:6]]) - gold["label_corners3d"]).max() <= 1e-12
    annos = {"name": np.array([o.cls_type for o in objs]), "bbox": np.stack([o.box2d for o in objs]), "score": np.array([o.score for o in objs])}
    kept = common_utils.drop_info_with_name(annos, "DontCare")
    assert list(kept["name"]) == [str(s) for s in gold["label_cls_type"][:6]] and kept["bbox"].shape == (6, 4) and kept["score"][5] == 0.87


def test_png_header_gives_the_shape(tmp_path):
    path = tmp_path / "a.png"
    path.write_bytes(cases.tiny_png(375, 1242))
    shape = png_image_shape(path)
    assert shape.dtype == np.int32 and shape.tolist() == [375, 1242]
    path.write_bytes(b"not a png at all, just twenty-four bytes+")
    with pytest.raises(ValueError):
        png_image_shape(path)


def test_split_files_and_infos_are_found(tree, gold):
    ds = KittiDataset(cases.dataset_cfg(tree), CLASSES, training=False, root_path=tree)
    assert ds.split == "val" and ds.sample_id_list == ["000002"] and ds.root_split_path == tree / "training"
    assert len(ds) == 0 and ds.kitti_infos == []                          # no pickle yet
    assert ds.on_device                                                   # FOV crop on the device: the loader takes no workers
    ds.set_split("test")
    assert ds.root_split_path == tree / "testing" and ds.sample_id_list == ["000000"]
    ds.set_split("train")
    assert ds.sample_id_list == ["000000", "000001"]
    assert ds.get_image_shape("000001").tolist() == [375, 1242]
    assert ds.get_lidar("000000").shape[1] == 4
    assert [o.cls_type for o in ds.get_label("000000")] == [f[0] for f in cases.FRAMES["000000"]] + ["DontCare"]
    assert np.array_equal(ds.get_calib("000000").P2, gold["P2"])
    plane = ds.get_road_plane("000000")
    assert plane.shape == (4,) and plane[1] < 0 and abs(np.linalg.norm(plane[:3]) - 1) < 1e-12
    assert ds.get_road_plane("000001") is None
    ds.set_split("nope")
    assert ds.sample_id_list is None
    infos = [{"point_cloud": {"lidar_idx": "000000"}}, {"point_cloud": {"lidar_idx": "000001"}}]
    with open(tree / "kitti_infos_val.pkl", "wb") as f:
        pickle.dump(infos, f)
    try:
        ds2 = KittiDataset(cases.dataset_cfg(tree), CLASSES, training=False, root_path=tree)
        assert len(ds2) == 2
        ds2.merge_all_iters_to_one_epoch(merge=True, epochs=5)
        assert len(ds2) == 10
        assert ds2.evaluation([], CLASSES) == (None, {})                   # infos without annos: nothing to score
    finally:
        (tree / "kitti_infos_val.pkl").unlink()
    assert not KittiDataset(cases.dataset_cfg(tree, FOV_POINTS_ONLY=False), CLASSES, training=False, root_path=tree).on_device


def test_prediction_dicts_and_result_files(tree, tmp_path, gold):
    ds = KittiDataset(cases.dataset_cfg(tree, SHIFT_COOR=[0.0, 0.0, 1.6]), CLASSES, training=False, root_path=tree)
    calib = cases.golden_calib(gold)
    lidar = gold["boxes_lidar"][1:4].copy()
    shifted = lidar.copy()
    shifted[:, 2] += 1.6
    batch = {"frame_id": ["000007", "000008"], "calib": [calib, calib], "image_shape": np.stack([gold["image_shape"]] * 2)}
    preds = [{"pred_boxes": torch.from_numpy(shifted), "pred_scores": torch.tensor([0.9, 0.5, 0.25]), "pred_labels": torch.tensor([1, 3, 2])},
             {"pred_boxes": torch.zeros((0, 7)), "pred_scores": torch.zeros(0), "pred_labels": torch.zeros(0, dtype=torch.long)}]
    annos = ds.generate_prediction_dicts(batch, preds, CLASSES, output_path=tmp_path)
    a, empty = annos
    assert list(a["name"]) == ["Car", "Cyclist", "Pedestrian"] and a["frame_id"] == "000007"
    assert np.abs(a["boxes_lidar"] - lidar).max() <= 1e-6                  # SHIFT_COOR undone
    assert np.abs(a["location"] - gold["boxes_camera"][1:4, 0:3]).max() <= 2e-5
    assert np.abs(a["dimensions"] - gold["boxes_camera"][1:4, 3:6]).max() <= TOL_M          # l, h, w
    assert np.abs(a["rotation_y"] - gold["boxes_camera"][1:4, 6]).max() <= TOL_M
    assert np.abs(a["alpha"] - gold["alpha"][1:4]).max() <= 1e-5
    assert np.abs(a["bbox"] - gold["image_boxes_clipped"][1:4]).max() <= 2e-3
    assert np.array_equal(a["score"], np.array([0.9, 0.5, 0.25], np.float32)) and a["truncated"].shape == (3,) and a["occluded"].shape == (3,)
    lines = (tmp_path / "000007.txt").read_text().splitlines()
    assert len(lines) == 3
    first = lines[0].split(" ")
    assert first[0] == "Car" and first[1:3] == ["-1", "-1"] and len(first) == 16 and all(len(v.split(".")[1]) == 4 for v in first[3:])
    vals = np.array([float(v) for v in first[3:]])
    l, h, w = a["dimensions"][0]
    want = np.concatenate([[a["alpha"][0]], a["bbox"][0], [h, w, l], a["location"][0], [a["rotation_y"][0], 0.9]])
    assert np.abs(vals - want).max() <= 5.1e-5                               # %.4f
    assert empty["frame_id"] == "000008" and empty["bbox"].shape == (0, 4) and empty["boxes_lidar"].shape == (0, 7) and len(empty["name"]) == 0
    assert (tmp_path / "000008.txt").read_text() == ""


@pytest.mark.parametrize("item", ["images", "depth_maps", "calib_matricies"])
def test_caddn_items_are_refused(tree, item):
    with pytest.raises(NotImplementedError, match="CaDDN"):
        KittiDataset(cases.dataset_cfg(tree, GET_ITEM_LIST=["points", item]), CLASSES, training=False, root_path=tree)


def test_collate_passes_calib_and_image_shape(gold):
    calib = cases.golden_calib(gold)
    sample = lambda k: {"points": np.zeros((k, 4), np.float32), "gt_boxes": np.zeros((k, 8), np.float32), "gt_boxes2d": np.ones((k, 4), np.float32),
                        "frame_id": f"{k:06d}", "calib": calib, "image_shape": gold["image_shape"], "use_lead_xyz": True}
    batch = DatasetTemplate.collate_batch([sample(2), sample(3)])
    assert isinstance(batch["calib"], list) and batch["calib"][1] is calib
    assert batch["image_shape"].shape == (2, 2) and batch["image_shape"].dtype == np.int32
    assert batch["gt_boxes"].shape == (2, 3, 8) and batch["gt_boxes2d"].shape == (2, 3, 4) and batch["gt_boxes2d"][0, 2].sum() == 0
    assert batch["points"].shape == (5, 5) and batch["batch_size"] == 2


def test_road_plane_lowers_sampled_boxes(gold):
    from toda_amd.pcdet.datasets.augmentor.database_sampler import DataBaseSampler
    calib = cases.golden_calib(gold)
    plane = np.array([0.0, -1.0, 0.0, 1.65])                                 # the road 1.65 m below the camera
    boxes = gold["boxes_lidar"][:4].astype(np.float64).copy()
    moved, shift = DataBaseSampler.put_boxes_on_road_planes(boxes.copy(), plane, calib)
    bottom_cam = calib.lidar_to_rect((moved[:, :3] - np.array([0, 0, 0.5]) * moved[:, 5:6]).astype(np.float32))
    assert np.abs(bottom_cam[:, 1] - 1.65).max() < 2e-3                       # bottom faces on the plane (R0 / V2C tilt the z axis a little)
    assert np.allclose(moved[:, 2] + shift, boxes[:, 2]) and np.array_equal(moved[:, [0, 1, 3, 4, 5, 6]], boxes[:, [0, 1, 3, 4, 5, 6]])
