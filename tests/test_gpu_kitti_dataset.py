"""KittiDataset on the MI355X: the field-of-view kernel (csrc/kitti_frame.hip) against the reference's flags
(tests/golden/kitti_dataset.npz), on an exactly representable calibration and at its shape edges, and the dataset end to end
on a mini KITTI tree: infos -> samples -> collate -> prediction dicts -> official AP.

The kernel sums in its own order and numpy's matrix product in another, so a point within tau_px of an image edge or
tau_depth of depth 0 (the fixture's bounds: 4 x the largest fp32-vs-fp64 difference of the reference's own arithmetic) may
take either the fp32 or the fp64 flag; every other point must take the reference's."""
import pickle

import numpy as np
import pytest
import torch

from tests import kitti_dataset_cases as cases
from toda_amd import ops
from toda_amd.pcdet.datasets.dataset import DatasetTemplate
from toda_amd.pcdet.datasets.kitti.kitti_dataset import KittiDataset, create_kitti_infos
from toda_amd.pcdet.utils import calibration_kitti

pytestmark = pytest.mark.gpu
CLASSES = ["Car", "Pedestrian", "Cyclist"]
SENTINEL = -7


@pytest.fixture(scope="module")
def gold():
    return cases.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_flags(points, calib, shape):
    return KittiDataset.get_fov_flag(calib.lidar_to_rect(points[:, :3]), shape, calib)


# ---- the kernel ---------------------------------------------------------------------------------------------------------
def test_flags_match_the_reference_off_the_borderline(gold):
    calib = cases.golden_calib(gold)
    m, p2 = calib.fov_matrices()
    flags = ops.points_fov_flags(dev(gold["points"]), m, p2, gold["image_shape"]).cpu().numpy()
    assert flags.dtype == np.int32 and set(np.unique(flags)) <= {0, 1}
    border = gold["borderline"]
    ref, ref64 = gold["fov_flags"].astype(np.int32), gold["fov_flags64"].astype(np.int32)
    print(f"in view {int(flags.sum())} of {len(flags)}, borderline {int(border.sum())}, differ from fp32 reference {int((flags != ref).sum())}")
    assert np.array_equal(flags[~border], ref[~border])
    assert ((flags[border] == ref[border]) | (flags[border] == ref64[border])).all()
    assert 0 < flags.sum() < len(flags)


def exact_calib():
    """Camera x = -y, y = -z, z = x of the LiDAR frame; f = 1, c = 0: u = -y / x, v = -z / x, depth = x, all exact in fp32."""
    return calibration_kitti.Calibration({"P2": np.eye(3, 4, dtype=np.float32), "R0": np.eye(3, dtype=np.float32),
                                          "Tr_velo2cam": np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0]], np.float32)})


def test_edges_of_the_image_and_of_depth_on_an_exact_calibration():
    rows = [
        ([1, 0, -1], 1),      # u = 0, v = 1
        ([2, -15, -2], 1),    # u = 7.5
        ([1, -8, -1], 0),     # u = 8 = width
        ([1, 1, -1], 0),      # u = -1
        ([1, -1, 0], 1),      # v = 0
        ([2, -2, -7], 1),     # v = 3.5
        ([1, -1, -4], 0),     # v = 4 = height
        ([1, -1, 1], 0),      # v = -1
        ([0, -1, -1], 0),     # depth 0, camera x != 0: u = +inf
        ([0, 1, 1], 0),       # depth 0: u = v = -inf
        ([0, 0, -1], 0),      # depth 0 and camera x = 0: u = NaN
        ([0, 0, 0], 0),       # the origin: NaN, NaN
        ([-1, 1, 1], 0),      # depth -1 although the pixel (1, 1) is in range
        ([-2, 6, 2], 0),      # depth -2, pixel (3, 1)
        ([4, -4, -4], 1),     # (1, 1) at depth 4
    ]
    pts = np.array([r[0] + [0.5] for r in rows], np.float32)
    want = np.array([r[1] for r in rows], np.int32)
    m, p2 = exact_calib().fov_matrices()
    assert np.array_equal(m, np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, 0]], np.float32))
    got = ops.points_fov_flags(dev(pts), m, p2, (4, 8)).cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    with np.errstate(all="ignore"):
        assert np.array_equal(host_flags(pts, exact_calib(), np.array([4, 8], np.int32)).astype(np.int32), want)      # numpy says the same
    assert torch.cuda.is_available() and ops.points_fov_flags(dev(pts), m, p2, (4, 8)).sum().item() == want.sum()       # the device is alive after the divisions by zero


@pytest.mark.parametrize("n", [0, 1, 63, 65, 257])
@pytest.mark.parametrize("layout", ["c4", "c5", "c4_unaligned"])
def test_row_counts_and_layouts(gold, n, layout):
    calib = cases.golden_calib(gold)
    m, p2 = calib.fov_matrices()
    pts = gold["points"][100:100 + n]
    want = gold["fov_flags"][100:100 + n].astype(np.int32)
    assert not gold["borderline"][100:357].any()
    if layout == "c5":                    # scalar loads
        table = dev(np.concatenate([pts, np.full((n, 1), 3.0, np.float32)], 1))
    elif layout == "c4_unaligned":        # a view one float into a 16-byte aligned allocation: c == 4, base not 16-byte aligned
        flat = torch.zeros(4 * n + 1, dtype=torch.float32, device="cuda")
        flat[1:] = dev(pts).reshape(-1)
        table = flat[1:].view(n, 4)
        assert n == 0 or table.data_ptr() % 16 == 4
    else:
        table = dev(pts)
        assert n == 0 or table.data_ptr() % 16 == 0
    got = ops.points_fov_flags(table, m, p2, gold["image_shape"])
    assert got.shape == (n,) and np.array_equal(got.cpu().numpy(), want)


def test_device_side_row_count_leaves_the_tail_untouched(gold):
    from toda_amd import lib as L
    lib = L.load()
    m, p2 = cases.golden_calib(gold).fov_matrices()
    mh, ph = L.host_f32(m.reshape(-1)), L.host_f32(p2.reshape(-1))
    pts = dev(gold["points"][:300])
    for rows in (0, 1, 200, 300, 1000):
        flags = torch.full((300,), SENTINEL, dtype=torch.int32, device="cuda")
        n_dev = torch.tensor([rows], dtype=torch.int32, device="cuda")
        rc = lib.toda_points_fov_flags(L.ptr(pts), 300, L.ptr(n_dev), 4, L.hptr(mh), L.hptr(ph), 375, 1242, L.ptr(flags), L.stream())
        assert rc == 0
        got, k = flags.cpu().numpy(), min(rows, 300)
        assert np.array_equal(got[:k], gold["fov_flags"][:k].astype(np.int32)) and (got[k:] == SENTINEL).all()


def test_bad_arguments_return_minus_one():
    from toda_amd import lib as L
    lib = L.load()
    mat = L.host_f32([0.0] * 12)
    p = L.hptr(mat)
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    out = torch.zeros(16, dtype=torch.int32, device="cuda")
    d, o = buf.data_ptr(), out.data_ptr()
    assert lib.toda_points_fov_flags(d, 4, None, 2, p, p, 4, 8, o, None) == -1 and b"columns" in lib.toda_last_error()
    assert lib.toda_points_fov_flags(d, -1, None, 4, p, p, 4, 8, o, None) == -1
    assert lib.toda_points_fov_flags(d, 4, None, 4, p, p, 0, 8, o, None) == -1 and b"image" in lib.toda_last_error()
    assert lib.toda_points_fov_flags(d, 4, None, 4, p, p, 4, -8, o, None) == -1
    assert lib.toda_points_fov_flags(d, 4, None, 4, None, p, 4, 8, o, None) == -1 and b"null" in lib.toda_last_error()
    assert lib.toda_points_fov_flags(d, 4, None, 4, p, None, 4, 8, o, None) == -1
    assert lib.toda_points_fov_flags(None, 4, None, 4, p, p, 4, 8, o, None) == -1 and b"null" in lib.toda_last_error()
    assert lib.toda_points_fov_flags(d, 4, None, 4, p, p, 4, 8, None, None) == -1
    assert lib.toda_points_fov_flags(None, 0, None, 4, p, p, 4, 8, None, None) == 0           # nothing to do
    with pytest.raises(RuntimeError):
        ops.points_fov_flags(torch.zeros(4, 4), np.zeros(12), np.zeros(12), (4, 8))              # a host tensor


# ---- the dataset end to end ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built(tmp_path_factory, gold):
    root = cases.write_tree(tmp_path_factory.mktemp("kitti"), gold)
    infos = create_kitti_infos(cases.dataset_cfg(root), CLASSES, data_path=root, save_path=root)
    return root, infos


def test_info_pickles(built, gold):
    root, _ = built
    loaded = {}
    for split, count in (("train", 2), ("val", 1), ("trainval", 3), ("test", 1)):
        with open(root / f"kitti_infos_{split}.pkl", "rb") as f:
            loaded[split] = pickle.load(f)
        assert len(loaded[split]) == count
    assert "annos" not in loaded["test"][0] and set(loaded["test"][0]) == {"point_cloud", "image", "calib"}
    for info, frame in zip(loaded["trainval"], ["000000", "000001", "000002"]):
        assert info["point_cloud"] == {"num_features": 4, "lidar_idx": frame} and info["image"]["image_idx"] == frame
        assert info["image"]["image_shape"].tolist() == [375, 1242]
        for key in ("P2", "R0_rect", "Tr_velo_to_cam"):
            assert info["calib"][key].shape == (4, 4) and info["calib"][key][3].tolist() == [0, 0, 0, 1]
        assert np.array_equal(info["calib"]["P2"][:3].astype(np.float32), gold["P2"]) and np.array_equal(info["calib"]["R0_rect"][:3, :3], gold["R0"])
        a, k = info["annos"], len(cases.FRAMES[frame])
        assert set(a) == {"name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score", "difficulty",
                          "index", "gt_boxes_lidar", "num_points_in_gt"}
        assert list(a["name"]) == [f[0] for f in cases.FRAMES[frame]] + ["DontCare"]
        assert a["bbox"].shape == (k + 1, 4) and a["dimensions"].shape == (k + 1, 3) and a["location"].shape == (k + 1, 3) and a["gt_boxes_lidar"].shape == (k, 7)
        assert a["index"].tolist() == list(range(k)) + [-1] and a["index"].dtype == np.int32 and a["difficulty"].dtype == np.int32
        want = np.array([f[1] for f in cases.FRAMES[frame]])
        assert np.abs(a["gt_boxes_lidar"] - want).max() < 0.012                       # labels carry two decimals
        # the first Car holds the 10 known points, each more than 0.2 m clear of its faces; its neighbourhood was emptied
        assert a["num_points_in_gt"].tolist() == [cases.N_KNOWN] + [0] * (k - 1) + [-1] and a["num_points_in_gt"].dtype == np.int32
    assert loaded["trainval"][0]["annos"]["difficulty"].tolist() == [0, 2] + [0] * 15 + [-1]
    with open(root / "kitti_dbinfos_train.pkl", "rb") as f:
        db = pickle.load(f)
    assert sorted(db) == ["Car", "Pedestrian"] and len(db["Car"]) == sum(f[0] == "Car" for fr in ("000000", "000001") for f in cases.FRAMES[fr])
    first = db["Car"][0]
    assert first["image_idx"] == "000000" and first["num_points_in_gt"] == cases.N_KNOWN and first["difficulty"] == 0 and first["bbox"].shape == (4,)
    obj = np.fromfile(str(root / first["path"]), np.float32).reshape(-1, 4)
    assert first["path"] == "gt_database/000000_Car_0.bin" and obj.shape == (cases.N_KNOWN, 4)
    assert np.abs(obj[:, :3] + first["box3d_lidar"][:3] - cases.known_points(cases.FRAMES["000000"][0][1])[:, :3]).max() < 1e-5


def open_dataset(root, **extra):
    cfg = cases.dataset_cfg(root, **extra)
    cfg["INFO_PATH"] = {"train": ["kitti_infos_train.pkl"], "test": ["kitti_infos_trainval.pkl"]}
    return KittiDataset(cfg, CLASSES, training=False, root_path=root)


def test_samples_keep_the_reference_rows_in_order(built, gold):
    root, _ = built
    shift = [0.0, 0.0, 1.6]
    plain = open_dataset(root, processors=("voxel",))
    moved = open_dataset(root, processors=("voxel",), SHIFT_COOR=shift, GET_ITEM_LIST=["points", "gt_boxes2d"])
    assert len(plain) == 3 and plain.on_device
    for i, frame in enumerate(["000000", "000001", "000002"]):
        points, in_fov = cases.frame_points(gold, frame)
        a, b = plain[i], moved[i]
        assert a["frame_id"] == frame and a["points"].is_cuda and a["image_shape"].tolist() == [375, 1242]
        assert isinstance(a["calib"], calibration_kitti.Calibration)
        assert np.array_equal(a["points"].cpu().numpy(), points[in_fov])                        # same rows, same order, same bits
        want = points[in_fov].copy()
        want[:, :3] += np.array(shift, np.float32)
        assert np.array_equal(b["points"].cpu().numpy(), want)
        boxes = np.array([f[1] for f in cases.FRAMES[frame]])
        cls = np.array([CLASSES.index(f[0]) + 1 for f in cases.FRAMES[frame]])
        assert a["gt_boxes"].shape == (len(boxes), 8) and np.abs(a["gt_boxes"][:, :7] - boxes).max() < 0.012 and np.array_equal(a["gt_boxes"][:, 7], cls)
        assert np.abs(b["gt_boxes"][:, :3] - a["gt_boxes"][:, :3] - shift).max() < 1e-6
        assert b["gt_boxes2d"].shape == (len(boxes), 4) and "gt_boxes2d" not in a
        assert ("road_plane" in a) == (frame == "000000")
    full = open_dataset(root)[0]["points"].cpu().numpy()                                        # with the range mask behind the crop
    points, in_fov = cases.frame_points(gold, "000000")
    kept = points[in_fov]
    inside = (kept[:, 0] >= 0) & (kept[:, 0] <= 70.4) & (kept[:, 1] >= -40) & (kept[:, 1] <= 40)
    assert np.array_equal(full, kept[inside])


def test_collate_predict_and_score_full_marks(built, tmp_path):
    root, _ = built
    ds = open_dataset(root, SHIFT_COOR=[0.0, 0.0, 1.6])
    samples = [ds[i] for i in range(3)]
    batch = DatasetTemplate.collate_batch(samples[:2])
    assert batch["batch_size"] == 2 and batch["points"].is_cuda and batch["points"].shape[1] == 5
    assert batch["points_per_sample"] == [len(s["points"]) for s in samples[:2]]
    assert isinstance(batch["calib"], list) and batch["calib"][1] is samples[1]["calib"]
    assert batch["image_shape"].shape == (2, 2) and batch["image_shape"].dtype == np.int32 and batch["gt_boxes"].shape == (2, 17, 8)
    whole = DatasetTemplate.collate_batch(samples)
    preds = [{"pred_boxes": dev(s["gt_boxes"][:, :7]), "pred_scores": torch.ones(len(s["gt_boxes"]), device="cuda"),
              "pred_labels": dev(s["gt_boxes"][:, 7].astype(np.int64))} for s in samples]
    annos = ds.generate_prediction_dicts(whole, preds, CLASSES, output_path=tmp_path)
    assert [a["frame_id"] for a in annos] == ["000000", "000001", "000002"] and (tmp_path / "000002.txt").read_text().count("\n") == 17
    for a, info in zip(annos, ds.kitti_infos):
        gt = info["annos"]
        assert list(a["name"]) == list(gt["name"][:-1])
        assert np.abs(a["location"] - gt["location"][:-1]).max() < 1e-4 and np.abs(a["dimensions"] - gt["dimensions"][:-1]).max() < 1e-5
        assert np.abs(a["bbox"] - gt["bbox"][:-1]).max() < 0.5 and np.abs(a["boxes_lidar"] - gt["gt_boxes_lidar"]).max() < 1e-4
    text, res = ds.evaluation(annos, CLASSES, eval_metric="kitti")
    print(text)
    # Cars: 48 Easy, one Moderate (occluded 1) and one Hard (occluded 2) - the evaluator takes one threshold per ground truth, so
    # 41 or more are needed for a full precision curve; every detection is its own ground truth
    for label in ("image", "bev", "3d"):
        for diff in ("easy", "moderate", "hard"):
            assert res[f"Car_{label}/{diff}_R40"] == 100.0
    r11, r40 = text.split("Car AP@0.70, 0.70, 0.70:\n")[1], text.split("Car AP_R40@0.70, 0.70, 0.70:\n")[1]
    for block in (r11, r40):
        rows = block.splitlines()[:3]
        assert [r.split(" AP:")[0].strip() for r in rows] == ["bbox", "bev", "3d"]
        for r in rows:
            assert [float(v) for v in r.split("AP:")[1].split(",")] == [100.0, 100.0, 100.0], r


def test_training_samples_through_the_shipped_dataset_config(built):
    """kitti_dataset.yaml as shipped (FOV crop, gt_sampling on the road plane, world flip / rotation / scaling) on the mini tree;
    only the sampler's groups are cut down to the one class whose database objects hold points."""
    import os

    from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
    root, _ = built
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = cfg_from_yaml_file(os.path.join(here, "toda_amd/tools/cfgs/dataset_configs/kitti_dataset.yaml"), AttrDict())
    sampler = cfg.DATA_AUGMENTOR.AUG_CONFIG_LIST[0]
    assert sampler.NAME == "gt_sampling" and sampler.USE_ROAD_PLANE and cfg.FOV_POINTS_ONLY and cfg.POINT_CLOUD_RANGE == [0, -40, -3, 70.4, 40, 1]
    sampler.SAMPLE_GROUPS = ["Car:20"]
    ds = KittiDataset(cfg, CLASSES, training=True, root_path=root)
    assert len(ds) == 2 and ds.on_device and len(ds.data_augmentor.data_augmentor_queue[0].db_infos["Car"]) == 2
    np.random.seed(3)
    samples = [ds[0], ds[1]]
    for s in samples:
        assert s["points"].is_cuda and s["points"].shape[1] == 4 and torch.isfinite(s["points"]).all()
        assert "calib" not in s and "road_plane" not in s and s["image_shape"].tolist() == [375, 1242]
        assert s["gt_boxes"].shape[1] == 8 and len(s["gt_boxes"]) >= 1 and set(s["gt_boxes"][:, 7]) <= {1.0, 2.0}
        xy = s["points"][:, :2].cpu().numpy()
        assert (xy[:, 0] >= 0).all() and (xy[:, 0] <= 70.4).all() and (np.abs(xy[:, 1]) <= 40).all()
    batch = ds.collate_batch(samples)
    assert batch["points"].is_cuda and batch["gt_boxes"].shape[0] == 2 and batch["image_shape"].shape == (2, 2)
