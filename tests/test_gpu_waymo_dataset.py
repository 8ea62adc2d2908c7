"""WaymoDataset and WaymoNusMixDataset on the MI355X: the frame kernel (csrc/waymo_frame.hip) against the reference's output
(tests/golden/waymo_dataset.npz) and, at its edges, against the numpy route; the dataset end to end on a mini Waymo tree: loader
-> collate -> one CenterPoint step, the GT database, GT sampling, the KITTI-style AP; and the two-domain dataset on that tree plus
a mini nuScenes tree.

x, y, z, the elongation and the flags are compared bit for bit.  The kernel's intensity is (float)tanh((double)x); it is compared
bit for bit with the same expression in numpy (waymo_dataset_cases.tanh_fp64) - the fixture's and the random intensities lie
farther than 2^-40 (relative) from every fp32 rounding midpoint, so two fp64 tanh routines that differ in their last bits round
alike - and with the reference's column (numpy's fp32 tanh) within `tanh_ulp_ref`, the distance the capture measured between
that routine and the fp64 criterion."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import nuscenes_dataset_cases as nus_cases
from tests import waymo_dataset_cases as cases
from toda_amd import ops
from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
from toda_amd.pcdet.datasets.nuscenes.nuscenes_dataset import NuScenesDataset
from toda_amd.pcdet.datasets.two_dataset import WaymoNusMixDataset
from toda_amd.pcdet.datasets.waymo.waymo_dataset import WaymoDataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = [-200.0, -200.0, -10.0, 200.0, 200.0, 10.0]
SENTINEL = -7
XYZE = [0, 1, 2, 4]


@pytest.fixture(scope="module")
def gold():
    return cases.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_bits_or_nan(a, b):
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and same_bits(np.where(nan, np.float32(0), a), np.where(nan, np.float32(0), b))


def frame_pass(rows, use_nlz=True):
    """(compacted rows, flags, every written row) of the device route on a device tensor."""
    out, flags = ops.waymo_frame(rows, use_nlz=use_nlz)
    kept = ops.RowBuffer(out.shape[0], 5, out.device).append(out, flags, 1).finish()
    return kept.cpu().numpy(), flags.cpu().numpy(), out.cpu().numpy()


def check_against_numpy(rows, use_nlz, device_rows=None):
    """The device route on `rows` against the numpy route and the fp64 criterion; returns the flags."""
    kept, flags, out = frame_pass(dev(rows) if device_rows is None else device_rows, use_nlz)
    want_flags = (rows[:, 5] == -1).astype(np.int32) if use_nlz else np.ones(len(rows), np.int32)
    assert flags.dtype == np.int32 and np.array_equal(flags, want_flags)
    assert out.shape == (len(rows), 5) and same_bits(out[:, XYZE], rows[:, XYZE])                 # every row is written, kept or not
    assert same_bits_or_nan(out[:, 3], cases.tanh_fp64(rows[:, 3]))
    want = cases.host_route(rows, use_nlz)
    assert kept.shape == want.shape and same_bits(kept[:, XYZE], want[:, XYZE])                   # the numpy route's rows in its order
    assert same_bits(kept, out[want_flags == 1])
    return flags


# ---- the kernel against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,use_nlz", [("nlz", True), ("all", False)])
@pytest.mark.parametrize("k", [0, 1])
def test_frame_pass_and_compaction_equal_the_reference(gold, tag, use_nlz, k):
    rows, want, ulp_ref = gold[f"frame{k}"], gold[f"points_{tag}_{k}"], int(gold["tanh_ulp_ref"])
    kept, flags, out = frame_pass(dev(rows), use_nlz)
    assert flags.dtype == np.int32 and np.array_equal(flags, np.isin(rows[:, 4], want[:, 4]).astype(np.int32))      # column 4 is a unique row id
    assert same_bits(out[:, XYZE], rows[:, XYZE]) and same_bits(out[:, 3], cases.tanh_fp64(rows[:, 3]))
    assert same_bits(kept[:, XYZE], want[:, XYZE])                                                # the reference's rows in its order
    distance = cases.ulp_distance(kept[:, 3], want[:, 3])
    print(f"{tag} frame {k}: intensity at most {int(distance.max())} ulp from the reference's column, tanh_ulp_ref {ulp_ref}")
    assert distance.max() <= ulp_ref
    assert flags.sum() == len(want) and (not use_nlz or 0 < flags.sum() < len(flags))


def test_dataset_frames_equal_the_reference(tmp_path, gold):
    seq = cases.write_golden_tree(tmp_path, gold)
    for tag, disable in (("nlz", False), ("all", True)):
        ds = WaymoDataset(cases.dataset_cfg(tmp_path, POINT_CLOUD_RANGE=WIDE, DISABLE_NLZ_FLAG_ON_POINTS=disable), cases.CLASSES, training=False)
        for k in range(2):
            points, want = ds.get_lidar(seq, k), gold[f"points_{tag}_{k}"]
            assert points.is_cuda and points.dtype == torch.float32
            got = points.cpu().numpy()
            assert same_bits(got[:, XYZE], want[:, XYZE]) and cases.ulp_distance(got[:, 3], want[:, 3]).max() <= int(gold["tanh_ulp_ref"])
        item = ds[0]["points"]
        assert item.is_cuda and same_bits(item.cpu().numpy()[:, XYZE], gold[f"points_{tag}_0"][:, XYZE])        # test mode: no shuffle, nothing out of range


# ---- edges, against the numpy route and the fp64 criterion -----------------------------------------------------------------
@pytest.mark.parametrize("c_in", [6, 7])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_row_counts_at_the_workgroup_edge(n, c_in):
    rows = cases.random_frame(np.random.default_rng(1000 * c_in + n), n, c_in=c_in)
    for use_nlz in (True, False):
        flags = check_against_numpy(rows, use_nlz)
        assert flags.shape == (n,)
    assert n < 255 or 0 < (rows[:, 5] == -1).sum() < n


def test_every_row_flagged_away_and_none():
    rng = np.random.default_rng(2)
    gone = cases.random_frame(rng, 300, nlz=(0.0, 1.0))
    assert not check_against_numpy(gone, True).any()
    kept, _, _ = frame_pass(dev(gone), True)
    assert kept.shape == (0, 5)
    stay = cases.random_frame(rng, 300, nlz=(-1.0,))
    assert check_against_numpy(stay, True).all()


def test_nlz_flags_next_to_minus_one_and_nan():
    rng = np.random.default_rng(3)
    rows = cases.random_frame(rng, 64, nlz=(-1.0,))
    minus = np.float32(-1.0)
    rows[:6, 5] = [np.nextafter(minus, np.float32(0)), np.nextafter(minus, np.float32(-2)), np.nan, -1.0, 1.0, -np.inf]
    assert check_against_numpy(rows, True)[:6].tolist() == [0, 0, 0, 1, 0, 0]
    rows[:, 5] = np.nan                                                                            # without the filter column 5 decides nothing
    assert check_against_numpy(rows, False).all()
    assert not check_against_numpy(rows, True).any()


def test_special_intensities():
    rng = np.random.default_rng(4)
    rows = cases.random_frame(rng, 40, nlz=(-1.0,))
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 9.0, 9.1, 100.0, np.inf, -np.inf, np.nan, -0.75, -9.1, 1.1754944e-38, 3.0e38], np.float32)
    assert cases.tanh_tie_free(special).all()
    rows[:len(special), 3] = special
    check_against_numpy(rows, True)
    _, _, out = frame_pass(dev(rows))
    got = out[:len(special), 3]
    assert got[0] == 0 and not np.signbit(got[0]) and got[1] == 0 and np.signbit(got[1])                   # the sign of zero is kept
    assert got[2] == special[2] and got[3] == special[3]                                                    # a denormal passes unchanged
    assert got[4] == np.nextafter(np.float32(1), np.float32(0)) and got[5] == 1                             # 9.0 and 9.1: either side of fp32 saturation
    assert got[6] == 1 and got[7] == 1 and got[8] == -1 and np.isnan(got[9]) and got[11] == -1 and got[13] == 1
    assert got[10] == np.float32(np.tanh(np.float64(np.float32(-0.75))))


@pytest.mark.parametrize("c_in", [6, 7])
def test_a_view_one_row_into_a_buffer(c_in):
    rows = cases.random_frame(np.random.default_rng(5 + c_in), 300, c_in=c_in)
    buf = torch.zeros((len(rows) + 1, c_in), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[1:] = dev(rows)
    view = buf[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * c_in) % 16                       # 24 or 28 bytes past a 16-byte boundary
    check_against_numpy(rows, True, device_rows=view)
    check_against_numpy(rows, False, device_rows=view)


def test_rows_after_the_tables_stay_untouched():
    from toda_amd import lib as L
    lib = L.load()
    n, extra = 257, 3
    rows = cases.random_frame(np.random.default_rng(6), n)
    table = dev(rows)
    out = torch.full((n + extra, 5), float(SENTINEL), dtype=torch.float32, device="cuda")
    flags = torch.full((n + extra,), SENTINEL, dtype=torch.int32, device="cuda")
    assert lib.toda_waymo_frame(L.ptr(table), n, 6, 1, L.ptr(out), L.ptr(flags), L.stream()) == 0
    torch.cuda.synchronize()
    assert (out[n:] == SENTINEL).all() and (flags[n:] == SENTINEL).all()
    assert same_bits(out[:n].cpu().numpy()[:, XYZE], rows[:, XYZE]) and np.array_equal(flags[:n].cpu().numpy(), (rows[:, 5] == -1).astype(np.int32))
    assert lib.toda_waymo_frame(None, n, 6, 1, L.ptr(out), L.ptr(flags), L.stream()) == -1 and b"null" in lib.toda_last_error()
    assert lib.toda_waymo_frame(L.ptr(table), n, 5, 1, L.ptr(out), L.ptr(flags), L.stream()) == -1 and b"columns" in lib.toda_last_error()
    assert lib.toda_waymo_frame(None, 0, 6, 1, None, None, L.stream()) == 0


def test_bad_tensors_are_refused():
    good = torch.zeros((4, 6), dtype=torch.float32, device="cuda")
    out, flags = ops.waymo_frame(torch.zeros((0, 6), dtype=torch.float32, device="cuda"))
    assert out.shape == (0, 5) and flags.shape == (0,) and flags.dtype == torch.int32
    with pytest.raises(RuntimeError, match="device"):
        ops.waymo_frame(torch.zeros((4, 6)))                                                       # a host tensor
    with pytest.raises(RuntimeError, match="float32"):
        ops.waymo_frame(good.double())
    with pytest.raises(RuntimeError, match="columns"):
        ops.waymo_frame(torch.zeros((4, 5), dtype=torch.float32, device="cuda"))                   # no NLZ column
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.waymo_frame(torch.zeros((4, 7), dtype=torch.float32, device="cuda")[:, :6])
    with pytest.raises(RuntimeError):
        ops.waymo_frame(torch.zeros((24,), dtype=torch.float32, device="cuda"))


# ---- the dataset end to end ---------------------------------------------------------------------------------------------
STEM = f"{cases.TAG}_gt_database_train_sampled_1"


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    data_path = cases.write_tree(tmp_path_factory.mktemp("waymo"))
    ds = WaymoDataset(cases.dataset_cfg(data_path), cases.CLASSES, training=True)
    info_path = data_path / f"{cases.TAG}_infos_train.pkl"
    with open(info_path, "wb") as f:
        pickle.dump(cases.all_infos(data_path), f)
    db = ds.create_groundtruth_database(info_path, data_path, used_classes=cases.CLASSES, split="train", sampled_interval=1, processed_data_tag=cases.TAG)
    return data_path, ds, db


def in_box(points, box, margin=0.0):
    return (np.abs(points[:, :3] - box[:3]) <= box[3:6] / 2 + margin).all(1)


def exact_cloud(k):
    """The frame pass on frame k of the mini tree in numpy with the fp64 criterion: what the device route returns."""
    rows = cases.frame_rows(k)
    kept = rows[rows[:, 5] == -1][:, 0:5].copy()
    kept[:, 3] = cases.tanh_fp64(kept[:, 3])
    return kept


@pytest.mark.parametrize("training", [False, True])
def test_getitem_equals_the_host_routes_sample(built, gold, training):
    data_path = built[0]
    still = [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
             {"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.1, 0.1, 0.15], "MAX_POINTS_PER_VOXEL": 5, "MAX_NUMBER_OF_VOXELS": {"train": 60000, "test": 60000}}]
    ds = WaymoDataset(cases.dataset_cfg(data_path, DATA_PROCESSOR=[AttrDict(s) for s in still], DATA_SPLIT={"train": "train", "test": "train"}),
                      cases.CLASSES, training=training)
    assert len(ds) == 8
    for k in (0, 5):
        got = ds[k]
        host = ds.raw_frame(k, host=True)
        host.pop("metadata")
        want = ds.prepare_data(host)
        assert got["points"].is_cuda and isinstance(want["points"], np.ndarray)
        points = got["points"].cpu().numpy()
        assert same_bits(points[:, XYZE], want["points"][:, XYZE]) and cases.ulp_distance(points[:, 3], want["points"][:, 3]).max() <= int(gold["tanh_ulp_ref"])
        assert same_bits(points, exact_cloud(k))                                          # nothing of the tree lies outside the range
        boxes, names, _ = cases.frame_boxes(k)
        keep = (names != "unknown") & ((cases.points_in_boxes_count(k) > 0) | (not training))
        assert same_bits(got["gt_boxes"], want["gt_boxes"]) and same_bits(got["gt_boxes"][:, :7], boxes[keep])
        assert got["gt_boxes"][:, 7].tolist() == [cases.CLASSES.index(n) + 1 for n in names[keep]]
        assert got["frame_id"] == f"{cases.SEQUENCES[k // 4]}_{k % 4:03d}" and got["metadata"]["context_name"] == cases.SEQUENCES[k // 4]
        assert "num_points_in_gt" not in got and "gt_names" not in got


def test_groundtruth_database(built):
    data_path, ds, db = built
    with open(data_path / f"{cases.TAG}_waymo_dbinfos_train_sampled_1.pkl", "rb") as f:
        stored = pickle.load(f)
    assert sorted(stored) == sorted(db) == ["Cyclist", "Pedestrian", "Vehicle"]
    # Vehicle boxes only from every 4th frame of the list, Pedestrian boxes from every 2nd
    assert sorted((e["sequence_name"], e["sample_idx"]) for e in stored["Vehicle"]) == sorted((cases.SEQUENCES[k // 4], k % 4) for k in (0, 4) for _ in range(6))
    assert [(e["sequence_name"], e["sample_idx"]) for e in stored["Pedestrian"]] == [(cases.SEQUENCES[k // 4], k % 4) for k in (0, 2, 4, 6)]
    assert [(e["sequence_name"], e["sample_idx"]) for e in stored["Cyclist"]] == [(cases.SEQUENCES[k // 4], k % 4) for k in range(8)]
    records, files = [], sorted(p.name for p in (data_path / STEM).iterdir())
    for k in range(8):
        boxes, names, difficulty = cases.frame_boxes(k)
        keep = np.ones(len(names), bool)
        if k % 4:
            keep &= names != "Vehicle"
        if k % 2:
            keep &= names != "Pedestrian"
        boxes, names, difficulty = boxes[keep], names[keep], difficulty[keep]
        seq, idx = cases.SEQUENCES[k // 4], k % 4
        cloud = exact_cloud(k)                                                       # the no-label-zone rows are gone
        for i, name in enumerate(names):
            rel = f"{STEM}/{seq}_{idx:04d}_{name}_{i}.bin"
            if name == "unknown":                                                     # not a used class: no file, no record
                assert not (data_path / rel).exists()
                continue
            info = [e for e in stored[name] if e["sequence_name"] == seq and e["sample_idx"] == idx and e["gt_idx"] == i]
            assert len(info) == 1
            info = info[0]
            inside = in_box(cloud, boxes[i])
            obj = np.fromfile(str(data_path / rel), np.float32).reshape(-1, 5)
            assert info["path"] == rel and info["name"] == name and info["difficulty"] == difficulty[i] and same_bits(info["box3d_lidar"], boxes[i])
            assert info["num_points_in_gt"] == inside.sum() == len(obj) == (0 if name == "Vehicle" and i == 5 else cases.N_IN_BOX)
            assert same_bits(obj[:, 3:], cloud[inside][:, 3:]) and np.abs(obj[:, :3] + boxes[i, :3] - cloud[inside][:, :3]).max(initial=0) < 1e-5
            records.append((info["global_data_offset"], obj))
    assert len(files) == len(records) == 12 + 4 + 8 and not any("unknown" in f for f in files)
    packed = np.load(data_path / f"{STEM}_global.npy")
    records.sort(key=lambda r: (r[0][0], r[0][1]))
    assert records[0][0][0] == 0 and records[-1][0][1] == len(packed) and all(a[0][1] == b[0][0] for a, b in zip(records, records[1:]))
    assert packed.dtype == np.float32 and same_bits(packed, np.concatenate([obj for _, obj in records], 0))
    for (lo, hi), obj in records:
        assert same_bits(packed[lo:hi], obj)


def test_database_feeds_gt_sampling(built):
    data_path = built[0]
    sampler = {"NAME": "gt_sampling", "USE_ROAD_PLANE": False, "DB_INFO_PATH": [f"{cases.TAG}_waymo_dbinfos_train_sampled_1.pkl"],
               "PREPARE": {"filter_by_min_points": ["Vehicle:5"], "filter_by_difficulty": [-1]}, "SAMPLE_GROUPS": ["Vehicle:9"], "NUM_POINT_FEATURES": 5,
               "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": True}
    cfg = cases.dataset_cfg(data_path, DATA_AUGMENTOR=AttrDict({"DISABLE_AUG_LIST": ["placeholder"], "AUG_CONFIG_LIST": [AttrDict(sampler)]}))
    ds = WaymoDataset(cfg, cases.CLASSES, training=True)
    assert len(ds.data_augmentor.data_augmentor_queue[0].db_infos["Vehicle"]) == 10        # 12 stored, two of them without points
    np.random.seed(0)
    k = 7                                                                                   # its own Vehicles are not in the database
    sample = ds[k]
    boxes, names, _ = cases.frame_boxes(k)
    own = boxes[(names != "unknown") & (cases.points_in_boxes_count(k) > 0)]
    got = sample["gt_boxes"]
    # the scene holds 5 Vehicles with points: 9 - 5 = 4 are drawn, and an object of another frame touches no box of this one
    assert got.shape == (len(own) + 4, 8) and (got[:, 7] == 1).sum() == 9
    pasted = np.array([b for b in got[:, :7] if not (np.abs(own - b).max(1) < 1e-6).any()])
    assert len(pasted) == 4 and all(any(np.abs(cases.frame_boxes(f)[0][:6] - b).max(1).min() < 1e-6 for f in (0, 4)) for b in pasted)
    cloud = exact_cloud(k)
    inside, near = np.zeros(len(cloud), bool), np.zeros(len(cloud), bool)
    for b in pasted:                                                                        # the scene's points under a pasted box give way; the test
        inside |= in_box(cloud, b)                                                          # that removes them has a margin of a centimetre
        near |= in_box(cloud, b, margin=0.011)
    assert sample["points"].is_cuda and len(cloud) - near.sum() <= sample["points"].shape[0] - 4 * cases.N_IN_BOX <= len(cloud) - inside.sum()
    pts = sample["points"].cpu().numpy()
    assert all(in_box(pts, b).sum() == cases.N_IN_BOX for b in pasted)


def small_model_cfg(data_path):
    cfg = cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/models/centerpoint_waymo_real.yaml"), AttrDict())
    data = cfg.DATA_CONFIG
    assert data.DATASET == "WaymoDataset" and data.SAMPLED_INTERVAL.train == 5 and data.DISABLE_NLZ_FLAG_ON_POINTS
    data.DATA_PATH, data.POINT_CLOUD_RANGE, data.SAMPLED_INTERVAL = str(data_path), cases.RANGE, AttrDict({"train": 1, "test": 1})
    sampler = data.DATA_AUGMENTOR.AUG_CONFIG_LIST[0]
    assert sampler.NAME == "gt_sampling" and sampler.DB_INFO_PATH == [f"{cases.TAG}_waymo_dbinfos_train_sampled_1.pkl"]      # the name the database got
    cfg.MODEL.BACKBONE_2D.LAYER_NUMS = [1, 1]
    return cfg


def test_loader_batch_and_one_centerpoint_step(built):
    from toda_amd.pcdet.datasets import build_dataloader
    from toda_amd.pcdet.models import build_network, prepare_batch_on_gpu
    cfg = small_model_cfg(built[0])
    np.random.seed(0)
    torch.manual_seed(0)
    ds, loader, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, batch_size=2, dist=False, workers=2, training=True)
    assert isinstance(ds, WaymoDataset) and ds.on_device and loader.num_workers == 0 and len(ds) == 8 and not ds.use_nlz
    assert len(ds.data_augmentor.data_augmentor_queue[0].db_infos["Vehicle"]) == 10         # the database is read
    batch = next(iter(loader))
    assert batch["batch_size"] == 2 and batch["points"].is_cuda and batch["points"].shape[1] == 6 and torch.isfinite(batch["points"]).all()
    assert batch["gt_boxes"].ndim == 3 and batch["gt_boxes"].shape[0] == 2 and batch["gt_boxes"].shape[2] == 8 and batch["gt_boxes"].shape[1] >= 7
    assert np.isfinite(batch["gt_boxes"]).all() and set(np.unique(batch["gt_boxes"][..., 7])) <= {0.0, 1.0, 2.0, 3.0}
    assert len(batch["frame_id"]) == 2 and len(batch["metadata"]) == 2 and "num_points_in_gt" not in batch
    assert float(batch["points"][:, 4].min()) >= 0 and float(batch["points"][:, 4].max()) <= 1      # tanh of a positive intensity
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    prepare_batch_on_gpu(batch, net)
    ret, tb, _ = net(batch)
    loss = ret["loss"]
    assert torch.isfinite(loss), tb
    loss.backward()
    grads = [p.grad for p in net.dense_head.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads) and float(sum(g.abs().sum() for g in grads)) > 0


def test_ground_truth_fed_back_scores_full_marks(built):
    data_path = built[0]
    ds = WaymoDataset(cases.dataset_cfg(data_path, DATA_SPLIT={"train": "train", "test": "train"}), cases.CLASSES, training=False)
    samples = [ds[i] for i in range(len(ds))]
    assert len(samples) == 8 and all(s["points"].is_cuda and s["gt_boxes"].shape == (8, 8) for s in samples)
    batch = ds.collate_batch(samples)
    preds = [{"pred_boxes": dev(s["gt_boxes"][:, :7]), "pred_scores": torch.ones(8, device="cuda"), "pred_labels": dev(s["gt_boxes"][:, 7].astype(np.int64))}
             for s in samples]
    annos = ds.generate_prediction_dicts(batch, preds, cases.CLASSES)
    for k, anno in enumerate(annos):
        assert anno["frame_id"] == f"{cases.SEQUENCES[k // 4]}_{k % 4:03d}" and list(anno["name"]) == list(cases.frame_boxes(k)[1][:8])
        assert same_bits(anno["boxes_lidar"], cases.frame_boxes(k)[0][:8])
    before = pickle.dumps(ds.infos)
    text, res = ds.evaluation(annos, cases.CLASSES, eval_metric="kitti")
    print(text)
    assert pickle.dumps(ds.infos) == before and annos[0]["name"][0] == "Vehicle"                 # the evaluator works on copies
    # 48 Vehicles, all Easy under the placeholder image box; every detection is its own ground truth
    for label in ("bev", "3d"):
        for diff in ("easy", "moderate", "hard"):
            assert res[f"Car_{label}/{diff}_R40"] == 100.0, (label, diff)
    assert "Pedestrian" in text and "Cyclist" in text


# ---- the two-domain dataset -------------------------------------------------------------------------------------------------
NUS_KEY_ROWS = 60_000       # CutMix draws its crop again until it holds more than 10 000 target points


@pytest.fixture(scope="module")
def two_trees(built, tmp_path_factory):
    nus_path = tmp_path_factory.mktemp("nuscenes")
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(nus_cases, "N_KEY", NUS_KEY_ROWS)
        nus_cases.write_tree(nus_path)
    return built[0], nus_path


def mix_cfg(waymo_path, nus_path, mix_type, waymo_classes=("Vehicle",), nus_classes=("car",), joint=("car",), **extra):
    nus = nus_cases.dataset_cfg(nus_path, MAX_SWEEPS=1, SHIFT_COOR=[0.0, 0.0, 1.8], BALANCED_RESAMPLING=False, CLASS_NAMES=list(nus_classes))
    way = cases.dataset_cfg(waymo_path, CLASS_NAMES=list(waymo_classes))
    cfg = {"DATASET": "WaymoNusMixDataset", "CLASS_NAMES": list(joint), "MIX_TYPE": mix_type, "MIX_INC_METHOD": "center", "POLARMIX_PROB": 1.0, "CUTMIX_PROB": 1.0,
           "POLARMIX_RC_NUM": 1, "POLARMIX_DEGREE": 1.570796, "POLARMIX_DIS": "FULL", "POLARMIX_UPDATE_METHOD": ["FIX", "FIX", "FIX"],
           "LASERMIX_NUM_AREAS": 3, "LASERMIX_NUM_ANGLES": 2, "POINT_CLOUD_RANGE": [-25.6, -25.6, -5.0, 25.6, 25.6, 4.8],
           "POINT_FEATURE_ENCODING": {"encoding_type": "absolute_coordinates_encoding", "used_feature_list": ["x", "y", "z", "intensity"],
                                      "src_feature_list": ["x", "y", "z", "intensity", "timestamp"]},
           "DATA_PROCESSOR": nus["DATA_PROCESSOR"], "WaymoDataset": way, "NuScenesDataset": nus}
    cfg.update(extra)
    return AttrDict(cfg)


def test_domain_frames_rename_the_first_class_and_cut_the_boxes(two_trees):
    ds = WaymoNusMixDataset(mix_cfg(*two_trees, "polarmix", waymo_classes=("Vehicle", "Cyclist"), nus_classes=("car", "truck"), joint=("car", "other")),
                            ["car", "other"], training=True)
    assert ds.on_device and len(ds) == 8 + 3 and ds.num_source == 8 and ds.num_target == 3
    assert ds.source.class_names == ["Vehicle", "Cyclist"] and ds.target.class_names == ["car", "truck"] and ds.target.max_sweeps == 1
    src = ds.source_frame(2)
    boxes, names, _ = cases.frame_boxes(2)
    keep = np.isin(names, ["Vehicle", "Cyclist"]) & (cases.points_in_boxes_count(2) > 0)
    assert list(src["gt_names"]) == ["car"] * 5 + ["Cyclist"] and src["gt_boxes"].shape == (6, 8) and same_bits(src["gt_boxes"][:, :7], boxes[keep])
    assert src["gt_boxes"][:, 7].tolist() == [1.0] * 5 + [2.0] and "num_points_in_gt" not in src             # the id of the domain's own list
    rows = cases.frame_rows(2)
    assert src["points"].is_cuda and src["points"].shape == ((rows[:, 5] == -1).sum(), 4) and same_bits(src["points"][:, :3].cpu().numpy(), rows[rows[:, 5] == -1][:, :3])
    tgt = ds.target_frame(1)
    nboxes, nnames = nus_cases.frame_boxes(1)
    nkeep = np.isin(nnames, ["car", "truck"])
    assert list(tgt["gt_names"]) == ["car"] * 15 + ["truck"] and tgt["gt_boxes"].shape == (16, 8) and tgt["gt_boxes"][:, 7].tolist() == [1.0] * 15 + [2.0]
    want = nboxes[nkeep][:, :7].copy()
    want[:, 2] += np.float32(1.8)
    assert np.abs(tgt["gt_boxes"][:, :7] - want).max() < 1e-6 and tgt["shift_coor"] == [0.0, 0.0, 1.8] and np.isfinite(tgt["gt_boxes"]).all()
    assert tgt["points"].is_cuda and tgt["points"].shape[1] == 4 and tgt["points"].shape[0] == NUS_KEY_ROWS + 17 * nus_cases.N_IN_BOX
    ped = WaymoNusMixDataset(mix_cfg(*two_trees, "polarmix", nus_classes=("pedestrian",)), ["car"], training=True).target_frame(1)
    assert list(ped["gt_names"]) == ["car"] and np.isfinite(ped["gt_boxes"]).all() and ped["gt_boxes"].shape == (1, 8)      # its NaN velocity is gone with the columns


def direct_mix(ds, source, target):
    from toda_amd.pcdet.datasets.processor.inter_domain_point_cutmix import inter_domain_point_cutmix
    from toda_amd.pcdet.datasets.processor.inter_domain_point_lasermix import inter_domain_point_lasermix
    from toda_amd.pcdet.datasets.processor.inter_domain_point_polarmix import inter_domain_point_polarmix
    r = ds.point_cloud_range
    if ds.mix_type == "cutmix":
        return inter_domain_point_cutmix(source, target, r, "center")
    if ds.mix_type == "polarmix":
        return inter_domain_point_polarmix(source, target, 1, 1.570796, 0.0, ["FIX", "FIX", "FIX"], r, "FULL", "center", False)
    return inter_domain_point_lasermix(source, target, [-20, 0], 3, 2, r, "center")


@pytest.mark.parametrize("mix_type", ["polarmix", "cutmix", "lasermix"])
def test_mixed_sample_equals_the_processor_on_the_two_prepared_frames(two_trees, mix_type):
    ds = WaymoNusMixDataset(mix_cfg(*two_trees, mix_type), ["car"], training=True)
    assert ds.mix_type == mix_type and ds.mix_prob == 1.0
    index = 9                                                                              # source frame 9 % 8 = 1, target frame 9 % 3 = 0
    np.random.seed(21)
    got = ds[index]
    np.random.seed(21)
    assert np.random.random(1) < 1.0                                                        # the draw against the probability
    source, target = ds.source_frame(1), ds.target_frame(0)
    assert source["frame_id"].startswith(cases.SEQUENCES[0]) and target["metadata"]["token"] == "token0"
    want = ds.data_processor.forward(direct_mix(ds, source, target))
    assert got["points"].is_cuda and got["points"].shape[1] == 4 and same_bits(got["points"].cpu().numpy(), want["points"].cpu().numpy())
    assert got["gt_boxes"].ndim == 2 and got["gt_boxes"].shape[1] == 8 and same_bits(got["gt_boxes"], want["gt_boxes"]) and len(got["gt_boxes"]) > 0
    assert (got["gt_boxes"][:, 7] == 1).all() and "gt_names" not in got
    n_source, n_target = source["points"].shape[0], target["points"].shape[0]
    assert min(n_source, n_target) < got["points"].shape[0] < n_source + n_target           # points of both domains


def test_unmixed_branches_equal_the_single_datasets_frames(two_trees):
    ds = WaymoNusMixDataset(mix_cfg(*two_trees, "polarmix", POLARMIX_PROB=0.0), ["car"], training=False)
    waymo = WaymoDataset(cases.dataset_cfg(two_trees[0], DATA_SPLIT={"train": "train", "test": "val"}), ["Vehicle"], training=False)
    nus = NuScenesDataset(nus_cases.dataset_cfg(two_trees[1], MAX_SWEEPS=1, SHIFT_COOR=[0.0, 0.0, 1.8]), ["car"], training=False)
    assert len(ds) == len(waymo) + len(nus) == 4 + 1
    got, want = ds[2], waymo[2]                                                             # source alone
    assert same_bits(got["points"].cpu().numpy(), want["points"].cpu().numpy()[:, :4]) and same_bits(got["gt_boxes"], want["gt_boxes"])
    assert got["frame_id"] == want["frame_id"] and (got["gt_boxes"][:, 7] == 1).all() and got["gt_boxes"].shape == (6, 8)
    got, want = ds[4], nus[0]                                                               # target alone: index - n_source
    assert got["points"].is_cuda and same_bits(got["points"].cpu().numpy(), want["points"][:, :4]) and same_bits(got["gt_boxes"], want["gt_boxes"])
    assert got["metadata"] == want["metadata"] and got["gt_boxes"].shape == (15, 8) and got["shift_coor"] == [0.0, 0.0, 1.8]


def test_one_stage1_step_through_the_loader(two_trees):
    from toda_amd.pcdet.datasets import build_dataloader
    from toda_amd.pcdet.models import build_network, prepare_batch_on_gpu
    cfg = cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/models/toda_stage1_waymo_nus_polarmix_real.yaml"), AttrDict())
    data = cfg.DATA_CONFIG
    data.POLARMIX_PROB, data.POINT_CLOUD_RANGE = 0.5, [-25.6, -25.6, -5.0, 25.6, 25.6, 4.8]
    data.DATA_PROCESSOR[2].VOXEL_SIZE = [0.1, 0.1, 0.2]
    data.WaymoDataset.DATA_PATH, data.WaymoDataset.SAMPLED_INTERVAL = str(two_trees[0]), AttrDict({"train": 1, "test": 1})
    data.WaymoDataset.pop("OTHER_CHANNEL")
    data.NuScenesDataset.DATA_PATH, data.NuScenesDataset.VERSION = str(two_trees[1]), nus_cases.VERSION
    data.NuScenesDataset.INFO_PATH = AttrDict({"train": ["nuscenes_infos_10sweeps_train.pkl"], "test": ["nuscenes_infos_10sweeps_val.pkl"]})
    cfg.MODEL.BACKBONE_2D.LAYER_NUMS = [1, 1]
    np.random.seed(3)
    torch.manual_seed(3)
    ds, loader, _ = build_dataloader(data, cfg.CLASS_NAMES, batch_size=4, dist=False, workers=2, training=True)
    assert isinstance(ds, WaymoNusMixDataset) and ds.on_device and loader.num_workers == 0 and len(ds) == 8 + 3 and ds.mix_inc_method == "corner_del"
    assert len(ds.source.data_augmentor.data_augmentor_queue) == 3 and len(ds.target.data_augmentor.data_augmentor_queue) == 3     # gt_sampling is disabled
    batch = next(iter(loader))
    assert batch["batch_size"] == 4 and batch["points"].is_cuda and batch["points"].shape[1] == 5 and torch.isfinite(batch["points"]).all()
    assert batch["gt_boxes"].ndim == 3 and batch["gt_boxes"].shape[2] == 8 and np.isfinite(batch["gt_boxes"]).all()
    assert set(np.unique(batch["gt_boxes"][..., 7])) <= {0.0, 1.0} and float(batch["points"][:, 4].max()) <= 1.0      # one class; intensity normalised
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    prepare_batch_on_gpu(batch, net)
    ret, tb, _ = net(batch)
    loss = ret["loss"]
    assert torch.isfinite(loss), tb
    loss.backward()
    grads = [p.grad for p in net.dense_head.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads) and float(sum(g.abs().sum() for g in grads)) > 0
