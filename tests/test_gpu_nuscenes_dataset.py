"""NuScenesDataset on the MI355X: the multi-sweep merge kernel (csrc/nuscenes_frame.hip) against the reference's output
(tests/golden/nuscenes_dataset.npz) and, at its edges, against the numpy route, and the dataset end to end on a mini nuScenes
tree: loader -> collate -> one CenterPoint step, the GT database, the KITTI-style AP.

Every comparison of coordinates is bit for bit.  The kernel's fp64 sum ((x m0 + y m1) + z m2) + m3 and numpy's float64 matrix
product may differ in the last fp64 bit (another order, fused multiply-adds); that reaches the fp32 result only when the sum
lies within that bit of a midpoint between two fp32 values.  The fixture was captured from inputs whose sums are farther than
2^-40 (relative) from every midpoint, and the random inputs made here are filtered by the same condition
(nuscenes_dataset_cases.tie_free, numpy only) before either route sees them."""
import pickle

import numpy as np
import pytest
import torch

from tests import nuscenes_dataset_cases as cases
from toda_amd import ops
from toda_amd.pcdet.datasets.nuscenes.nuscenes_dataset import NuScenesDataset

pytestmark = pytest.mark.gpu
SHIFT = [0.0, 0.0, 1.8]
SENTINEL = -7


@pytest.fixture(scope="module")
def gold():
    return cases.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def merged(rows, offsets, mats, lags, ego, shift=None):
    out, flags = ops.sweeps_merge(rows, offsets, mats, lags, ego, radius=1.0, shift=shift)
    kept = ops.RowBuffer(out.shape[0], 5, out.device).append(out, flags, 1).finish()
    return kept.cpu().numpy(), flags.cpu().numpy(), out.cpu().numpy()


# ---- the kernel against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample,max_sweeps", [(0, 1), (0, 5), (1, 3)])
def test_merge_and_compaction_equal_the_reference_bit_for_bit(gold, sample, max_sweeps):
    rows, offsets, mats, lags, ego = cases.golden_table(gold, sample, max_sweeps)
    want, want_shifted = gold[f"points_{sample}_{max_sweeps}"], gold[f"shifted_{sample}_{max_sweeps}"]
    got, flags, _ = merged(dev(rows), offsets, mats, lags, ego)
    assert flags.dtype == np.int32 and np.array_equal(flags, np.isin(rows[:, 3], want[:, 3]).astype(np.int32))      # column 3 is a unique row id
    assert same_bits(got, want)
    got_shifted, flags_shifted, _ = merged(dev(rows), offsets, mats, lags, ego, shift=SHIFT)
    assert same_bits(got_shifted, want_shifted) and np.array_equal(flags_shifted, flags)
    assert flags.sum() == len(want) and (max_sweeps == 1 or flags.sum() < len(flags))


def test_dataset_samples_equal_the_reference(tmp_path, gold):
    root = tmp_path / cases.VERSION
    root.mkdir()
    with open(root / "infos.pkl", "wb") as f:
        pickle.dump(cases.write_golden_files(root, gold), f)
    wide = [-200.0, -200.0, -10.0, 200.0, 200.0, 10.0]
    for sample, max_sweeps in ((0, 5), (1, 3)):
        cfg = cases.dataset_cfg(tmp_path, INFO_PATH={"train": ["infos.pkl"], "test": ["infos.pkl"]}, POINT_CLOUD_RANGE=wide, MAX_SWEEPS=max_sweeps,
                                SHIFT_COOR=SHIFT)
        ds = NuScenesDataset(cfg, cases.CLASSES, training=False)
        assert ds.on_device
        np.random.seed(int(gold["seed"]))
        points = ds[sample]["points"]
        assert points.is_cuda and same_bits(points.cpu().numpy(), gold[f"shifted_{sample}_{max_sweeps}"])


# ---- edges, against the numpy route on the same files --------------------------------------------------------------------
def rigid(yaw, tilt, t):
    cz, sz, cy, sy = np.cos(yaw), np.sin(yaw), np.cos(tilt), np.sin(tilt)
    m = np.eye(4)
    m[:3, :3] = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    m[:3, 3] = t
    return m


def random_rows(rng, n, matrix=None, inside_ego=False):
    """n raw rows; with a matrix only rows whose transformed coordinates are clear of every fp32 rounding midpoint."""
    m = 2 * n + 16
    r, theta = 0.2 + 50.0 * rng.uniform(0, 1, m) ** 1.5, rng.uniform(-np.pi, np.pi, m)
    rows = np.stack([r * np.cos(theta), r * np.sin(theta), rng.uniform(-3, 2, m), rng.uniform(0, 1, m), rng.integers(0, 32, m)], 1).astype(np.float32)
    if inside_ego:
        rows[:, 0:2] = rng.uniform(-0.999, 0.999, (m, 2)).astype(np.float32)
    if matrix is not None:
        rows = rows[cases.tie_free(rows, matrix)]
    assert len(rows) >= n
    return np.ascontiguousarray(rows[:n])


def both_routes(tmp_path, key, sweeps, shift=None, seed=5):
    """key rows and [(rows, matrix, lag)] written as files of one sample; returns (numpy route, device route through the
    dataset, the sweep table the draw gave: rows, offsets, matrices, lags, drop_ego)."""
    key.tofile(str(tmp_path / "key.pcd.bin"))
    entries = []
    for j, (rows, matrix, lag) in enumerate(sweeps):
        rows.tofile(str(tmp_path / f"s{j}.pcd.bin"))
        entries.append({"lidar_path": f"s{j}.pcd.bin", "transform_matrix": matrix, "time_lag": lag})
    ds = NuScenesDataset.__new__(NuScenesDataset)
    ds.root_path, ds.infos = tmp_path, [{"lidar_path": "key.pcd.bin", "token": "t", "sweeps": entries}]
    np.random.seed(seed)
    want = ds.get_lidar_with_sweeps_host(0, len(sweeps) + 1)
    if shift is not None:
        want[:, 0:3] += np.array(shift, dtype=np.float32)
    np.random.seed(seed)
    got = ds.get_lidar_with_sweeps(0, len(sweeps) + 1, shift=None if shift is None else np.array(shift, np.float32))
    np.random.seed(seed)
    paths, mats, lags, ego = ds._sweep_table(ds.infos[0], len(sweeps) + 1)
    rows, offsets = ds.read_rows(paths)
    return want, got.cpu().numpy(), (rows, offsets, mats, lags, ego)


M1, M2, M3 = rigid(0.4, 0.013, [31.5, -48.2, 0.7]), rigid(-2.1, -0.02, [-66.3, 17.9, -0.35]), rigid(1.3, 0.007, [12.8, 73.4, 1.1])


def test_key_frame_alone(tmp_path):
    rng = np.random.default_rng(1)
    key = random_rows(rng, 300)
    key[:4, 0:2] = [[0.1, 0.2], [-0.5, 0.9], [0.0, 0.0], [0.99, -0.99]]          # inside the ego square: the key frame is not cut
    want, got, (rows, offsets, mats, lags, ego) = both_routes(tmp_path, key, [], shift=SHIFT)
    assert offsets == [0, 300] and mats == [None] and ego == [False]
    assert same_bits(got, want) and len(got) == 300 and (got[:, 4] == 0).all()
    plain, flags, _ = merged(dev(rows), offsets, mats, lags, ego)
    assert same_bits(plain[:, :4], key[:, :4]) and flags.all()                    # no matrix, no shift: x, y, z pass through


@pytest.mark.parametrize("counts", [(1, 255, 256, 257), (257, 0, 1, 256), (3, 0, 0, 2)])
def test_row_counts_at_the_workgroup_edge_and_empty_sweeps(tmp_path, counts):
    rng = np.random.default_rng(sum(counts))
    key = random_rows(rng, counts[0])
    sweeps = [(random_rows(rng, n, m), m, lag) for n, m, lag in zip(counts[1:], (M1, M2, M3), (0.05, 0.45, 0.3))]
    want, got, (rows, offsets, mats, lags, ego) = both_routes(tmp_path, key, sweeps, shift=SHIFT)
    assert offsets[-1] == sum(counts) and sorted(np.diff(offsets).tolist()) == sorted(counts)
    assert same_bits(got, want)
    plain_want, plain_got, _ = both_routes(tmp_path, key, sweeps)
    assert same_bits(plain_got, plain_want)


def test_a_sweep_cut_to_nothing_and_one_without_a_matrix(tmp_path):
    rng = np.random.default_rng(11)
    key = random_rows(rng, 100)
    sweeps = [(random_rows(rng, 70, M1), M1, 0.05), (random_rows(rng, 300, M2, inside_ego=True), M2, 0.1), (random_rows(rng, 90), None, 0.15)]
    want, got, (rows, offsets, mats, lags, ego) = both_routes(tmp_path, key, sweeps)
    assert same_bits(got, want) and np.float32(0.1) not in got[:, 4] and np.float32(0.15) in got[:, 4]
    _, flags, out = merged(dev(rows), offsets, mats, lags, ego)
    cut = lags.index(0.1)
    assert not flags[offsets[cut]:offsets[cut + 1]].any() and (out[offsets[cut]:offsets[cut + 1], 4] == np.float32(0.1)).all()       # written, flagged


def test_the_ego_square_is_open_and_a_nan_row_is_kept(tmp_path):
    rng = np.random.default_rng(12)
    one = np.float32(1.0)
    below = np.nextafter(one, np.float32(0))
    edge = np.array([[1.0, 0.5], [-1.0, -0.3], [0.5, 1.0], [0.2, -1.0], [below, below], [-below, -below], [0.0, 0.0], [1.0, 1.0], [np.nan, 0.0], [0.0, np.nan],
                     [np.nan, np.nan], [5.0, 0.1], [0.1, -5.0]], np.float32)
    keep = [1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1]
    sweep = random_rows(rng, 40, M1)
    sweep[:len(edge), 0:2] = edge
    ok = cases.tie_free(sweep, M1) | np.isnan(sweep[:, :2]).any(1)
    assert ok.all()
    want, got, (rows, offsets, mats, lags, ego) = both_routes(tmp_path, random_rows(rng, 10), [(sweep, M1, 0.05)], shift=SHIFT)
    _, flags, out = merged(dev(rows), offsets, mats, lags, ego, shift=SHIFT)
    assert flags[10:10 + len(edge)].tolist() == keep
    nan_want, nan_got = np.isnan(want), np.isnan(got)
    assert np.array_equal(nan_got, nan_want) and nan_got[:, :3].any(1).sum() == 3 and not nan_got[:, 3:].any()       # kept, and still NaN
    assert same_bits(np.where(nan_got, np.float32(0), got), np.where(nan_want, np.float32(0), want))
    assert np.isnan(out[10 + 8, 0]) and np.isnan(out[10 + 9, 1])


def test_a_view_one_row_into_a_buffer(tmp_path):
    rng = np.random.default_rng(13)
    want, _, (rows, offsets, mats, lags, ego) = both_routes(tmp_path, random_rows(rng, 130), [(random_rows(rng, 200, M3), M3, 0.45)], shift=SHIFT)
    buf = torch.zeros((len(rows) + 1, 5), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[1:] = dev(rows)
    view = buf[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 == 4                       # 20 bytes past a 16-byte boundary
    got, _, _ = merged(view, offsets, mats, lags, ego, shift=SHIFT)
    assert same_bits(got, want)


def test_shift_is_added_in_fp32_after_the_rounding(tmp_path):
    rng = np.random.default_rng(14)
    n = 100_000
    sweep = random_rows(rng, n, M1)
    want, got, _ = both_routes(tmp_path, random_rows(rng, 50), [(sweep, M1, 0.05)], shift=SHIFT)
    assert same_bits(got, want)
    # the inputs tell the two forms apart: folding the shift into the fp64 translation rounds z once instead of twice, which differs
    # on more than 0.5 % of these rows (z' is of the shift's magnitude, so the first rounding is a good part of the second's ulp)
    x, y, z = (sweep[:, c].astype(np.float64) for c in range(3))
    v = ((x * M1[2, 0] + y * M1[2, 1]) + z * M1[2, 2]) + M1[2, 3]
    folded, after = (v + float(np.float32(1.8))).astype(np.float32), v.astype(np.float32) + np.float32(1.8)
    assert (folded != after).mean() > 0.005


def test_bounds_and_bad_arguments():
    from toda_amd import lib as L
    lib = L.load()
    bound = lib.toda_sweeps_merge_max_sweeps()
    assert bound >= 11                                                             # MAX_SWEEPS 10 is the shipped config
    rows = torch.ones((8, 5), dtype=torch.float32, device="cuda")
    out = torch.full((8, 5), float(SENTINEL), dtype=torch.float32, device="cuda")
    flags = torch.full((8,), SENTINEL, dtype=torch.int32, device="cuda")

    def call(n, s, offsets, radius=1.0, table=True, r=rows, o=out, f=flags):
        off, mats, zeros, lags = L.host_i32(offsets), L.host_f64([0.0] * 12 * max(s, 1)), L.host_i32([0] * max(s, 1)), L.host_f64([0.0] * max(s, 1))
        return lib.toda_sweeps_merge(L.ptr(r), n, s, L.hptr(off), L.hptr(mats) if table else None, L.hptr(zeros), L.hptr(zeros), L.hptr(lags), radius,
                                     None, L.ptr(o), L.ptr(f), L.stream())

    assert call(8, bound + 1, [0] * (bound + 1) + [8]) == -1 and b"sweeps, supported are 1 to %d" % bound in lib.toda_last_error()
    assert call(8, 0, [0]) == -1 and call(-1, 1, [0, -1]) == -1
    assert call(8, 2, [0, 4, 7]) == -1 and b"offsets" in lib.toda_last_error()         # does not end at n
    assert call(8, 2, [1, 4, 8]) == -1 and call(8, 3, [0, 9, 5, 8]) == -1               # does not start at 0; decreases
    assert call(8, 1, [0, 8], radius=-1.0) == -1 and call(8, 1, [0, 8], radius=float("nan")) == -1 and b"radius" in lib.toda_last_error()
    assert call(8, 1, [0, 8], table=False) == -1 and b"null" in lib.toda_last_error()
    assert call(8, 1, [0, 8], r=None) == -1 and call(8, 1, [0, 8], o=None) == -1 and call(8, 1, [0, 8], f=None) == -1
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (flags == SENTINEL).all()                       # nothing was launched
    assert call(0, 1, [0, 0], r=None, o=None, f=None) == 0                              # nothing to do
    assert call(8, bound, [0] * bound + [8]) == 0                                       # the bound itself is served
    torch.cuda.synchronize()
    assert (flags == 1).all() and (out[:, :4] == 1).all() and (out[:, 4] == 0).all()
    with pytest.raises(RuntimeError, match="sweeps, supported are 1 to"):
        ops.sweeps_merge(rows, [0] * (bound + 1) + [8], [None] * (bound + 1), [0.0] * (bound + 1), [False] * (bound + 1))
    empty_out, empty_flags = ops.sweeps_merge(torch.zeros((0, 5), device="cuda"), [0, 0, 0], [None, M1], [0.0, 0.05], [False, True])
    assert empty_out.shape == (0, 5) and empty_flags.shape == (0,)
    with pytest.raises(RuntimeError):
        ops.sweeps_merge(torch.zeros((4, 4), device="cuda"), [0, 4], [None], [0.0], [False])      # not five columns
    with pytest.raises(RuntimeError):
        ops.sweeps_merge(torch.zeros((4, 5)), [0, 4], [None], [0.0], [False])                     # a host tensor


# ---- the dataset end to end ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built(tmp_path_factory):
    data_path = tmp_path_factory.mktemp("nuscenes")
    root = cases.write_tree(data_path)
    ds = NuScenesDataset(cases.dataset_cfg(data_path), cases.CLASSES, training=True)
    db = ds.create_groundtruth_database(max_sweeps=cases.TREE_SWEEPS)
    return data_path, root, ds, db


def test_groundtruth_database_counts_the_points_in_the_boxes(built):
    data_path, root, ds, db = built
    with open(root / f"nuscenes_dbinfos_{cases.TREE_SWEEPS}sweeps_withvelo.pkl", "rb") as f:
        stored = pickle.load(f)
    assert sorted(stored) == ["car", "pedestrian", "truck"] and [len(stored[k]) for k in ("car", "pedestrian", "truck")] == [45, 3, 3]
    assert sorted(db) == sorted(stored)
    for k in range(3):
        boxes, names = cases.frame_boxes(k)
        cloud = ds.get_lidar_with_sweeps_host(k, cases.TREE_SWEEPS)                 # both sweeps are drawn, in either order
        owner = ops.points_in_boxes(dev(cloud), dev(boxes[:, :7]), mode=2).cpu().numpy()
        counts = np.bincount(owner[owner >= 0], minlength=len(boxes))
        assert counts.tolist() == [cases.N_IN_BOX + 2 * cases.N_IN_FIRST] + [cases.N_IN_BOX] * 16
        for i, name in enumerate(names):
            rel = f"gt_database_{cases.TREE_SWEEPS}sweeps_withvelo/{k}_{name}_{i}.bin"
            obj = np.fromfile(str(root / rel), np.float32).reshape(-1, 5)
            assert len(obj) == counts[i] and np.abs(obj[:, :3]).max() < 3.6
            info = [e for e in stored[name] if e["image_idx"] == k and e["gt_idx"] == i][0]
            assert info["path"] == rel and info["num_points_in_gt"] == counts[i] and info["box3d_lidar"].shape == (9,)
    first = np.fromfile(str(root / stored["car"][0]["path"]), np.float32).reshape(-1, 5)
    assert sorted(set(first[:, 4].tolist())) == [0.0, float(np.float32(0.05)), float(np.float32(0.1))]      # key frame and both sweeps


def small_model_cfg(data_path):
    import os

    from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = cfg_from_yaml_file(os.path.join(here, "toda_amd/tools/cfgs/models/centerpoint_nuscenes_real.yaml"), AttrDict())
    data = cfg.DATA_CONFIG
    assert data.DATASET == "NuScenesDataset" and data.MAX_SWEEPS == 10 and not data.PRED_VELOCITY
    data.DATA_PATH, data.VERSION, data.MAX_SWEEPS, data.POINT_CLOUD_RANGE = str(data_path), cases.VERSION, cases.TREE_SWEEPS, cases.RANGE
    sampler = data.DATA_AUGMENTOR.AUG_CONFIG_LIST[0]
    assert sampler.NAME == "gt_sampling"
    sampler.DB_INFO_PATH = [f"nuscenes_dbinfos_{cases.TREE_SWEEPS}sweeps_withvelo.pkl"]
    # the tree holds three of the ten classes: with all ten, class-balanced resampling would give each present class
    # int(3 frames * (1 / 10) / (1 / 3)) = 0 frames
    cfg.CLASS_NAMES = ["car", "truck", "pedestrian"]
    cfg.MODEL.DENSE_HEAD.CLASS_NAMES_EACH_HEAD = [["car"], ["truck"], ["pedestrian"]]
    cfg.MODEL.BACKBONE_2D.LAYER_NUMS = [1, 1]
    return cfg


def test_loader_batch_and_one_centerpoint_step(built):
    from toda_amd.pcdet.datasets import build_dataloader
    from toda_amd.pcdet.models import build_network, prepare_batch_on_gpu
    data_path = built[0]
    cfg = small_model_cfg(data_path)
    np.random.seed(0)
    torch.manual_seed(0)
    ds, loader, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, batch_size=2, dist=False, workers=2, training=True)
    assert isinstance(ds, NuScenesDataset) and ds.on_device and loader.num_workers == 0
    assert len(ds) == 9 and len(ds.data_augmentor.data_augmentor_queue[0].db_infos["car"]) == 45     # CBGS: 3 classes x 3 frames; the database is read
    batch = next(iter(loader))
    assert batch["batch_size"] == 2 and batch["points"].is_cuda and batch["points"].shape[1] == 6 and torch.isfinite(batch["points"]).all()
    assert batch["gt_boxes"].ndim == 3 and batch["gt_boxes"].shape[0] == 2 and batch["gt_boxes"].shape[2] == 8 and batch["gt_boxes"].shape[1] >= 10
    assert np.isfinite(batch["gt_boxes"]).all() and set(np.unique(batch["gt_boxes"][..., 7])) <= {0.0, 1.0, 2.0, 3.0}
    assert len(batch["frame_id"]) == 2 and batch["metadata"][0]["token"].startswith("token")
    lags = torch.unique(batch["points"][:, 5]).cpu().numpy()
    assert set(lags.tolist()) == {0.0, float(np.float32(0.05)), float(np.float32(0.1))}
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
    cfg = cases.dataset_cfg(data_path, SHIFT_COOR=SHIFT, INFO_PATH={"train": ["nuscenes_infos_10sweeps_train.pkl"], "test": ["nuscenes_infos_10sweeps_train.pkl"]})
    ds = NuScenesDataset(cfg, cases.CLASSES, training=False)
    samples = [ds[i] for i in range(len(ds))]
    assert len(samples) == 3 and all(s["points"].is_cuda and s["gt_boxes"].shape == (17, 8) for s in samples)
    batch = ds.collate_batch(samples)
    preds = [{"pred_boxes": dev(s["gt_boxes"][:, :7]), "pred_scores": torch.ones(17, device="cuda"), "pred_labels": dev(s["gt_boxes"][:, 7].astype(np.int64))}
             for s in samples]
    annos = ds.generate_prediction_dicts(batch, preds, cases.CLASSES)
    for k, anno in enumerate(annos):
        assert anno["metadata"]["token"] == f"token{k}" and list(anno["name"]) == list(cases.frame_boxes(k)[1])
        assert np.abs(anno["boxes_lidar"] - cases.frame_boxes(k)[0][:, :7]).max() < 1e-6        # SHIFT_COOR undone
    before = pickle.dumps(ds.infos)
    text, res = ds.evaluation(annos, cases.CLASSES, eval_metric="kitti")
    print(text)
    assert pickle.dumps(ds.infos) == before and annos[0]["name"][0] == "car"                     # the evaluator works on copies
    # 45 cars, all Easy under the placeholder image box; every detection is its own ground truth
    for label in ("bev", "3d"):
        for diff in ("easy", "moderate", "hard"):
            assert res[f"Car_{label}/{diff}_R40"] == 100.0, (label, diff)
    assert "Pedestrian" in text and "Truck" in text and "Person_sitting" in text
