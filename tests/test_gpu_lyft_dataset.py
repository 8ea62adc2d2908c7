"""LyftDataset on the MI355X: toda_sweeps_merge_rect (csrc/nuscenes_frame.hip) against the reference's own clouds
(tests/golden/lyft_dataset.npz), against toda_sweeps_merge and against the numpy route, and the dataset end to end on a mini Lyft
tree: GT database, loader -> one CenterPoint step -> one evaluation pass, the KITTI-style AP and the Lyft mAP.

Every comparison of coordinates is bit for bit (a NaN only has to be a NaN): the fixture and the tree's files hold only rows whose
fp64 sums lie clear of every fp32 rounding midpoint (nuscenes_dataset_cases.tie_free), so the kernel's summation order and numpy's
round alike."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import lyft_dataset_cases as cases
from toda_amd import ops
from toda_amd.pcdet.datasets.lyft.lyft_dataset import EGO_RADIUS_X, EGO_RADIUS_Y, LyftDataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7


@pytest.fixture(scope="module")
def gold():
    return cases.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def merged(rows, offsets, mats, lags, ego, rx=EGO_RADIUS_X, ry=EGO_RADIUS_Y, shift=None):
    out, flags = ops.sweeps_merge_rect(rows, offsets, mats, lags, ego, rx, ry, shift=shift)
    kept = ops.RowBuffer(out.shape[0], 5, out.device).append(out, flags, 1).finish()
    return kept.cpu().numpy(), flags.cpu().numpy(), out.cpu().numpy()


# ---- the kernel against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample,max_sweeps", [(0, 1), (0, 5), (1, 3), (1, 1)])
def test_merge_and_compaction_equal_the_reference_bit_for_bit(gold, sample, max_sweeps):
    rows, offsets, mats, lags, ego = cases.golden_table(gold, sample, max_sweeps)
    want = gold[f"points_{sample}_{max_sweeps}"]
    got, flags, out = merged(dev(rows), offsets, mats, lags, ego)
    assert cases.same_bits_nan_aware(got, want)
    assert flags.dtype == np.int32 and flags.sum() == len(want) and flags[:offsets[1]].all()                       # the key frame is never cut
    assert out.shape == rows.shape and (max_sweeps == 1 or flags.sum() < len(flags))
    if max_sweeps == 5:
        # the repeated sweep is there twice, and rows between the nuScenes square and this rectangle (1 <= |x| < 1.5) are cut
        ids, counts = np.unique(got[:, 3], return_counts=True)
        f3 = cases.golden_rows(gold, 3)
        assert set(counts[np.isin(ids, f3[:, 3])].tolist()) == {2}
        f2 = cases.golden_rows(gold, 2)
        between = (np.abs(f2[:, 0]) >= 1.0) & (np.abs(f2[:, 0]) < 1.5) & (np.abs(f2[:, 1]) < 1.0)
        assert between.sum() >= 3 and not np.isin(f2[between, 3], ids).any()


def test_dataset_samples_equal_the_reference(tmp_path, gold):
    root = tmp_path / cases.VERSION
    root.mkdir()
    with open(root / "infos.pkl", "wb") as f:
        pickle.dump(cases.write_golden_files(root, gold), f)
    wide = [-200.0, -200.0, -10.0, 200.0, 200.0, 10.0]
    for sample, max_sweeps in ((0, 5), (1, 3)):
        cfg = cases.dataset_cfg(tmp_path, INFO_PATH={"train": ["infos.pkl"], "test": ["infos.pkl"]}, POINT_CLOUD_RANGE=wide, MAX_SWEEPS=max_sweeps)
        ds = LyftDataset(cfg, cases.CLASSES, training=False)
        assert ds.on_device
        np.random.seed(int(gold["seed"]))
        cloud = ds.get_lidar_with_sweeps(sample, max_sweeps)
        assert cloud.is_cuda and cases.same_bits_nan_aware(cloud.cpu().numpy(), gold[f"points_{sample}_{max_sweeps}"])
        np.random.seed(int(gold["seed"]))
        points = ds[sample]["points"]                                                     # the range mask drops the NaN rows, nothing else
        want = gold[f"points_{sample}_{max_sweeps}"]
        want = want[~np.isnan(want).any(1)]
        assert points.is_cuda and points.cpu().numpy().tobytes() == want.tobytes()


def test_equal_half_sides_are_the_square_of_sweeps_merge(gold):
    rng = np.random.default_rng(5)
    rows, offsets, mats, lags, ego = cases.golden_table(gold, 0, 5)
    near = rng.uniform(-2.0, 2.0, (4000, 5)).astype(np.float32)                          # a band around every radius below
    rows = np.concatenate([rows, near])
    offsets, mats, lags, ego = offsets + [len(rows)], mats + [gold["matrices"][3]], lags + [0.3], ego + [True]
    for r in (1.0, 1.5, 0.0, 0.37):
        for shift in (None, [0.0, 0.0, 1.8]):
            a_out, a_flags = ops.sweeps_merge(dev(rows), offsets, mats, lags, ego, radius=r, shift=shift)
            b_out, b_flags = ops.sweeps_merge_rect(dev(rows), offsets, mats, lags, ego, r, r, shift=shift)
            assert torch.equal(a_flags, b_flags) and a_out.cpu().numpy().tobytes() == b_out.cpu().numpy().tobytes()
            assert r == 0.0 or 0 < int((a_flags == 0).sum()) < len(rows)
    wide, _ = ops.sweeps_merge_rect(dev(rows), offsets, mats, lags, ego, 1.5, 1.0)[1], None
    square = ops.sweeps_merge(dev(rows), offsets, mats, lags, ego, radius=1.0)[1]
    assert int(wide.sum()) < int(square.sum())                                            # the rectangle cuts more than the unit square


def test_placed_rows_on_the_device(tmp_path):
    """The rows placed for the cut: on a side (kept), one ulp inside (dropped), between square and rectangle (dropped), NaN (kept);
    with drop_ego off (the key frame) all are kept."""
    xy = np.array([p for p, _ in cases.EGO_ROWS], np.float32)
    keep = [k for _, k in cases.EGO_ROWS]
    rows = np.concatenate([xy, np.full((len(xy), 1), -1.0, np.float32), np.arange(len(xy), dtype=np.float32)[:, None], np.zeros((len(xy), 1), np.float32)], 1)
    both = np.concatenate([rows, rows])
    _, flags, out = merged(dev(both), [0, len(rows), 2 * len(rows)], [None, None], [0.0, 0.1], [False, True])
    assert flags[:len(rows)].all() and flags[len(rows):].tolist() == keep
    assert cases.same_bits_nan_aware(out[:, :4], both[:, :4]) and (out[len(rows):, 4] == np.float32(0.1)).all()          # written for every row


def test_bounds_and_bad_arguments():
    from toda_amd import lib as L
    lib = L.load()
    bound = lib.toda_sweeps_merge_max_sweeps()
    rows = torch.ones((8, 5), dtype=torch.float32, device="cuda")
    out = torch.full((8, 5), float(SENTINEL), dtype=torch.float32, device="cuda")
    flags = torch.full((8,), SENTINEL, dtype=torch.int32, device="cuda")

    def call(n, s, offsets, rx=1.5, ry=1.0, table=True, r=rows, o=out, f=flags):
        off, mats, zeros, lags = L.host_i32(offsets), L.host_f64([0.0] * 12 * max(s, 1)), L.host_i32([0] * max(s, 1)), L.host_f64([0.0] * max(s, 1))
        return lib.toda_sweeps_merge_rect(L.ptr(r), n, s, L.hptr(off), L.hptr(mats) if table else None, L.hptr(zeros), L.hptr(zeros), L.hptr(lags), rx, ry,
                                          None, L.ptr(o), L.ptr(f), L.stream())

    assert call(8, bound + 1, [0] * (bound + 1) + [8]) == -1 and b"sweeps, supported are 1 to %d" % bound in lib.toda_last_error()
    assert call(8, 0, [0]) == -1 and call(-1, 1, [0, -1]) == -1
    assert call(8, 2, [0, 4, 7]) == -1 and b"offsets" in lib.toda_last_error()
    assert call(8, 2, [1, 4, 8]) == -1 and call(8, 3, [0, 9, 5, 8]) == -1
    assert call(8, 1, [0, 8], rx=-1.0) == -1 and call(8, 1, [0, 8], ry=float("nan")) == -1 and b"half-sides" in lib.toda_last_error()
    assert call(8, 1, [0, 8], table=False) == -1 and b"null" in lib.toda_last_error()
    assert call(8, 1, [0, 8], r=None) == -1 and call(8, 1, [0, 8], o=None) == -1 and call(8, 1, [0, 8], f=None) == -1
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (flags == SENTINEL).all()                          # nothing was launched
    assert call(0, 1, [0, 0], r=None, o=None, f=None) == 0
    assert call(8, bound, [0] * bound + [8]) == 0
    torch.cuda.synchronize()
    assert (flags == 1).all() and (out[:, :4] == 1).all() and (out[:, 4] == 0).all()
    with pytest.raises(RuntimeError, match="sweeps_merge_rect: rows must be"):
        ops.sweeps_merge_rect(torch.zeros((4, 4), device="cuda"), [0, 4], [None], [0.0], [False], 1.5, 1.0)
    with pytest.raises(RuntimeError):
        ops.sweeps_merge_rect(torch.zeros((4, 5)), [0, 4], [None], [0.0], [False], 1.5, 1.0)          # a host tensor


# ---- the dataset end to end ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built(tmp_path_factory):
    data_path = tmp_path_factory.mktemp("lyft")
    root = cases.write_tree(data_path)
    ds = LyftDataset(cases.dataset_cfg(data_path), cases.CLASSES, training=True)
    db = ds.create_groundtruth_database(max_sweeps=cases.TREE_SWEEPS)
    return data_path, root, ds, db


def test_device_cloud_equals_the_numpy_route_on_every_frame(built):
    data_path, root, ds, _ = built
    for training in (True, False):
        split = LyftDataset(cases.dataset_cfg(data_path), cases.CLASSES, training=training)
        for k in range(len(split)):
            np.random.seed(10 + k)
            want = split.get_lidar_with_sweeps_host(k, cases.TREE_SWEEPS)
            np.random.seed(10 + k)
            got = split.get_lidar_with_sweeps(k, cases.TREE_SWEEPS)
            assert got.is_cuda and cases.same_bits_nan_aware(got.cpu().numpy(), want)          # the same rows in the same order
            assert np.isnan(want[:, :2]).any(1).sum() >= 6


def test_groundtruth_database_round_trip(built):
    data_path, root, ds, db = built
    with open(root / f"lyft_dbinfos_{cases.TREE_SWEEPS}sweeps.pkl", "rb") as f:
        stored = pickle.load(f)
    assert sorted(stored) == ["car", "pedestrian", "truck"] and [len(stored[k]) for k in ("car", "pedestrian", "truck")] == [30, 2, 2]
    assert sorted(db) == sorted(stored)
    for k in range(2):
        boxes, names = cases.frame_boxes(k)
        cloud = ds.get_lidar_with_sweeps_host(k, cases.TREE_SWEEPS)
        cloud = cloud[~np.isnan(cloud).any(1)]
        owner = ops.points_in_boxes(dev(cloud), dev(boxes), mode=2).cpu().numpy()
        counts = np.bincount(owner[owner >= 0], minlength=len(boxes))
        files = 3 if k == 1 else 4                                                        # sweep entries with rows: frame 1 has an empty file
        assert counts.tolist() == [cases.N_IN_BOX + files * cases.N_IN_FIRST] + [cases.N_IN_BOX] * 16
        for i, name in enumerate(names):
            rel = f"gt_database/{k}_{name}_{i}.bin"
            obj = np.fromfile(str(root / rel), np.float32).reshape(-1, 5)
            assert len(obj) == counts[i] and np.abs(obj[:, :3]).max() < 3.6
            info = [e for e in stored[name] if e["image_idx"] == k and e["gt_idx"] == i][0]
            assert info["path"] == rel and info["num_points_in_gt"] == counts[i] and info["box3d_lidar"].shape == (7,)


def test_ground_truth_fed_back_scores_full_marks_in_both_metrics(built):
    data_path = built[0]
    cfg = cases.dataset_cfg(data_path, INFO_PATH={"train": ["lyft_infos_train.pkl"], "test": ["lyft_infos_train.pkl", "lyft_infos_val.pkl"]})
    ds = LyftDataset(cfg, cases.CLASSES, training=False)
    np.random.seed(0)
    samples = [ds[i] for i in range(len(ds))]
    assert len(samples) == 3 and all(s["points"].is_cuda and s["gt_boxes"].shape == (17, 8) for s in samples)
    batch = ds.collate_batch(samples)
    preds = [{"pred_boxes": dev(s["gt_boxes"][:, :7]), "pred_scores": torch.linspace(0.9, 0.2, 17, device="cuda"), "pred_labels": dev(s["gt_boxes"][:, 7].astype(np.int64))}
             for s in samples]
    annos = ds.generate_prediction_dicts(batch, preds, cases.CLASSES)
    for k, anno in enumerate(annos):
        assert anno["metadata"]["token"] == f"token{k}" and sorted(anno["name"]) == sorted(cases.frame_boxes(k)[1])
        assert anno["pred_labels"].tolist() == [cases.CLASSES.index(n) + 1 for n in anno["name"]]
    before = pickle.dumps(ds.infos)
    text, res = ds.evaluation(annos, ["car", "pedestrian", "truck"], eval_metric="lyft")
    print(text)
    assert res["car"] == pytest.approx(1.0, abs=1e-12) and res["pedestrian"] == pytest.approx(1.0, abs=1e-12) and res["truck"] == pytest.approx(1.0, abs=1e-12)
    assert res["mAP"] == pytest.approx(1.0, abs=1e-12) and text.startswith("----------------Lyft trainval results")
    # all nine classes: the six without boxes score 0 and enter the mean
    text9, res9 = ds.evaluation(annos, cases.CLASSES, eval_metric="lyft")
    assert res9["mAP"] == pytest.approx(3 / 9, abs=1e-12) and res9["animal"] == 0.0
    # a car moved by half its length: IoU 1 / 3, a TP at no cut-off -> one of 45 cars is missed, one prediction is false
    moved = pickle.loads(pickle.dumps(annos))
    first_car = list(moved[0]["name"]).index("car")
    moved[0]["boxes_lidar"][first_car, 0] += 2.0
    _, res_moved = ds.evaluation(moved, ["car"], eval_metric="lyft")
    assert 0.9 < res_moved["car"] < 1.0
    ktext, kres = ds.evaluation(annos, ["car", "pedestrian", "truck"], eval_metric="kitti")
    assert pickle.dumps(ds.infos) == before and annos[0]["name"].dtype.kind == "U"          # the evaluators work on copies
    for label in ("bev", "3d"):
        assert np.isfinite(kres[f"Car_{label}/easy_R40"]) and kres[f"Car_{label}/easy_R40"] > 90.0
    assert "Pedestrian" in ktext and "Truck" in ktext


def small_model_cfg(data_path):
    from toda_amd.pcdet.config import AttrDict, cfg_from_yaml_file
    cwd = os.getcwd()
    os.chdir(os.path.join(ROOT, "toda_amd", "tools"))
    try:
        cfg = cfg_from_yaml_file(os.path.join(ROOT, "toda_amd/tools/cfgs/models/centerpoint_lyft_real.yaml"), AttrDict())
    finally:
        os.chdir(cwd)
    data = cfg.DATA_CONFIG
    assert data.DATASET == "LyftDataset" and data.MAX_SWEEPS == 5 and cfg.MODEL.POST_PROCESSING.EVAL_METRIC == "lyft"
    data.DATA_PATH, data.POINT_CLOUD_RANGE = str(data_path), cases.RANGE
    sampler = data.DATA_AUGMENTOR.AUG_CONFIG_LIST[0]
    assert sampler.NAME == "gt_sampling" and list(sampler.DB_INFO_PATH) == ["lyft_dbinfos_5sweeps.pkl"]
    sampler.PREPARE.filter_by_min_points = ["car:5", "pedestrian:5", "truck:5"]           # the tree holds three of the nine classes
    sampler.SAMPLE_GROUPS = ["car:3", "pedestrian:3", "truck:3"]
    cfg.MODEL.BACKBONE_2D.LAYER_NUMS = [1, 1]
    cfg.MODEL.DENSE_HEAD.POST_PROCESSING.SCORE_THRESH = 0.0                              # an untrained head: keep what it predicts
    cfg.MODEL.DENSE_HEAD.POST_PROCESSING.POST_CENTER_LIMIT_RANGE = [-30.0, -30.0, -10.0, 30.0, 30.0, 10.0]
    cfg.LOCAL_RANK = 0
    return cfg


def one_step_and_one_eval(data_path, out_dir):
    import logging

    from toda_amd.pcdet.datasets import build_dataloader
    from toda_amd.pcdet.models import build_network, prepare_batch_on_gpu
    from toda_amd.tools.eval_utils import eval_utils
    cfg = small_model_cfg(data_path)
    np.random.seed(0)
    torch.manual_seed(0)
    ds, loader, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, batch_size=2, dist=False, workers=2, training=True)
    assert isinstance(ds, LyftDataset) and ds.on_device and loader.num_workers == 0 and len(ds) == 2
    assert len(ds.data_augmentor.data_augmentor_queue[0].db_infos["car"]) == 30
    batch = next(iter(loader))
    assert batch["batch_size"] == 2 and batch["points"].is_cuda and batch["points"].shape[1] == 6 and torch.isfinite(batch["points"]).all()
    assert batch["gt_boxes"].ndim == 3 and batch["gt_boxes"].shape[2] == 8 and batch["gt_boxes"].shape[1] >= 17
    assert batch["metadata"][0]["token"].startswith("token")
    net = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).cuda().train()
    prepare_batch_on_gpu(batch, net)
    ret, tb, _ = net(batch)
    loss = ret["loss"]
    assert torch.isfinite(loss), tb
    loss.backward()
    grads = [p.grad for p in net.dense_head.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads) and float(sum(g.abs().sum() for g in grads)) > 0
    test_set, test_loader, _ = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, batch_size=1, dist=False, workers=0, training=False)
    np.random.seed(1)
    result = eval_utils.eval_one_epoch(cfg, net, test_loader, 0, logging.getLogger("lyft-test"), result_dir=out_dir)
    return float(loss.detach()), result


def test_one_centerpoint_step_and_one_evaluation_pass_are_finite_and_repeat(built, tmp_path):
    data_path = built[0]
    loss_a, res_a = one_step_and_one_eval(data_path, tmp_path / "a")
    loss_b, res_b = one_step_and_one_eval(data_path, tmp_path / "b")
    assert np.isfinite(loss_a) and loss_a == loss_b
    assert set(cases.CLASSES) <= set(res_a) and "mAP" in res_a and all(np.isfinite(res_a[k]) for k in res_a)
    assert all(-1.0 <= res_a[c] <= 1.0 for c in cases.CLASSES) and res_a == res_b
    with open(tmp_path / "a" / "result.pkl", "rb") as f:
        annos = pickle.load(f)
    assert len(annos) == 1 and annos[0]["metadata"] == {"token": "token2"} and len(annos[0]["name"]) > 0 and "pred_labels" in annos[0]
