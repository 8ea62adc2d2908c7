"""The nuScenes mAP / NDS evaluator on the device: the match kernel against the loop restatement (match table exactly equal, errors
to 1e-12), the prepare kernel against numpy (1e-12 relative, strict range boundary exact), and NuScenesDataset.evaluation(eval_metric=
"nds") end to end on the mini tree."""
import json
import math

import numpy as np
import pytest
import torch

from tests import nusc_eval_cases as C

pytestmark = pytest.mark.gpu

GT_SIZES = (0, 1, 63, 64, 65, 129)
PRED_SIZES = (0, 1, 2, 64, 65, 500)


def run_match(segments):
    from toda_amd import ops
    pred, score, p_attr, gt, g_attr, p_off, g_off, cls = C.pack_segments(segments)
    dev = torch.device("cuda")
    match, err = ops.nusc_eval_match(torch.from_numpy(pred).to(dev), torch.from_numpy(score).to(dev), torch.from_numpy(p_attr).to(dev),
                                     torch.from_numpy(gt).to(dev), torch.from_numpy(g_attr).to(dev), p_off, g_off, cls)
    return match.cpu().numpy(), err.cpu().numpy()


def check(segments, want=None):
    match, err = run_match(segments)
    want_match, want_err = want if want is not None else C.expect_segments(segments)
    assert np.array_equal(match, want_match)
    assert np.array_equal(np.isnan(err), np.isnan(want_err))
    diff = np.abs(err - want_err)[~np.isnan(want_err)]
    print("max |err - restatement| =", diff.max() if diff.size else 0.0)
    assert not diff.size or diff.max() <= 1e-12
    return match, err


@pytest.fixture(scope="module")
def size_grid():
    """Every ground-truth count against every prediction count, the classes in turn (barrier among them), in one launch."""
    rng = np.random.default_rng(11)
    segments = []
    for ng in GT_SIZES:
        for npred in PRED_SIZES:
            name = C.CLASSES[len(segments) % 10]
            span = 3 if ng * npred < 5000 else 6
            segments.append((name, C.grid_boxes(rng, npred, span, True), C.grid_boxes(rng, ng, span, False)))
    return segments, C.expect_segments(segments)


def test_match_kernel_sizes(size_grid):
    size_grid, want = size_grid
    match, err = check(size_grid, want)
    want_match, _ = want
    # the grid does hold what it is there for: equal scores, equal distances, threshold-equal distances, every outcome
    pred, score, _, gt, _, p_off, g_off, _ = C.pack_segments(size_grid)
    ties = exact = 0
    for s in range(len(size_grid)):
        p, g = pred[p_off[s]:p_off[s + 1], :2], gt[g_off[s]:g_off[s + 1], :2]
        if len(p) and len(g):
            d = np.sqrt(((p[:, None] - g[None]) ** 2).sum(-1))
            ties += int((np.sort(d, 1)[:, :-1] == np.sort(d, 1)[:, 1:]).any(1).sum()) if len(g) > 1 else 0
            exact += int(np.isin(d, C.THS).sum())
        assert len(np.unique(score[p_off[s]:p_off[s + 1]])) < max(len(p), 2) or len(p) < 16
    assert ties > 100 and exact > 100
    assert (want_match[0] >= 0).any() and (want_match[3] == -1).any() and (want_match[0] != want_match[3]).any()
    # a ground truth is taken at most once per threshold
    for t in range(4):
        hit = match[t][match[t] >= 0]
        assert len(np.unique(hit)) == len(hit)


def test_match_kernel_hand_cases():
    B = C.hand_box
    segments = [
        # equal scores: the higher index goes first and takes the only ground truth in reach of both
        ("car", [B(0.0, 0.25, 0.5), B(0.0, 0.375, 0.5)], [B(0.0, 0.0)]),
        # equal distances: the lower ground truth wins
        ("car", [B(1.0, 0.0, 0.9)], [B(1.0, 0.25), B(1.0, -0.25), B(0.75, 0.0)]),
        # the nearest ground truth is already taken: the second prediction gets the next one, if it is in reach
        ("truck", [B(0.0, 0.0, 0.9), B(0.125, 0.0, 0.8)], [B(0.0, 0.0), B(1.5, 0.0)]),
        # the nearest ground truth is taken and the nearest free one lies just beyond 0.5 m (0.625): a false positive there that takes
        # nothing, so the third prediction still finds that ground truth free; at 1 m the second prediction takes it
        ("bus", [B(0.0, 0.0, 0.9), B(0.0, 0.125, 0.8), B(0.0, 0.5, 0.7)], [B(0.0, 0.0), B(0.0, 0.75), B(3.0, 0.125)]),
        # distances of exactly 0.5, 1, 2, 4 (axis offsets) and 2.5 (the 3-4-5 triple): equal to the threshold is not a match
        ("pedestrian", [B(10.0, 10.0, 0.9)], [B(10.5, 10.0)]),
        ("pedestrian", [B(10.0, 10.0, 0.9)], [B(10.0, 9.0)]),
        ("pedestrian", [B(10.0, 10.0, 0.9)], [B(8.0, 10.0)]),
        ("pedestrian", [B(10.0, 10.0, 0.9)], [B(10.0, 14.0)]),
        ("pedestrian", [B(10.0, 10.0, 0.9)], [B(11.5, 12.0)]),
        # barrier: period pi, so a barrier turned by pi is no orientation error; a car's is
        ("barrier", [B(0.0, 0.0, 0.9, yaw=0.25)], [B(0.0, 0.0, yaw=0.25 + math.pi)]),
        ("car", [B(0.0, 0.0, 0.9, yaw=0.25)], [B(0.0, 0.0, yaw=0.25 + math.pi)]),
        ("barrier", [B(0.0, 0.0, 0.9, yaw=3.0)], [B(0.0, 0.0, yaw=-3.0)]),
        # attribute: equal, different, none
        ("car", [B(0.0, 0.0, 0.9, attr=1), B(5.0, 0.0, 0.8, attr=1), B(10.0, 0.0, 0.7, attr=1)], [B(0.0, 0.0, attr=1), B(5.0, 0.0, attr=2), B(10.0, 0.0, attr="")]),
    ]
    match, err = check(segments)
    p_off = np.concatenate([[0], np.cumsum([len(s[1]) for s in segments])])
    g_off = np.concatenate([[0], np.cumsum([len(s[2]) for s in segments])])
    local = lambda s, t: [int(m - g_off[s]) if m >= 0 else -1 for m in match[t, p_off[s]:p_off[s + 1]]]     # noqa: E731
    assert local(0, 0) == [-1, 0] and local(0, 3) == [-1, 0]
    assert local(1, 0) == [0] and local(1, 3) == [0]                          # 0.25, 0.25, 0.25 away: index 0
    assert local(2, 0) == [0, -1] and local(2, 1) == [0, -1] and local(2, 2) == [0, 1]   # 1.375 to the free one
    assert local(3, 0) == [0, -1, 1] and local(3, 1) == [0, 1, -1] and local(3, 3) == [0, 1, 2]
    for s, d in ((4, 0.5), (5, 1.0), (6, 2.0), (7, 4.0), (8, 2.5)):
        assert [local(s, t) == [0] for t in range(4)] == [d < th for th in C.THS], (s, d)
    e = lambda s, k=0: err[:, p_off[s] + k]                                                 # noqa: E731
    assert e(4)[0] == 0.5 and e(5)[0] == 1.0 and np.isnan(e(6)).all() and np.isnan(e(8)).all()
    assert abs(e(9)[3]) <= 1e-12 and abs(e(10)[3] - math.pi) <= 1e-12 and abs(e(11)[3] - (2 * math.pi - 6.0)) <= 1e-12
    assert e(12, 0)[4] == 0.0 and e(12, 1)[4] == 1.0 and np.isnan(e(12, 2)[4]) and e(12, 2)[0] == 0.0
    assert e(12, 0)[2] == 0.0 and e(12, 0)[1] == 0.0


def test_match_kernel_700_samples():
    rng = np.random.default_rng(7)
    segments = []
    for s in range(700):
        for name in C.CLASSES:
            segments.append((name, C.grid_boxes(rng, int(rng.integers(0, 5)), 2, True), C.grid_boxes(rng, int(rng.integers(0, 4)), 2, False)))
    check(segments)


def test_match_kernel_twice_same_bits(size_grid):
    size_grid, _ = size_grid
    a, b = run_match(size_grid), run_match(size_grid)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def test_prepare_kernel():
    from toda_amd import ops
    rng = np.random.default_rng(2)
    poses = C.sample_poses()
    G = np.stack([(np.linalg.inv(c) @ np.linalg.inv(r))[:3] for r, c in poses] + [np.eye(4)[:3]])
    ego = np.stack([np.linalg.inv(c)[:3, 3] for r, c in poses] + [np.zeros(3)])
    n = 1500
    rows = np.concatenate([rng.uniform(-60, 60, (n, 2)), rng.uniform(-3, 2, (n, 1)), rng.uniform(0.3, 8, (n, 3)), rng.uniform(-3.2, 3.2, (n, 1)),
                           rng.uniform(-5, 5, (n, 3))], 1)
    rows[::17, 7:9] = np.nan
    sample = rng.integers(0, 3, n).astype(np.int32)
    cls = rng.integers(-1, 11, n).astype(np.int32)
    # the strict boundary under the identity transform (sample 3): exact distances 50, 40, 30 by an axis offset and by 3-4-5
    below = lambda v: float(np.nextafter(v, 0.0))                                            # noqa: E731
    edge = [(0, 50.0, 0.0, 0), (0, below(50.0), 0.0, 1), (4, 30.0, 40.0, 0), (4, 30.0, 39.999, 1), (5, 0.0, -40.0, 0), (5, 0.0, -below(40.0), 1),
            (7, 24.0, 32.0, 0), (8, 30.0, 0.0, 0), (8, below(30.0), 0.0, 1), (9, -18.0, 24.0, 0), (9, -18.0, 23.999, 1), (3, 49.0, 0.0, 1),
            (10, 1.0, 1.0, 0), (-1, 1.0, 1.0, 0)]
    e_rows = np.zeros((len(edge), 10))
    e_rows[:, 0], e_rows[:, 1], e_rows[:, 3:6] = [e[1] for e in edge], [e[2] for e in edge], 1.0
    rows, sample, cls = np.concatenate([rows, e_rows]), np.concatenate([sample, np.full(len(edge), 3, np.int32)]), np.concatenate([cls, np.array([e[0] for e in edge], np.int32)])
    dev = torch.device("cuda")
    out, keep = ops.nusc_eval_prepare(torch.from_numpy(rows).to(dev), torch.from_numpy(sample).to(dev), torch.from_numpy(cls).to(dev),
                                      torch.from_numpy(G).to(dev), torch.from_numpy(ego).to(dev))
    out, keep = out.cpu().numpy(), keep.cpu().numpy()
    Gs, R = G[sample], G[sample][:, :, :3]
    centre = np.einsum("nij,nj->ni", R, rows[:, :3]) + Gs[:, :, 3]
    head = np.einsum("nij,nj->ni", R, np.stack([np.cos(rows[:, 6]), np.sin(rows[:, 6]), np.zeros(len(rows))], 1))
    vel = np.einsum("nij,nj->ni", R, rows[:, 7:10])
    want = np.concatenate([centre, np.arctan2(head[:, 1], head[:, 0])[:, None], vel[:, :2]], 1)
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(out), ~ok) and (~ok).sum() > 0
    rel = np.abs(out[ok] - want[ok]) / np.abs(want[ok]).clip(1e-300)
    print("prepare: max relative error", rel.max())
    np.testing.assert_allclose(out[ok], want[ok], rtol=1e-12, atol=0)
    limit = np.array([C.RANGE[C.CLASSES[c]] if 0 <= c < 10 else -1.0 for c in cls])
    dist = np.sqrt(((centre[:, :2] - ego[sample][:, :2]) ** 2).sum(1))
    decided = np.abs(dist - limit) > 1e-9                        # the random rows: clear of the boundary by far more than rounding
    assert decided[:n].all() and np.array_equal(keep[:n], (dist < limit)[:n].astype(np.int32))
    assert list(keep[n:]) == [e[3] for e in edge]
    assert keep[:n].sum() > 100 and (keep[:n] == 0).sum() > 100
    # nothing to do, and a sample index outside the table
    o, k = ops.nusc_eval_prepare(torch.zeros((0, 10), dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                                 torch.zeros(0, dtype=torch.int32, device=dev), torch.from_numpy(G).to(dev), torch.from_numpy(ego).to(dev))
    assert o.shape == (0, 6) and k.shape == (0,)
    o, k = ops.nusc_eval_prepare(torch.ones((2, 10), dtype=torch.float64, device=dev), torch.tensor([4, -1], dtype=torch.int32, device=dev),
                                 torch.zeros(2, dtype=torch.int32, device=dev), torch.from_numpy(G).to(dev), torch.from_numpy(ego).to(dev))
    assert torch.isnan(o).all() and not k.any()


# ---- end to end
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from toda_amd.pcdet.datasets.nuscenes.nuscenes_dataset import NuScenesDataset
    path = tmp_path_factory.mktemp("nusc_eval")
    C.write_tree(path)
    return path, NuScenesDataset(C.dataset_cfg(path), C.CLASSES, training=False)


def assert_metrics_close(got, want, tol):
    for key in ("label_aps", "label_tp_errors"):
        for name in C.CLASSES:
            for k, v in want[key][name].items():
                g = got[key][name][k]
                assert (math.isnan(g) and math.isnan(v)) or abs(g - v) <= tol, (key, name, k, g, v)
    for key in ("mean_dist_aps", "tp_errors", "tp_scores"):
        for k, v in want[key].items():
            assert abs(got[key][k] - v) <= tol, (key, k, got[key][k], v)
    for key in ("mean_ap", "nd_score"):
        assert abs(got[key] - want[key]) <= tol, (key, got[key], want[key])


def test_perfect_detections_give_the_hand_derived_table(tree):
    """The detections are copies of the ground truths, so each goes through the same arithmetic as its ground truth: distance,
    scale, orientation and velocity errors are exactly 0, and every prediction of a class with ground truth is a TP: precision 1
    at every recall, AP = mean(1 - 0.1) / 0.9 = 1 at all four thresholds.

      with ground truth (5): car (5 in range; the one at 54 m is out and has no prediction: were it counted, recall would stop at
          5/6 and AP would be below 1), truck, pedestrian, motorcycle, traffic_cone
      without (5): bus, trailer, construction_vehicle never occur; the only bicycle stands in the bike rack and the only barrier is
          34.7 m away (limit 30 m), and both ARE among the detections: counted, they would give their classes AP 1.  No
          ground truth: AP 0 and every error 1.
      attr: the car without an attribute is skipped (NaN in a cumulative mean that has numbers); the truck's ground truth says
          vehicle.stopped, a prediction at rest is stated as vehicle.parked: 1.  The pedestrian with NaN velocity has a NaN velocity
          error, skipped next to the other pedestrian's 0.
      NaN by definition: traffic_cone attr / vel / orient, barrier attr / vel.

      mAP = 5 / 10.  trans = scale = (5 x 0 + 5 x 1) / 10 = 0.5.  orient (no cone): (4 x 0 + 5 x 1) / 9.  vel (no cone, barrier):
      (4 x 0 + 4 x 1) / 8 = 0.5.  attr (no cone, barrier): car 0, truck 1, pedestrian 0, motorcycle 0, four classes at 1: 5 / 8.
      NDS = (5 x 0.5 + 0.5 + 0.5 + 4/9 + 0.5 + 3/8) / 10."""
    path, ds = tree
    out = path / "perfect"
    text, res = ds.evaluation(C.perfect_detections(ds.infos), C.CLASSES, eval_metric="nds", output_path=str(out))
    with open(out / "metrics_summary.json") as f:
        m = json.load(f)
    have = ("car", "truck", "pedestrian", "motorcycle", "traffic_cone")
    for name in C.CLASSES:
        for th in ("0.5", "1.0", "2.0", "4.0"):
            assert abs(m["label_aps"][name][th] - (1.0 if name in have else 0.0)) <= 1e-12, (name, th)
        for k, v in m["label_tp_errors"][name].items():
            if name == "traffic_cone" and k in ("attr_err", "vel_err", "orient_err") or name == "barrier" and k in ("attr_err", "vel_err"):
                assert math.isnan(v)
            elif name not in have:
                assert v == 1.0, (name, k)
            elif name == "truck" and k == "attr_err":
                assert v == 1.0
            else:
                assert v == 0.0, (name, k, v)
    want = {"trans_err": 0.5, "scale_err": 0.5, "orient_err": 5 / 9, "vel_err": 0.5, "attr_err": 5 / 8}
    for k, v in want.items():
        assert abs(m["tp_errors"][k] - v) <= 1e-12 and abs(res[k] - v) <= 1e-12
    assert abs(m["mean_ap"] - 0.5) <= 1e-12 and abs(res["mAP"] - 0.5) <= 1e-12
    assert abs(m["nd_score"] - (2.5 + 0.5 + 0.5 + 4 / 9 + 0.5 + 3 / 8) / 10) <= 1e-12 and res["NDS"] == m["nd_score"]
    assert_metrics_close(m, C.restate_evaluation(ds.infos, C.perfect_detections(ds.infos)), 1e-9)
    assert "***car error@trans, scale, orient, vel, attr | AP@0.5, 1.0, 2.0, 4.0" in text and "mAP:\t 0.5000" in text and "NDS:\t 0.4819" in text


def test_perturbed_detections_equal_the_restatement_and_the_files_reload(tree):
    path, ds = tree
    dets = C.perturbed_detections(ds.infos)
    out = path / "perturbed"
    text, res = ds.evaluation(dets, C.CLASSES, eval_metric="nds", output_path=str(out))
    with open(out / "metrics_summary.json") as f:
        m = json.load(f)
    want = C.restate_evaluation(ds.infos, dets)
    for name in C.CLASSES:
        print(name, m["label_aps"][name], m["label_tp_errors"][name])
    assert_metrics_close(m, want, 1e-9)
    assert 0.05 < m["mean_ap"] < 0.95 and any(0 < v < 1 for per in m["label_aps"].values() for v in per.values())      # neither trivial end
    assert res["mAP"] == m["mean_ap"] and res["NDS"] == m["nd_score"] and all(res[k] == m["tp_errors"][k] for k in C.METRICS)
    assert m["eval_time"] > 0
    # the submission file: every detection, in the global frame
    with open(out / "results_nusc.json") as f:
        sub = json.load(f)
    assert sub["meta"] == {"use_camera": False, "use_lidar": True, "use_radar": False, "use_map": False, "use_external": False}
    assert sorted(sub["results"]) == ["sample0", "sample1", "sample2"]
    for det in dets:
        boxes = sub["results"][det["metadata"]["token"]]
        k = int(det["metadata"]["token"][-1])
        info = ds.infos[k]
        G = np.linalg.inv(info["car_from_global"]) @ np.linalg.inv(info["ref_from_car"])
        assert len(boxes) == len(det["name"])
        for i, box in enumerate(boxes):
            b = det["boxes_lidar"][i]
            assert np.allclose(box["translation"], G[:3, :3] @ b[:3] + G[:3, 3], rtol=1e-12, atol=0)
            assert box["size"] == [b[4], b[3], b[5]] and box["detection_name"] == det["name"][i] and box["detection_score"] == det["score"][i]
            Rq = np.array(C.quat_matrix(box["rotation"]))
            want_R = G[:3, :3] @ np.array([[math.cos(b[6]), -math.sin(b[6]), 0], [math.sin(b[6]), math.cos(b[6]), 0], [0, 0, 1]])
            assert np.allclose(Rq, want_R, atol=1e-12)
            assert np.allclose(box["velocity"], (G[:3, :3] @ [b[7], b[8], 0.0])[:2], rtol=1e-12, atol=1e-15)
            assert box["attribute_name"] == C.stated_attribute(box["detection_name"], math.hypot(*box["velocity"]))
    # a second run: the same bits
    text2, res2 = ds.evaluation(dets, C.CLASSES, eval_metric="nds", output_path=str(path / "perturbed2"))
    with open(path / "perturbed2" / "metrics_summary.json") as f:
        m2 = json.load(f)
    m.pop("eval_time"), m2.pop("eval_time")
    assert json.dumps(m) == json.dumps(m2) and text == text2
    assert (out / "results_nusc.json").read_bytes() == (path / "perturbed2" / "results_nusc.json").read_bytes()


def test_filtered_boxes_do_not_count(tree):
    """Detections ONLY on the racked bicycle, the barrier beyond 30 m and the car beyond 50 m: nothing is left to score, every
    AP is 0 - and with them removed from a perfect set nothing changes."""
    path, ds = tree
    dets = C.perfect_detections(ds.infos)
    only = []
    for k, det in enumerate(dets):
        boxes, _, names, _ = C.sample_gt(k)
        pick = {0: [3, 6], 1: [3], 2: []}[k]
        only.append(dict(det, name=names[pick], score=np.full(len(pick), 0.9), boxes_lidar=boxes[pick].astype(np.float64), pred_labels=np.ones(len(pick), np.int64)))
    _, res = ds.evaluation(only, C.CLASSES, eval_metric="nds", output_path=str(path / "only"))
    assert res["mAP"] == 0.0 and all(res[k] == 1.0 for k in C.METRICS) and res["NDS"] == 0.0
    without = []
    for k, det in enumerate(dets):
        keep = [i for i, n in enumerate(det["name"]) if n not in ("bicycle", "barrier")]
        without.append(dict(det, name=det["name"][keep], score=det["score"][keep], boxes_lidar=det["boxes_lidar"][keep], pred_labels=det["pred_labels"][keep]))
    _, a = ds.evaluation(dets, C.CLASSES, eval_metric="nds", output_path=str(path / "with"))
    _, b = ds.evaluation(without, C.CLASSES, eval_metric="nds", output_path=str(path / "without"))
    assert a == b


def test_refused_inputs_and_infos_without_ground_truth(tree, tmp_path):
    from toda_amd.pcdet.datasets.nuscenes.nuscenes_dataset import NuScenesDataset
    path, ds = tree
    dets = C.perfect_detections(ds.infos)
    many = dict(dets[1], name=np.array(["car"] * 501), score=np.full(501, 0.5), boxes_lidar=np.zeros((501, 9)), pred_labels=np.ones(501, np.int64))
    with pytest.raises(ValueError, match="sample1.*501"):
        ds.evaluation([dets[0], many, dets[2]], C.CLASSES, eval_metric="nds", output_path=str(tmp_path / "o"))
    with pytest.raises(ValueError, match="exactly"):
        ds.evaluation(dets[:2], C.CLASSES, eval_metric="nds", output_path=str(tmp_path / "o"))
    # exactly 500 predictions in one sample and one class are served
    full = dict(dets[1], name=np.array(["car"] * 500), score=np.linspace(0.9, 0.1, 500), boxes_lidar=np.tile(dets[1]["boxes_lidar"][:1], (500, 1)),
                pred_labels=np.ones(500, np.int64))
    _, res = ds.evaluation([dets[0], full, dets[2]], C.CLASSES, eval_metric="nds", output_path=str(tmp_path / "full"))
    assert 0 < res["mAP"] < 0.5
    # infos without gt_boxes, and the test split: the submission is written, nothing is scored
    C.write_tree(tmp_path / "nogt", with_gt=False)
    blind = NuScenesDataset(C.dataset_cfg(tmp_path / "nogt"), C.CLASSES, training=False)
    assert blind.evaluation(dets, C.CLASSES, eval_metric="nds", output_path=str(tmp_path / "blind")) == ("No ground-truth annotations for evaluation", {})
    assert (tmp_path / "blind" / "results_nusc.json").exists() and not (tmp_path / "blind" / "metrics_summary.json").exists()
    (tmp_path / "t").mkdir()
    (tmp_path / "t" / "v1.0-test").mkdir()
    (tmp_path / "t" / "v1.0-test" / "nuscenes_infos_10sweeps_val.pkl").write_bytes((path / C.VERSION / "nuscenes_infos_10sweeps_val.pkl").read_bytes())
    test_split = NuScenesDataset(C.dataset_cfg(tmp_path / "t", version="v1.0-test"), C.CLASSES, training=False)
    assert test_split.evaluation(dets, C.CLASSES, eval_metric="nds", output_path=str(tmp_path / "ts"))[0] == "No ground-truth annotations for evaluation"
    with open(tmp_path / "ts" / "results_nusc.json") as f:
        assert sum(len(v) for v in json.load(f)["results"].values()) == sum(len(d["name"]) for d in dets)


def test_tools_test_reports_map_and_nds_for_the_nuscenes_config(tmp_path):
    """tools.test with EVAL_METRIC nds on centerpoint_nuscenes_real.yaml (untrained weights, the LiDAR tree of the dataset tests with
    the two poses added to its infos and the four tables written for its ground truths): the report carries every mean, mAP and NDS."""
    import os
    import pickle

    from tests import nuscenes_dataset_cases as D
    from toda_amd.tools import test as tester
    root = D.write_tree(tmp_path)
    pkl = root / "nuscenes_infos_10sweeps_val.pkl"
    with open(pkl, "rb") as f:
        infos = pickle.load(f)
    poses = C.sample_poses()
    tables = {"attribute": [{"token": "attr_p", "name": "vehicle.parked"}], "category": [{"token": "cat_any", "name": "vehicle.car"}],
              "instance": [{"token": "inst_any", "category_token": "cat_any"}], "sample_annotation": []}
    for k, info in enumerate(infos):
        info["ref_from_car"], info["car_from_global"] = poses[k % 3]
        for tok, name in zip(info["gt_boxes_token"], info["gt_names"]):
            tables["sample_annotation"].append({"token": str(tok), "sample_token": info["token"], "instance_token": "inst_any",
                                                "attribute_tokens": ["attr_p"] if name != "pedestrian" else [], "translation": [0.0, 0.0, 0.0],
                                                "size": [1.0, 1.0, 1.0], "rotation": [1.0, 0.0, 0.0, 0.0]})
    with open(pkl, "wb") as f:
        pickle.dump(infos, f)
    (root / D.VERSION).mkdir()
    for name, rows in tables.items():
        with open(root / D.VERSION / f"{name}.json", "w") as f:
            json.dump(rows, f)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "out"
    ret = tester.main(["--cfg_file", os.path.join(here, "toda_amd/tools/cfgs/models/centerpoint_nuscenes_real.yaml"), "--batch_size", "1",
                       "--output_dir", str(out), "--set", "DATA_CONFIG.DATA_PATH", str(tmp_path), "DATA_CONFIG.VERSION", D.VERSION,
                       "DATA_CONFIG.MAX_SWEEPS", str(D.TREE_SWEEPS), "DATA_CONFIG.POINT_CLOUD_RANGE", str(D.RANGE).replace(" ", ""),
                       "MODEL.POST_PROCESSING.EVAL_METRIC", "nds"])
    for key in C.METRICS + ["mAP", "NDS"]:
        assert key in ret and 0.0 <= ret[key] <= 1.0 + 1e-12, key
    assert "Car_3d/moderate_R40" not in ret
    summary = sorted(out.rglob("metrics_summary.json"))
    assert len(summary) == 1 and (summary[0].parent / "results_nusc.json").exists()
    with open(summary[0]) as f:
        m = json.load(f)
    assert m["mean_ap"] == ret["mAP"] and m["nd_score"] == ret["NDS"] and sorted(m["label_aps"]) == sorted(C.CLASSES)
    log = "".join(p.read_text() for p in out.rglob("log_eval_*.txt"))
    assert "***car error@trans, scale, orient, vel, attr | AP@0.5, 1.0, 2.0, 4.0" in log and "mAP:\t" in log and "NDS:\t" in log
