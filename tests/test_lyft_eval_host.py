"""The Lyft mAP without a GPU: the numpy / Python restatement (tests/lyft_eval_cases.py) against hand-computed cases, the table
loader and its grouping, the global-frame rows under a tilted pose, the numpy route of the evaluator against the restatement,
the report text, and the argument checks and size queries of the new exports."""
import json

import numpy as np
import pytest

from tests import lyft_eval_cases as C
from toda_amd import lib as L
from toda_amd.pcdet.datasets.lyft import lyft_eval as E

IDENT = [1.0, 0.0, 0.0, 0.0]


def box(x, y, z, w, l, h, rotation=IDENT, token="s", name="car", **extra):
    return {"sample_token": token, "translation": [x, y, z], "size": [w, l, h], "rotation": list(rotation), "name": name, **extra}


def iou(a, b):
    return C.Box3D(**a).get_iou(C.Box3D(**b))


# ---- the restatement against hand-computed cases -------------------------------------------------------------------------
def test_axis_aligned_pairs_have_their_closed_form_iou():
    # identity rotation: length along x, width along y.  4 x 2 x 1 boxes shifted by (1, 0.5, 0.25): 3 * 1.5 * 0.75 over 16 - that
    a, b = box(0, 0, 0, 2, 4, 1), box(1, 0.5, 0.25, 2, 4, 1)
    inter = 3 * 1.5 * 0.75
    assert iou(a, b) == pytest.approx(inter / (16 - inter), abs=1e-15)
    # a quarter turn swaps the footprint: 2 x 4 against 4 x 2 at one centre overlap in a 2 x 2 square
    q = C.quat_axis([0, 0, 1], np.pi / 2)
    assert iou(a, box(0, 0, 0, 2, 4, 1, rotation=q)) == pytest.approx(4 / (8 + 8 - 4), abs=1e-15)
    # a small box inside a large one: the ratio of the volumes
    assert iou(box(0.3, -0.2, 0.1, 1, 1, 1), box(0, 0, 0, 4, 6, 2)) == pytest.approx(1 / 48, abs=1e-15)
    # 45 degrees: a unit square turned inside a square of side 2 stays inside
    assert iou(box(0, 0, 0, 1, 1, 1, rotation=C.quat_axis([0, 0, 1], np.pi / 4)), box(0, 0, 0, 2, 2, 1)) == pytest.approx(1 / 4, abs=1e-15)
    # two unit squares at 45 degrees about one centre: a regular octagon of area 2 (sqrt 2 - 1)
    octagon = 2 * (np.sqrt(2) - 1)
    assert iou(box(0, 0, 0, 1, 1, 1, rotation=C.quat_axis([0, 0, 1], np.pi / 4)), box(0, 0, 0, 1, 1, 1)) == pytest.approx(octagon / (2 - octagon), abs=1e-14)


def test_a_box_against_itself_disjoint_boxes_and_a_shared_edge():
    a = box(120.5, -310.25, 3.0, 1.9, 4.6, 1.7, rotation=C.quat_axis([0, 0, 1], 0.7))
    assert iou(a, a) == pytest.approx(1.0, abs=1e-12) and iou(a, a) <= 1.0
    # tilted, a box misses itself: the footprint shrinks by n = c^2 + s^2 while the volume stays, so IoU = n / (2 - n)
    q = C.quat_ypr(0.7, 0.02, -0.03)
    rot = C.quat_matrix(q)
    n = rot[0, 0] ** 2 + rot[1, 0] ** 2
    tilted = box(120.5, -310.25, 3.0, 1.9, 4.6, 1.7, rotation=q)
    assert n < 1 and iou(tilted, tilted) == pytest.approx(n / (2 - n), abs=1e-12)
    assert iou(box(0, 0, 0, 2, 4, 1), box(10, 0, 0, 2, 4, 1)) == 0.0
    assert iou(box(0, 0, 0, 2, 4, 1), box(4, 0, 0, 2, 4, 1)) == 0.0             # the faces x = 2 touch: a segment has no area
    assert iou(box(0, 0, 0, 2, 4, 1), box(0, 0, 1, 2, 4, 1)) == 0.0             # stacked: the z intervals share one point
    assert iou(box(0, 0, 0, 2, 4, 1), box(0, 0, 5, 2, 4, 1)) == 0.0


def test_a_tilted_box_has_a_shrunk_footprint_and_its_full_volume():
    # pitch p: the rotation's first column is (cos p, 0, -sin p), so c = cos p, s = 0; the footprint is l cos p by w cos p
    p = 0.5
    tilted = box(0, 0, 0, 2, 4, 1, rotation=C.quat_axis([0, 1, 0], p))
    inter = (4 * np.cos(p)) * (2 * np.cos(p)) * 1
    assert iou(tilted, box(0, 0, 0, 2, 4, 1)) == pytest.approx(inter / (8 + 8 - inter), abs=1e-14)


def test_a_three_point_pr_curve():
    # three predictions by score: TP, FP, TP over two ground truths -> recall 0.5 0.5 1, precision 1 0.5 2/3
    gt = [box(0, 0, 0, 2, 4, 1), box(20, 0, 0, 2, 4, 1)]
    pred = [box(0, 0, 0, 2, 4, 1, score=0.9, uid=0), box(50, 0, 0, 2, 4, 1, score=0.8, uid=1), box(20, 0, 0, 2, 4, 1, score=0.7, uid=2)]
    recalls, precisions, ap, seen = C.recall_precision(gt, pred, [0.5])
    assert recalls[:, 0].tolist() == [0.5, 0.5, 1.0] and precisions[:, 0].tolist() == pytest.approx([1.0, 0.5, 2 / 3])
    assert ap[0] == pytest.approx(0.5 * 1.0 + 0.5 * (2 / 3), abs=1e-15)           # envelope 1, 2/3, 2/3
    assert [seen[k][2] for k in range(3)] == [0, 0, 1] and [seen[k][3][0] for k in range(3)] == [1.0, 0.0, 1.0]
    # get_ap on its own: recall stays, precision drops -> only the first step counts
    assert C.get_ap(np.array([0.5, 0.5]), np.array([1.0, 0.5])) == pytest.approx(0.5)


def test_a_claimed_ground_truth_makes_the_later_prediction_a_false_positive_per_cutoff():
    # two predictions on one ground truth: IoU 0.6 with the higher score, IoU 1 with the lower one
    gt = [box(0, 0, 0, 2, 4, 1)]
    shifted = box(1.0, 0, 0, 2, 4, 1, score=0.9, uid="far")                     # 3 / 5 = 0.6
    pred = [shifted, box(0, 0, 0, 2, 4, 1, score=0.5, uid="exact")]
    _, _, ap, seen = C.recall_precision(gt, pred, [0.5, 0.7])
    assert seen["far"][1] == pytest.approx(0.6) and seen["far"][3].tolist() == [1.0, 0.0]
    assert seen["exact"][3].tolist() == [0.0, 1.0]                              # claimed at 0.5, free at 0.7
    assert ap[0] == pytest.approx(1.0) and ap[1] == pytest.approx(0.5)


def test_the_class_rules():
    gt = [box(0, 0, 0, 2, 4, 1, name="car"), box(9, 9, 0, 1, 1, 2, name="pedestrian")]
    pred = [box(0, 0, 0, 2, 4, 1, name="car", score=0.9, uid=0), box(5, 5, 0, 2, 6, 2, name="truck", score=0.5, uid=1)]
    avg, per_cut, _ = C.get_average_precisions(gt, pred, ["car", "truck", "pedestrian"], [0.5, 0.7])
    assert avg.tolist() == [1.0, -1.0, 0.0]                                     # predictions without ground truth: -1; no predictions: 0
    assert per_cut[1].tolist() == [-1.0, -1.0]
    text, res = E.format_lyft_results(avg, ["car", "truck", "pedestrian"], [0.5, 0.7], version="one_scene")
    assert res == {"car": 1.0, "truck": -1.0, "pedestrian": 0.0, "mAP": 0.0}   # the -1 enters the mean


def test_the_result_string():
    text, res = E.format_lyft_results(np.array([0.25, -1.0]), ["car", "animal"], [0.5, 0.55])
    assert text == ("----------------Lyft trainval results-----------------\n"
                    "Average precision over IoUs: [0.5, 0.55]\n"
                    "car                 : \t 0.2500\n"
                    "animal              : \t -1.0000\n"
                    "--------------average performance-------------\n"
                    "mAP:\t -0.3750\n")
    assert list(res) == ["car", "animal", "mAP"] and res["mAP"] == -0.375


# ---- the tables ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    built = C.build(C.small_world())
    built["ref"] = C.get_average_precisions(built["gt"], built["pred"], C.CLASSES, C.THRESHOLDS)
    return built


def write_tables(root, tables):
    (root / "data").mkdir(parents=True, exist_ok=True)
    for name, records in tables.items():
        with open(root / "data" / f"{name}.json", "w") as f:
            json.dump(records, f)


def test_the_loader_reads_three_tables_and_names_a_missing_one(tmp_path, world):
    with pytest.raises(FileNotFoundError, match=r"sample_annotation\.json.*eval_metric 'kitti'"):
        E.load_tables(tmp_path)
    write_tables(tmp_path, world["tables"])
    tables = E.load_tables(tmp_path)
    assert sorted(tables) == sorted(E.TABLES) and tables == world["tables"]
    (tmp_path / "data" / "instance.json").unlink()
    with pytest.raises(FileNotFoundError, match=str(tmp_path / "data" / "instance.json")):
        E.load_tables(tmp_path)


def test_ground_truths_group_by_sample_in_table_order(world):
    mixed = C.interleaved_tables(world["tables"], np.random.default_rng(3))
    assert [a["token"] for a in mixed["sample_annotation"]] != [a["token"] for a in world["tables"]["sample_annotation"]]
    straight, shuffled = E.ground_truth_rows(world["tables"]), E.ground_truth_rows(mixed)
    assert sorted(straight) == ["a", "b", "c"]
    for k, tok in enumerate(["a", "b", "c"]):
        rows, names = straight[tok]
        info = world["infos"][k]
        assert names.tolist() == info["gt_names"].tolist() and rows.shape == (len(names), 8)
        assert np.array_equal(shuffled[tok][0], rows) and shuffled[tok][1].tolist() == names.tolist()
        for row, gt in zip(rows, [g for g in world["gt"] if g["sample_token"] == tok]):
            ref = C.Box3D(**gt)
            rot = C.quat_matrix(gt["rotation"])
            assert row[:3].tolist() == gt["translation"] and row[5:].tolist() == gt["size"]
            assert row[3] == pytest.approx(rot[0, 0], abs=1e-15) and row[4] == pytest.approx(rot[1, 0], abs=1e-15)
            assert np.abs(E.corners_host(row[None])[0] - np.array(ref.ground)).max() < 1e-12
    only = E.ground_truth_rows(world["tables"], ["b"])
    assert list(only) == ["b"] and np.array_equal(only["b"][0], straight["b"][0])


def test_an_unnormalised_quaternion_and_a_bad_size(world):
    ann = dict(world["tables"]["sample_annotation"][0])
    scaled = {**world["tables"], "sample_annotation": [{**ann, "rotation": [3 * v for v in ann["rotation"]]}]}
    assert np.allclose(E.ground_truth_rows(scaled)[ann["sample_token"]][0], E.ground_truth_rows({**world["tables"], "sample_annotation": [ann]})[ann["sample_token"]][0],
                       rtol=0, atol=1e-15)
    for size in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0]):
        with pytest.raises(ValueError, match="not positive"):
            E.ground_truth_rows({**world["tables"], "sample_annotation": [{**ann, "size": size}]})


# ---- the global rows of the predictions ---------------------------------------------------------------------------------------
def test_prediction_rows_under_a_tilted_pose_equal_the_quaternion_chain(world):
    info, anno = world["infos"][1], world["det_annos"][1]                         # sample b: 0.3 rad of roll and pitch
    rows = E.prediction_rows(info, anno["boxes_lidar"])
    refs = [p for p in world["pred"] if p["sample_token"] == "b"]
    assert len(rows) == len(refs) > 0
    norms = rows[:, 3] ** 2 + rows[:, 4] ** 2
    assert (norms < 1 - 1e-3).any() and (norms <= 1 + 1e-12).all()                # the footprint shrinks, (c, s) is not normalised
    for row, ref in zip(rows, refs):
        rot = C.quat_matrix(ref["rotation"])
        assert np.abs(row[:3] - ref["translation"]).max() < 1e-10                 # a few hundred metres from the origin
        assert abs(row[3] - rot[0, 0]) < 1e-14 and abs(row[4] - rot[1, 0]) < 1e-14
        assert row[5:].tolist() == ref["size"]
    assert E.prediction_rows(info, np.zeros((0, 7))).shape == (0, 8)


def test_segments_follow_samples_then_classes_and_count_every_ground_truth(world):
    seg = E.segment(world["infos"], world["det_annos"], C.CLASSES, E.ground_truth_rows(world["tables"]))
    uids = C.segment_uids(world["det_annos"], C.CLASSES)
    assert len(seg["pred"]) == len(uids) == seg["pred_off"][-1] and seg["pred_off"].dtype == np.int32 and seg["gt_off"].dtype == np.int32
    scores = {p["uid"]: p["score"] for p in world["pred"]}
    assert seg["pred_score"].tolist() == [scores[u] for u in uids]
    # a: car, truck, pedestrian; b: car, bus, animal; c: pedestrian (bicycle in b has no prediction: no segment, but counted)
    assert np.diff(seg["pred_off"]).tolist() == [14, 2, 5, 7, 3, 2, 9] and np.diff(seg["gt_off"]).tolist() == [6, 0, 3, 4, 2, 0, 5]
    assert seg["n_gt"].tolist() == [10, 0, 2, 0, 0, 0, 2, 8, 0]
    with pytest.raises(ValueError, match="twice"):
        E.segment(world["infos"], world["det_annos"] + world["det_annos"][:1], C.CLASSES, {})
    bad = [dict(world["det_annos"][0])]
    bad[0]["score"] = np.where(np.arange(len(bad[0]["score"])) == 2, np.nan, bad[0]["score"])
    with pytest.raises(ValueError, match="NaN"):
        E.segment(world["infos"], bad, C.CLASSES, {})
    with pytest.raises(KeyError, match="nowhere"):
        E.segment(world["infos"], [{**world["det_annos"][0], "metadata": {"token": "nowhere"}}], C.CLASSES, {})


# ---- the numpy route against the restatement ------------------------------------------------------------------------------------
def test_the_numpy_route_equals_the_restatement(world):
    avg, per_cut, seen = world["ref"]
    assert C.away_from_edges(seen)
    seg = E.segment(world["infos"], world["det_annos"], C.CLASSES, E.ground_truth_rows(world["tables"]))
    tp, best_iou, best_gt = E.flags_host(seg, C.THRESHOLDS)
    for k, uid in enumerate(C.segment_uids(world["det_annos"], C.CLASSES)):
        if uid not in seen:                                                      # a class without any ground truth is never walked
            assert best_gt[k] == -1 and best_iou[k] == -np.inf and not tp[:, k].any()
            continue
        _, best, jmax, flags = seen[uid]
        assert best_gt[k] == jmax and tp[:, k].tolist() == flags.tolist()
        assert (best == -np.inf and best_iou[k] == -np.inf) or abs(best_iou[k] - best) < 1e-12
    aps = E.class_aps(seg, C.THRESHOLDS, len(C.CLASSES), route="host")
    assert np.abs(aps - per_cut).max() < 1e-9 and (aps[[1, 8]] == -1).all() and (aps[6] == 0).all()
    text, res = E.evaluate(world["infos"], world["det_annos"], C.CLASSES, None, C.THRESHOLDS, version="one_scene", route="host", tables=world["tables"])
    assert text == E.format_lyft_results(aps.mean(1), C.CLASSES, C.THRESHOLDS, version="one_scene")[0]
    assert abs(res["mAP"] - avg.mean()) < 1e-9 and res["truck"] == -1.0 and res["car"] > 0.1


def test_bad_cutoffs_and_routes_are_refused(world):
    seg = E.segment(world["infos"], world["det_annos"], C.CLASSES, E.ground_truth_rows(world["tables"]))
    for ths in ([], [0.7, 0.5], [0.5, 0.5], [0.5, 1.5]):
        with pytest.raises(ValueError, match="cut-offs"):
            E.class_aps(seg, ths, len(C.CLASSES), route="host")
    with pytest.raises(ValueError, match="route"):
        E.class_aps(seg, [0.5], len(C.CLASSES), route="shapely")


# ---- the exports without a GPU -----------------------------------------------------------------------------------------------
def test_the_new_exports_validate_before_they_launch():
    lib = L.load()
    assert lib.toda_lyft_eval_flags_chunk() == 256
    assert lib.toda_lyft_eval_workspace_bytes(0) == 0 and lib.toda_lyft_eval_workspace_bytes(-3) == 0
    assert lib.toda_lyft_eval_workspace_bytes(1) == 512 and lib.toda_lyft_eval_workspace_bytes(40000) >= 2 * 40001 * 4
    one = L.host_f64([0.0] * 8)
    p = L.hptr(one)
    big = 1 << 20

    def best(n_pred, n_gt, pred_off, gt_off, n_seg, ws=p, ws_bytes=big, rows=p):
        return lib.toda_lyft_eval_best(rows, n_pred, rows, n_gt, None if pred_off is None else L.hptr(L.host_i32(pred_off)),
                                       None if gt_off is None else L.hptr(L.host_i32(gt_off)), n_seg, rows, rows, ws, ws_bytes, None)

    def err():
        return lib.toda_last_error().decode()

    assert best(-1, 0, [0], [0], 0) == -1 and "negative size" in err()
    assert best(0, 0, None, None, 0) == 0                                          # no segment: nothing to do
    assert best(2, 0, None, None, 0) == -1 and "no segment" in err()
    assert best(2, 2, None, [0, 2], 1) == -1 and "null offsets" in err()
    assert best(2, 2, [0, 1], [0, 2], 1) == -1 and "predictions must run from 0 to 2" in err()
    assert best(2, 2, [0, 2], [1, 2], 1) == -1 and "ground truths must run from 0 to 2" in err()
    assert best(2, 2, [0, 3, 2], [0, 1, 2], 2) == -1 and "descend at segment 1" in err()
    assert best(0, 5, [0, 0], [0, 5], 1, rows=None, ws=None, ws_bytes=0) == 0      # no prediction: nothing to do
    assert best(2, 2, [0, 2], [0, 2], 1, rows=None) == -1 and "null boxes" in err()
    assert best(2, 2, [0, 2], [0, 2], 1, ws_bytes=511) == -1 and "workspace too small" in err()
    assert best(2, 2, [0, 2], [0, 2], 1, ws=None) == -1 and "workspace too small" in err()

    def flags(n_pred, pred_off, n_seg, ths, n_ths=None, ws=p, ws_bytes=big, rows=p):
        return lib.toda_lyft_eval_flags(rows, rows, rows, n_pred, None if pred_off is None else L.hptr(L.host_i32(pred_off)), n_seg,
                                        None if ths is None else L.hptr(L.host_f64(ths)), len(ths) if n_ths is None else n_ths, rows, ws, ws_bytes, None)

    assert flags(-1, [0], 0, [0.5]) == -1 and "negative size" in err()
    assert flags(2, [0, 2], 1, [0.5], n_ths=0) == -1 and "0 cut-offs, supported are 1 to 16" in err()
    assert flags(2, [0, 2], 1, [0.5] * 17) == -1 and "17 cut-offs" in err()
    assert flags(2, [0, 2], 1, None, n_ths=1) == -1 and "null cut-offs" in err()
    assert flags(2, [0, 2], 1, [0.5, 0.5]) == -1 and "ascend (entry 1)" in err()
    assert flags(2, [0, 2], 1, [0.5, float("nan")]) == -1 and "ascend (entry 1)" in err()
    assert flags(0, None, 0, [0.5]) == 0 and flags(0, [0, 0], 1, [0.5], rows=None, ws=None, ws_bytes=0) == 0
    assert flags(2, None, 0, [0.5]) == -1 and "no segment" in err()
    assert flags(2, None, 1, [0.5]) == -1 and "null offsets" in err()
    assert flags(2, [0, 1], 1, [0.5]) == -1 and "must run from 0 to 2" in err()
    assert flags(2, [0, 2], 1, [0.5], rows=None) == -1 and "null scores" in err()
    assert flags(2, [0, 2], 1, [0.5], ws_bytes=100) == -1 and "workspace too small" in err()


def test_sweeps_merge_rect_has_the_argument_rules_of_sweeps_merge():
    lib = L.load()
    bound = lib.toda_sweeps_merge_max_sweeps()
    fake = L.hptr(L.host_f64([0.0] * 16))

    def merge(n, s, p, rx=1.5, ry=1.0):
        return lib.toda_sweeps_merge_rect(p, n, s, p, p, p, p, p, rx, ry, None, p, p, None)

    def err():
        return lib.toda_last_error().decode()

    assert merge(-1, 1, fake) == -1 and err() == "sweeps_merge_rect: need n >= 0"
    for s in (0, bound + 1):
        assert merge(8, s, fake) == -1 and err() == "sweeps_merge_rect: %d sweeps, supported are 1 to %d (key frame included)" % (s, bound)
    for rx, ry in ((-1.0, 1.0), (1.5, -0.5), (float("nan"), 1.0), (1.5, float("nan"))):
        assert merge(8, 1, fake, rx, ry) == -1 and err() == "sweeps_merge_rect: the ego half-sides must be numbers >= 0"
    assert merge(0, 0, None) == -1 and merge(0, 1, None, ry=float("nan")) == -1           # sizes come first
    assert merge(0, 1, None) == 0 and merge(0, bound, None) == 0 and merge(0, 1, None, 0.0, 0.0) == 0
    assert merge(8, 1, None) == -1 and err() == "sweeps_merge_rect: null sweep table"
    header = open(L.os.path.join(L.os.path.dirname(L._HERE), "include", "toda.h")).read()
    assert "int toda_sweeps_merge_rect(const float* rows, int n, int n_sweeps," in header and "float radius_x, float radius_y," in header
    assert lib.toda_abi_version() == 3
