"""The adversarial point-edit kernels (csrc/adv_frame.hip, ops.adv_edit) against the literal restatement of the reference loop
(tests/adv_frame_cases.py), bit for bit: the rows, their order, the per-box counts and the row count."""
import numpy as np
import pytest
import torch

from tests import adv_frame_cases as A
from toda_amd import lib as L
from toda_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25
CFG = {"point_cloud_range": list(A.LO) + list(A.LO + A.VOXEL * np.asarray(A.GRID, np.float32)), "voxel_size": list(A.VOXEL), "grid_size": list(A.GRID)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(case, cap):
    """ops.adv_edit into a sentinel-filled buffer of `cap` rows: (the whole buffer, the device's row count, counts)."""
    buf = ops.RowBuffer(cap, case["points"].shape[1], "cuda")
    buf.data.fill_(SENTINEL)
    _, counts = ops.adv_edit(_dev(case["points"]), case["boxes"], case["op"], case["frac"], case["seed"], _dev(case["keys"]), _dev(case["grads"]),
                             CFG, A.EPS, out=buf)
    return buf.data.cpu().numpy(), int(buf.cursor.item()), counts.cpu().numpy()


def _check(case):
    want, counts, n_kept = A.expected(case)
    got, total, got_counts = _run(case, len(want) + 3)
    assert total == len(want)
    assert (got_counts == counts).all()
    assert got[:total].tobytes() == want.tobytes()
    assert (got[total:] == np.float32(SENTINEL)).all()                 # nothing written beyond the output rows
    return want, counts, n_kept


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_edge_sizes_of_the_row_map(n, k):
    _, counts, _ = _check(A.general(n, k, seed=100 * k + n))
    if n >= 63:
        assert counts.max() > 5


def test_the_largest_table_and_one_more_box_than_a_staging_chunk():
    lib = L.load()
    assert lib.toda_adv_edit_max_boxes() >= 512
    for k in (lib.toda_adv_edit_chunk() + 1, lib.toda_adv_edit_max_boxes()):
        _, counts, _ = _check(A.many_boxes(k, seed=k))
        assert (counts > 5).sum() > k // 2
    with pytest.raises(RuntimeError, match="boxes"):
        _check(A.many_boxes(lib.toda_adv_edit_max_boxes() + 1, seed=1, n=10))


@pytest.mark.parametrize("name", list(A.OBJECT_CASES))
def test_object_cases(name):
    case = A.objects(A.OBJECT_CASES[name], seed=50 + len(name))
    want, counts, n_kept = _check(case)
    assert list(counts) == [c for c, edits in A.OBJECT_CASES[name] for _ in edits]
    n = len(case["points"])
    if name == "single_row":                       # c = 1: k = 0 and the row is selected - moved, copied, and (c <= 5) not removed
        assert n_kept == n and len(want) == n + 1
    if name == "remove_thresholds":                # c = 5 does nothing; c = 6 acts: all six rows, then exactly one
        assert n_kept == n - 6 - 1
    if name == "frac_zero":
        assert n_kept == n - 40 and len(want) == n_kept + 40
    if name == "frac_almost_one":
        assert n_kept == n - 1 and len(want) == n_kept + 1


def _displacement(case):
    return np.float32(A.EPS) * A.point_gradients(case["points"][:, :3], case["keys"], case["grads"], A.LO, A.VOXEL, A.GRID)


def test_overlapping_boxes_walk_in_table_order():
    """The first cluster of each overlap case sits in two boxes with frac 0 (every row selected), rows 200 .. 224."""
    rows = slice(200, 225)
    for name in ("modify_modify", "modify_add", "remove_add", "add_remove"):
        case = A.objects(A.OBJECT_CASES[name], seed=77)
        got, total, _ = _run(case, 400)
        d, xyz = _displacement(case)[rows], case["points"][rows, :3]
        assert (np.abs(d).max(1) > 0).sum() > 10
        once, twice = xyz - d, (xyz - d) - d
        want_all, _, n_kept = A.expected(case)
        assert got[:total].tobytes() == want_all.tobytes()
        added = got[n_kept:total]
        first = added[np.isin(added[:, 3], case["points"][rows, 3])]               # the copies of the first cluster, in row order
        if name == "modify_modify":                 # moved twice
            assert got[rows, :3].tobytes() == twice.astype(np.float32).tobytes()
        if name == "modify_add":                    # the original once displaced, the copy at the doubly displaced position
            assert got[rows, :3].tobytes() == once.tobytes() and first[:, :3].tobytes() == twice.tobytes()
            assert first[:, 3:].tobytes() == case["points"][rows, 3:].tobytes()
        if name in ("remove_add", "add_remove"):    # the copy exists, the original does not
            assert first[:, :3].tobytes() == once.tobytes() and len(first) == 25
            assert not np.isin(got[:n_kept, 3], case["points"][rows, 3]).any()


@pytest.mark.parametrize("kind", ["present", "absent", "no_keys"])
def test_voxel_lookup(kind):
    case = A.lookup_case(absent=kind == "absent", with_keys=kind != "no_keys")
    want, counts, n_kept = _check(case)
    pts = case["points"]
    moved = (want[:, :3] != pts[:, :3]) & ~np.isnan(pts[:, :3])
    assert n_kept == len(pts) == len(want)
    if kind != "present":
        assert not moved.any()                      # an absent key, m = 0: nothing moves, -0.0 and NaN rows included (bytes above)
        return
    assert not moved[:6].any()                      # outside the grid on each of the six sides
    assert moved[6].any() and moved[7].any()        # the first and the last key
    assert moved[8].any() and moved[11].any()       # (x - lo) / voxel an integer
    d = _displacement(case)
    assert (want[8, :3] == pts[8, :3] - d[8]).all()
    assert np.isnan(want[9, 0]) and np.isnan(want[10, 1]) and want[9:11].tobytes() == pts[9:11].tobytes()      # NaN rows pass through
    assert counts[0] == len(pts) - 2


def test_a_box_with_more_rows_than_lds_holds():
    case = A.big_box()
    want, counts, n_kept = _check(case)
    assert counts[0] == counts[1] >= 70000
    c = int(counts[0])
    assert len(want) - n_kept == c - c // 2 and len(case["points"]) - n_kept == c - c // 4


def test_overflow_is_reported_when_the_capacity_is_one_row_short():
    case = A.objects(A.OBJECT_CASES["add_modify_add_remove_modify"], seed=5)
    want, _, _ = A.expected(case)
    got, total, _ = _run(case, len(want) - 1)
    assert total == len(want)                                                        # the cursor counts every row
    assert got.tobytes() == want[:-1].tobytes()                                      # the rows that fit are right, nothing beyond is touched
    pts, keys, grads = _dev(case["points"]), _dev(case["keys"]), _dev(case["grads"])
    with pytest.raises(RuntimeError, match="overflow"):
        ops.adv_edit(pts, case["boxes"], case["op"], case["frac"], case["seed"], keys, grads, CFG, A.EPS, cap_rows=len(want) - 1)
    out, _ = ops.adv_edit(pts, case["boxes"], case["op"], case["frac"], case["seed"], keys, grads, CFG, A.EPS, cap_rows=len(want))
    assert out.cpu().numpy().tobytes() == want.tobytes()


def test_the_default_capacity_grows_when_a_frame_adds_more_rows_than_it_has():
    case = A.objects([(50, [(A.ADD, 0.0)] * 5)], seed=6, n_bg=10)
    want, _, _ = A.expected(case)
    assert len(want) == 60 + 250
    out, counts = ops.adv_edit(_dev(case["points"]), case["boxes"], case["op"], case["frac"], case["seed"], _dev(case["keys"]), _dev(case["grads"]), CFG, A.EPS)
    assert out.is_cuda and out.cpu().numpy().tobytes() == want.tobytes() and counts.tolist() == [50] * 5


def test_two_identical_calls_give_identical_bytes():
    case = A.general(4099, 2, seed=9)
    a, b = _run(case, 9000), _run(case, 9000)
    assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes() and (a[2] == b[2]).all()


def test_no_boxes_and_no_rows():
    case = A.general(65, 2, seed=3)
    pts = _dev(case["points"])
    out, counts = ops.adv_edit(pts, np.zeros((0, 7), np.float32), [], [], [], _dev(case["keys"]), _dev(case["grads"]), CFG, A.EPS)
    assert out.cpu().numpy().tobytes() == case["points"].tobytes() and counts.numel() == 0
    out, counts = ops.adv_edit(pts[:0], case["boxes"], case["op"], case["frac"], case["seed"], None, None, CFG, A.EPS)
    assert out.shape == (0, 5) and counts.tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="frac"):
        ops.adv_edit(pts, case["boxes"], case["op"], [0.5, 1.0], case["seed"], None, None, CFG, A.EPS)
    with pytest.raises(RuntimeError, match="op"):
        ops.adv_edit(pts, case["boxes"], [0, 4], case["frac"], case["seed"], None, None, CFG, A.EPS)
