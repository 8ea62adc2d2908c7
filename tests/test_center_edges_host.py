"""The CenterPoint head's edge cases without a GPU: the oracle against the reference's own target assignment
(tests/golden/center_edges.npz), the conditions that make those cases reach the kernel's paths, the float64 clip of
tests/center_edge_cases.py against closed forms, the oracle's measured error against the clip, the NMS constructions, and the
argument checks of the fused loss that return before anything is launched or dereferenced."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import center_edge_cases as E
from toda_amd import lib as L

FAKE = 4096        # a non-null "device pointer" for arguments a refused call must not touch
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "center_edges.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------- target assignment
def test_fixture_holds_arrays_only_and_the_cases_of_the_table(golden):
    assert all(v.dtype.kind in "fi" for v in golden.values())
    assert {k.split(".")[0] for k in golden} == set(E.ASSIGN_CASES)
    for case, c in E.ASSIGN_CASES.items():
        assert golden[f"{case}.settings"].tolist() == [c["h"], c["w"], c["code"], c["max_objs"], c["min_radius"], len(c["heads"])]
        gt = golden[f"{case}.gt"]
        assert gt.dtype == np.float32 and gt.shape == (c["batch"], c["g"], c["code"])
        assert np.array_equal(gt, E.assign_gt(case))                       # the builder regenerates the stored input
        for i, names in enumerate(c["heads"]):
            assert golden[f"{case}.heatmap{i}"].shape == (c["batch"], len(names), c["h"], c["w"])
            assert golden[f"{case}.target_boxes{i}"].shape == (c["batch"], c["max_objs"], c["code"])
            assert golden[f"{case}.inds{i}"].dtype == np.int64 and golden[f"{case}.masks{i}"].dtype == np.int64
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "center_head.npz"))


@pytest.mark.parametrize("case", list(E.ASSIGN_CASES))
def test_center_assign_oracle_matches_reference_at_the_edges(golden, case):
    c = E.ASSIGN_CASES[case]
    pc_range, vs, _ = E.assign_geometry(case)
    for i, names in enumerate(c["heads"]):
        gt = E.head_gt(golden[f"{case}.gt"], case, i)
        hm, rb, inds, mask = O.center_assign(gt, len(names), c["w"], c["h"], pc_range, vs, E.STRIDE, c["max_objs"], E.OVERLAP, c["min_radius"])
        assert np.array_equal(inds, golden[f"{case}.inds{i}"])
        assert np.array_equal(mask, golden[f"{case}.masks{i}"])
        assert np.array_equal(hm, golden[f"{case}.heatmap{i}"])
        np.testing.assert_allclose(rb, golden[f"{case}.target_boxes{i}"], rtol=1e-6, atol=1e-6)


def in_head_counts(golden, case, head):
    return (E.head_gt(golden[f"{case}.gt"], case, head)[..., -1] > 0).sum(1)


def test_assign_cases_reach_the_paths_they_are_meant_for(golden):
    # overflow: more in-head boxes than slots, in every sample of `wide` and in both heads of `two_heads`
    assert (in_head_counts(golden, "wide", 0) > E.ASSIGN_CASES["wide"]["max_objs"]).all()
    assert (golden["wide.masks0"].sum(1) == 150).all()
    for i in range(2):
        assert (in_head_counts(golden, "two_heads", i) > E.ASSIGN_CASES["two_heads"]["max_objs"]).all()
    # ... in `wide` the cap is reached inside the first chunk of 256 rows: the second chunk lies entirely past it
    first = (E.head_gt(golden["wide.gt"], "wide", 0)[:, :256, -1] > 0).sum(1)
    assert (first >= 150).all()
    assert np.abs(golden["wide.target_boxes0"][..., 8:10]).min(-1).max() > 0          # velocity columns carry values
    # `tall`: drawn rows with gt index >= 256, at slots that continue the count of the first chunk
    gt = E.head_gt(golden["tall.gt"], "tall", 0)
    before, total = int((gt[0, :256, -1] > 0).sum()), int((gt[0, :, -1] > 0).sum())
    assert total > before + 10 and total <= 500
    mask = golden["tall.masks0"]
    assert mask[0, before:total].sum() > 10 and mask[0, total:].sum() == 0
    # ... and its planted rows
    assert mask[0, int((gt[0, :E.TALL_DX0, -1] > 0).sum())] == 0                      # dx = 0 keeps its (empty) slot
    slot = lambda r: int((gt[0, :r, -1] > 0).sum())                                   # noqa: E731
    inds = golden["tall.inds0"][0]
    a, b = E.TALL_TWICE
    assert inds[slot(a)] == inds[slot(b)] and mask[0, slot(a)] == mask[0, slot(b)] == 1 and gt[0, a, -1] == gt[0, b, -1]
    a, b = E.TALL_BLEND
    assert inds[slot(a)] == inds[slot(b)] and gt[0, a, -1] == gt[0, b, -1] and gt[0, a, 3] > 3 * gt[0, b, 3]
    a, b = E.TALL_CELL
    assert inds[slot(a)] == inds[slot(b)] and gt[0, a, -1] != gt[0, b, -1]
    assert (gt[E.TALL_CLASS0_SAMPLE, :, -1] == 0).all() and mask[E.TALL_CLASS0_SAMPLE].sum() == 0
    assert not golden["tall.heatmap0"][E.TALL_CLASS0_SAMPLE].any()
    # `tiny`: radius >= MIN_RADIUS = 4, so 2 r + 1 >= 9 exceeds both axes of the 3 x 5 map - every window is clipped on four sides
    c = E.ASSIGN_CASES["tiny"]
    assert max(c["h"], c["w"]) < 2 * c["min_radius"] + 1 and golden["tiny.masks0"].sum() > 40
    # borders: centres clamp at each of the four borders of the non-square maps
    for case in ("wide", "tall"):
        c, g0 = E.ASSIGN_CASES[case], golden[f"{case}.gt"]
        live = g0[..., -1] > 0
        assert (g0[live][:, 0] < 0).any() and (g0[live][:, 0] > c["w"]).any() and (g0[live][:, 1] < 0).any() and (g0[live][:, 1] > c["h"]).any()
        assert c["h"] != c["w"] and golden[f"{case}.inds0"].max() >= c["w"] * (c["h"] - 1)
    assert golden["cell.masks0"].sum(1).tolist() == [3, 2] and golden["empty.gt"].shape[1] == 0
    assert not golden["empty.heatmap0"].any() and not golden["empty.masks0"].any()


# ------------------------------------------------------------------------------- fused loss: case table and refusals
def test_loss_cases_have_the_properties_they_are_named_for():
    for name, (b, c, h, w, k, chans) in E.LOSS_CASES.items():
        hm, heatmap, inds, mask, target, regs = E.loss_case(name)
        assert hm.shape == heatmap.shape == (b, c, h, w) and inds.shape == mask.shape == (b, k)
        assert target.shape == (b, k, sum(chans)) and [r.shape[1] for r in regs] == list(chans)
        assert w <= 20 and int(inds.min()) >= 0 and int(inds.max()) < h * w
        assert (inds[mask == 0] == 0).all()
        if name not in ("no_positive", "all_masked"):
            for bi in range(b):      # every live slot sits under a positive, as the assigner leaves it
                assert all(bool((heatmap[bi, :, cell // w, cell % w] == 1).any()) for cell in inds[bi][mask[bi] == 1].tolist())
    assert not (E.loss_case("no_positive")[1] == 1).any() and E.loss_case("no_positive")[3].sum() > 0
    assert E.loss_case("all_masked")[3].sum() == 0 and (E.loss_case("all_masked")[1] == 1).any()
    assert E.LOSS_CASES["k1"][4] == 1
    _, _, inds, mask, _, _ = E.loss_case("one_cell_300")
    assert inds.shape[1] == 300 > 256 and all(len(set(r.tolist())) == 1 for r in inds) and bool(mask.all())
    assert sum(E.LOSS_CASES["d16"][5]) == 16 and len(E.LOSS_CASES["d16"][5]) == 8
    for name, blocks in (("n1024", 1), ("n2048", 2)):
        b, c, h, w = E.LOSS_CASES[name][:4]
        assert b * c * h * w == blocks * E.LOSS_BLOCK_ELEMS
    b, c, h, w = E.LOSS_CASES["last_cell"][:4]
    _, _, inds, mask, _, _ = E.loss_case("last_cell")
    assert (h, w) == (12, 20) and (inds[:, 0] == h * w - 1).all() and bool(mask[:, 0].all())
    assert E.LOSS_CASES["k8192"][4] == E.LOSS_K_MAX and E.LOSS_CASES["k8192"][2:4] == (4, 4)


def loss_fwd_rc(chans, k, d):
    lib = L.load()
    maps = L.host_addrs([FAKE] * len(chans))
    return lib.toda_center_loss_fwd(FAKE, FAKE, 1, 1, 4, 4, len(chans), maps, L.hptr(L.host_i32(chans)), FAKE, FAKE, FAKE, k, d,
                                    L.hptr(L.host_f32([1.0] * 16)), 1.0, 1.0, FAKE, FAKE, FAKE, 1 << 30, None)


def loss_bwd_rc(chans, k, d):
    lib = L.load()
    maps = L.host_addrs([FAKE] * len(chans))
    return lib.toda_center_loss_bwd(FAKE, FAKE, FAKE, 1, 1, 4, 4, len(chans), maps, L.hptr(L.host_i32(chans)), FAKE, FAKE, k, d,
                                    L.hptr(L.host_f32([1.0] * 16)), 1.0, 1.0, FAKE, FAKE, 1 << 30, None)


def test_center_loss_refuses_17_code_dimensions_and_8193_slots_before_it_launches():
    for fn, who in ((loss_fwd_rc, "center_loss_fwd"), (loss_bwd_rc, "center_loss_bwd")):
        assert fn((2, 2, 2, 2, 2, 2, 2, 3), 7, 17) == -1                    # 17 code dimensions over 8 branches
        assert who in L.last_error() and "17" in L.last_error()
        assert fn((2, 1, 3, 2), E.LOSS_K_MAX + 1, 8) == -1                  # 8193 object slots
        assert who in L.last_error() and "8192" in L.last_error()
        assert fn((1,) * 9, 7, 9) == -1 and "branches" in L.last_error()   # nine branches
        assert fn((2, 1, 3, 2), 7, 9) == -1 and who in L.last_error()       # channels that do not sum to the code size


def test_center_loss_supported_is_false_past_16_code_dimensions():
    from toda_amd import ops

    class OnGpu(torch.Tensor):
        is_cuda = True

    def meta(*shape):
        return torch.empty(shape, dtype=torch.float32, device="meta").as_subclass(OnGpu)

    hm = meta(2, 3, 4, 4)
    ok = [meta(2, 2, 4, 4) for _ in range(8)]
    assert ops.center_loss_supported(hm, ok, meta(2, 7, 16))
    assert not ops.center_loss_supported(hm, ok[:7] + [meta(2, 3, 4, 4)], meta(2, 7, 17))
    assert not ops.center_loss_supported(hm, ok + [meta(2, 1, 4, 4)], meta(2, 7, 17))


# ------------------------------------------------------------------------------- exact overlap
def test_clip_matches_the_closed_forms():
    """The clip of the float32 boxes against the closed forms: 1e-6, which covers the float32 rounding of the inputs (a heading of
    0.5 + pi is off by up to 1.2e-7 rad, a centre near 70 m by up to 3.8e-6 m, for boxes of a few metres)."""
    for shift in E.SHIFTS:
        a, b, area, iou = E.closed_form_batch(shift)
        for i, c in enumerate(E.CLOSED_FORMS):
            assert abs(E.clip_area(a[i], b[i]) - area[i]) <= 1e-6 * max(1.0, area[i]), (c[0], shift)
            assert abs(E.clip_area(b[i], a[i]) - area[i]) <= 1e-6 * max(1.0, area[i]), (c[0], shift)
            assert abs(E.clip_iou(a[i], b[i]) - iou[i]) <= 1e-6, (c[0], shift)
        for p, q, q_reduced in E.WRAPPED:
            p, q, q_reduced = E.shifted(p, shift)[0], E.shifted(q, shift)[0], E.shifted(q_reduced, shift)[0]
            assert abs(E.clip_area(p, q) - E.clip_area(p, q_reduced)) <= 1e-6 and E.clip_area(p, q) > 1.0
            assert abs(float(q[6])) > math.pi > abs(float(q_reduced[6]))
    assert E.CLOSED_FORMS[2][3] == pytest.approx(3.3137085, abs=1e-7)


def test_clip_against_a_polygon_area_it_does_not_compute_itself():
    """The clip on generic pairs against a count of the cells of a fine grid whose centres lie in both rectangles: no polygon, no
    clipping, only the definition of `inside`."""
    rng = np.random.default_rng(5)
    n = 400
    xs = (np.arange(n) + 0.5) / n * 8 - 4
    gx, gy = np.meshgrid(xs, xs)

    def inside(b):
        c, s = math.cos(b[6]), math.sin(b[6])
        rx, ry = (gx - b[0]) * c + (gy - b[1]) * s, -(gx - b[0]) * s + (gy - b[1]) * c
        return (np.abs(rx) <= b[3] / 2) & (np.abs(ry) <= b[4] / 2)

    for _ in range(6):
        a = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 0, rng.uniform(1, 3), rng.uniform(1, 3), 1, rng.uniform(-7, 7)])
        b = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 0, rng.uniform(1, 3), rng.uniform(1, 3), 1, rng.uniform(-7, 7)])
        count = float((inside(a) & inside(b)).sum()) * (8.0 / n) ** 2
        # a cell of 0.02 m is miscounted only along the outline (< 12 m): a few hundredths of a square metre at the very most
        assert abs(E.clip_area(a, b) - count) < 0.03, (a, b)


@pytest.mark.parametrize("offset", E.PAIR_OFFSETS)
def test_random_pairs_are_separated_overlap_and_bound_the_oracle(offset):
    a, b = E.random_pairs(offset)
    assert a.shape == b.shape == (E.PAIRS, 7) and a.dtype == np.float32
    assert min(E.separation(p, q) for p, q in zip(a, b)) >= E.SEPARATION
    assert 0.5 <= a[:, 3:5].min() and a[:, 3:5].max() <= 5.0 and np.abs(a[:, 6]).max() <= 7.0 and np.abs(a[:, 6]).max() > math.pi
    assert abs(float(a[:, 0].mean()) - offset) < 1.0 and abs(float(a[:, 1].mean()) + 3.0 / 7.0 * offset) < 1.0
    area = np.array([E.clip_area(p, q) for p, q in zip(a, b)])
    iou = np.array([E.clip_iou(p, q) for p, q in zip(a, b)])
    assert (area > 0.5).mean() >= 0.5
    # the oracle (the reference's algorithm in fp32) pair by pair, in both argument orders
    err_area = max(float(np.abs(oracle_pairs(O.boxes_overlap_bev, x, y) - area).max()) for x, y in ((a, b), (b, a)))
    err_iou = max(float(np.abs(oracle_pairs(O.boxes_iou_bev, x, y) - iou).max()) for x, y in ((a, b), (b, a)))
    print(f"offset {offset}: oracle area error {err_area:.3e}, IoU error {err_iou:.3e}")
    assert err_area <= E.ORACLE_ERR[offset][0] and err_iou <= E.ORACLE_ERR[offset][1]
    # ... and the recorded bound is a measurement, not head-room
    assert err_area >= 0.5 * E.ORACLE_ERR[offset][0] and err_iou >= 0.5 * E.ORACLE_ERR[offset][1]


def oracle_pairs(fn, a, b):
    return np.array([fn(a[i:i + 1], b[i:i + 1])[0, 0] for i in range(len(a))], np.float64)


def test_oracle_on_the_closed_forms_stays_within_its_error_at_that_offset():
    for shift, offset in zip(E.SHIFTS, E.PAIR_OFFSETS):
        assert shift == (offset, -3.0 / 7.0 * offset)                      # the closed forms sit on the pairs' centre
        a, b, area, iou = E.closed_form_batch(shift)
        for x, y in ((a, b), (b, a)):
            err_area = np.abs(oracle_pairs(O.boxes_overlap_bev, x, y) - area).max()
            err_iou = np.abs(oracle_pairs(O.boxes_iou_bev, x, y) - iou).max()
            print(f"shift {shift}: oracle area error {err_area:.3e}, IoU error {err_iou:.3e}")
            assert err_area <= E.ORACLE_ERR[offset][0] and err_iou <= E.ORACLE_ERR[offset][1]
        for p, q, q_reduced in E.WRAPPED:
            p, q, q_reduced = E.shifted(p, shift), E.shifted(q, shift), E.shifted(q_reduced, shift)
            for r in (q, q_reduced):
                assert abs(float(O.boxes_overlap_bev(p, r)[0, 0]) - E.clip_area(p[0], r[0])) <= E.ORACLE_ERR[offset][0]


# ------------------------------------------------------------------------------- NMS constructions
def test_lattice_boxes_are_disjoint_and_the_constructed_keep_lists_are_the_greedy_ones():
    for n in (65, 129):
        iou = E.aabb_iou(E.lattice(n))
        assert np.array_equal(iou > 0, np.eye(n, dtype=bool))
        assert np.array_equal(E.greedy_keep(iou, 0.5), np.arange(n))
        assert E.greedy_keep(iou, -1.0).tolist() == [0]                    # every IoU, 0 included, exceeds a negative threshold
        assert np.array_equal(E.greedy_keep(iou, 1.5), np.arange(n))
    assert (4160 + 63) // 64 == 65                                          # 65 suppression words: a second trip of `w += 64`
    boxes, keep = E.late_duplicates()
    iou = E.aabb_iou(boxes)
    assert np.array_equal(E.greedy_keep(iou, 0.5), keep) and len(keep) == 4160 - 62
    assert all(4100 // 64 == 64 and i // 64 == 0 for i in range(60))        # word 64, removed by rows of word 0
    iou = E.aabb_iou(np.repeat(E.lattice(1), 200, 0))
    assert E.greedy_keep(iou, 0.5).tolist() == [0]


@pytest.mark.parametrize("triple", E.CHAIN_TRIPLES)
def test_chains_keep_a_and_c_with_every_iou_clear_of_the_threshold(triple):
    boxes, keep = E.chain(triple)
    a, b, c = (boxes[i] for i in triple)
    ious = E.clip_iou(a, b), E.clip_iou(b, c), E.clip_iou(a, c)
    assert ious[0] > E.CHAIN_THRESH + 0.02 and ious[1] > E.CHAIN_THRESH + 0.02 and ious[2] < E.CHAIN_THRESH - 0.02
    assert ious[0] == pytest.approx(2.8 / 5.2, abs=1e-6) and ious[2] == pytest.approx(0.25, abs=1e-6)
    iou = E.aabb_iou(boxes)
    assert abs(iou[triple[0], triple[1]] - ious[0]) < 1e-12
    others = np.ones(len(boxes), bool)
    others[list(triple)] = False
    assert not (iou[others][:, ~others] > 0).any()                         # the chain touches nothing else
    assert np.array_equal(E.greedy_keep(iou, E.CHAIN_THRESH), keep)
    assert triple[0] in keep and triple[2] in keep and triple[1] not in keep
    assert np.array_equal(O.nms_rotated(boxes, E.CHAIN_THRESH), keep)      # the oracle, as a cross-check


def test_mask_words_reference_is_the_strict_upper_triangle():
    boxes, _ = E.chain((62, 63, 64), n=129)
    boxes[128] = boxes[0]
    words = E.mask_words(E.aabb_iou(boxes), 0.5)
    assert words.shape == (129, 3) and words.dtype == np.uint64
    assert int(words[62, 0]) == 1 << 63 and int(words[62, 1]) == 0          # A removes B (63), not C (64)
    assert int(words[63, 0]) == 0 and int(words[63, 1]) == 1               # B removes C: bit 0 of word 1
    assert int(words[0, 2]) == 1 and int(words[128].sum()) == 0 and int(words[64].sum()) == 0
    assert sum(bin(int(w)).count("1") for w in words.ravel()) == 3
