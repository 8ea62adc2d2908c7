"""The CenterPoint head's kernels at their edges (cases and references: tests/center_edge_cases.py): target assignment
against the reference's own Python (tests/golden/center_edges.npz), the fused centre loss against the torch operators in
float64, rotated overlap and IoU against exact geometry, and NMS against keep lists known from the construction."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import center_edge_cases as E
from tests.test_gpu_center_loss import torch_losses

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "center_edges.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------- target assignment
def check_targets(got, golden, case, head):
    hm, rb, inds, mask = (t.cpu().numpy() for t in got)
    ref = golden[f"{case}.heatmap{head}"]
    assert np.array_equal(inds, golden[f"{case}.inds{head}"])
    assert np.array_equal(mask, golden[f"{case}.masks{head}"])
    np.testing.assert_allclose(hm, ref, rtol=0, atol=1e-6)
    assert np.array_equal(hm == 1, ref == 1)                   # the focal loss picks its positives by `t == 1.0f`
    np.testing.assert_allclose(rb, golden[f"{case}.target_boxes{head}"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("case", list(E.ASSIGN_CASES))
def test_center_assign_at_its_edges_matches_reference(golden, case):
    from toda_amd import ops

    c = E.ASSIGN_CASES[case]
    pc_range, vs, _ = E.assign_geometry(case)
    for i, names in enumerate(c["heads"]):
        gt = dev(E.head_gt(golden[f"{case}.gt"], case, i))
        args = (gt, len(names), c["w"], c["h"], pc_range, vs, E.STRIDE, c["max_objs"], E.OVERLAP, c["min_radius"])
        got = ops.center_assign(*args)
        check_targets(got, golden, case, i)
        again = ops.center_assign(*args)                       # max-blend by integer atomics: order independent
        assert all(torch.equal(x, y) for x, y in zip(got, again))


@pytest.mark.parametrize("case", [k for k, c in E.ASSIGN_CASES.items() if c["h"] != c["w"]])
def test_center_head_assign_targets_takes_height_then_width(golden, case):
    from tests.test_golden_reference import HEAD_CFG
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.dense_heads import CenterHead

    c = E.ASSIGN_CASES[case]
    cfg = copy.deepcopy(HEAD_CFG)
    cfg.update(E.head_cfg(case))
    if c["code"] > 8:
        cfg["SEPARATE_HEAD_CFG"]["HEAD_ORDER"] = ["center", "center_z", "dim", "rot", "vel"]
        cfg["SEPARATE_HEAD_CFG"]["HEAD_DICT"]["vel"] = dict(out_channels=c["code"] - 8, num_conv=2)
        cfg["LOSS_CONFIG"]["LOSS_WEIGHTS"]["code_weights"] = [1.0] * c["code"]
    pc_range, vs, grid = E.assign_geometry(case)
    head = CenterHead(AttrDict(cfg), 24, 3, E.CLASSES, grid, pc_range, vs, predict_boxes_when_training=False).cuda()
    td = head.assign_targets(dev(golden[f"{case}.gt"].copy()), feature_map_size=(c["h"], c["w"]))
    for i in range(len(c["heads"])):
        check_targets((td["heatmaps"][i], td["target_boxes"][i], td["inds"][i], td["masks"][i]), golden, case, i)


# ------------------------------------------------------------------------------- fused centre loss
CODE_W = [1.0 + 0.1 * i for i in range(16)]
CLS_W, LOC_W = 1.0, 0.25


def run_loss(name, w_hm=1.7, w_loc=0.6, sliced=False):
    """One LOSS_CASES entry through ops.center_loss and through torch_losses in float64, forward and backward of
    w_hm * hm_loss + w_loc * loc_loss, with the bounds of test_fused_center_loss_matches_torch_fp64.  sliced: the regression maps
    are channel slices of one larger tensor (non-contiguous), and the gradient is read from that tensor."""
    from toda_amd import ops

    hm, heatmap, inds, mask, target, regs = E.loss_case(name)
    d = target.shape[2]
    code_w = CODE_W[:d]
    heatmap, inds, mask, target = heatmap.cuda(), inds.cuda(), mask.cuda(), target.cuda()

    def leaves(dtype):
        z = hm.to(dtype).cuda().requires_grad_(True)
        if not sliced:
            rs = [r.to(dtype).cuda().requires_grad_(True) for r in regs]
            return z, rs, rs
        big = torch.cat([torch.full_like(regs[0][:, :1], 7.0)] + [x for r in regs for x in (r, torch.full_like(r[:, :1], -7.0))], dim=1)
        big = big.to(dtype).cuda().requires_grad_(True)
        views, at = [], 1
        for r in regs:
            views.append(big[:, at:at + r.shape[1]])
            at += r.shape[1] + 1
        assert not any(v.is_contiguous() for v in views)
        return z, views, [big]

    def grads_of(roots):
        return [torch.zeros_like(r) if r.grad is None else r.grad for r in roots]

    def once():
        z, rs, roots = leaves(torch.float32)
        assert ops.center_loss_supported(z, rs, target)
        la, lb, prob = ops.center_loss(z, rs, heatmap, inds, mask, target, code_w, CLS_W, LOC_W)
        (w_hm * la + w_loc * lb).backward()
        return la.detach(), lb.detach(), prob, z.grad, grads_of(roots)

    la, lb, prob, gz, gr = once()
    z64, rs64, roots64 = leaves(torch.float64)
    ra, rb, p_ref = torch_losses(z64, rs64, heatmap.double(), inds, mask, target.double(), code_w, CLS_W, LOC_W)
    (w_hm * ra + w_loc * rb).backward()
    ra, rb = float(ra.detach()), float(rb.detach())
    gz_ref = z64.grad if z64.grad is not None else torch.zeros_like(z64)
    gr_ref = grads_of(roots64)
    print(f"{name}: hm {float(la):.7g} vs {ra:.7g}, loc {float(lb):.7g} vs {rb:.7g}, prob {float((prob.double() - p_ref.detach()).abs().max()):.2e}, "
          f"dz {float((gz.double() - gz_ref).abs().max()):.2e} of {float(gz_ref.abs().max()):.2e}, "
          f"dreg {max(float((a.double() - b).abs().max()) for a, b in zip(gr, gr_ref)):.2e} of {max(float(b.abs().max()) for b in gr_ref):.2e}")
    assert abs(float(la) - ra) <= 2e-5 * max(1.0, abs(ra))
    assert abs(float(lb) - rb) <= 2e-5 * max(1.0, abs(rb))
    assert float((prob.double() - p_ref.detach()).abs().max()) < 1e-6
    assert float((gz.double() - gz_ref).abs().max()) <= 5e-5 * float(gz_ref.abs().max())
    for a, b in zip(gr, gr_ref):
        assert float((a.double() - b).abs().max()) <= 1e-5 * max(1e-6, float(b.abs().max()))
    la2, lb2, prob2, gz2, gr2 = once()                          # run-to-run identical (no float atomics)
    assert torch.equal(la, la2) and torch.equal(lb, lb2) and torch.equal(prob, prob2) and torch.equal(gz, gz2)
    assert all(torch.equal(x, y) for x, y in zip(gr, gr2))
    return la, lb, gz, gr, gz_ref, gr_ref


@pytest.mark.parametrize("name", list(E.LOSS_CASES))
def test_fused_center_loss_at_its_edges_matches_torch_fp64(name):
    la, lb, gz, gr, gz_ref, gr_ref = run_loss(name)
    if name == "all_masked":
        assert float(lb) == 0.0 and all(not bool(g.any()) for g in gr)      # exactly zero, not merely small
        assert float(gz_ref.abs().max()) > 0
    if name == "no_positive":
        assert float(la) > 0 and float(lb) > 0
    if name in ("one_cell_300", "k8192"):
        assert max(float(g.abs().max()) for g in gr_ref) > 0


def test_fused_center_loss_backward_of_one_loss_alone():
    _, _, gz, gr, _, _ = run_loss("last_cell", w_hm=1.7, w_loc=0.0)
    assert bool(gz.any()) and all(not bool(g.any()) for g in gr)            # the unused branch: exactly zero
    _, _, gz, gr, _, _ = run_loss("last_cell", w_hm=0.0, w_loc=0.6)
    assert not bool(gz.any()) and all(bool(g.any()) for g in gr)


def test_fused_center_loss_backward_when_one_loss_is_left_out_of_the_graph():
    """hm_loss.backward() alone and loc_loss.backward() alone: autograd hands the other upstream gradient over as None."""
    from toda_amd import ops

    hm, heatmap, inds, mask, target, regs = E.loss_case("last_cell")
    heatmap, inds, mask, target = heatmap.cuda(), inds.cuda(), mask.cuda(), target.cuda()
    code_w = CODE_W[:target.shape[2]]
    z64 = hm.double().cuda().requires_grad_(True)
    rs64 = [r.double().cuda().requires_grad_(True) for r in regs]
    ra, rb, _ = torch_losses(z64, rs64, heatmap.double(), inds, mask, target.double(), code_w, CLS_W, LOC_W)
    ra.backward(retain_graph=True)
    gz_ref = z64.grad.clone()
    rb.backward()
    for which in (0, 1):
        z = hm.cuda().requires_grad_(True)
        rs = [r.cuda().requires_grad_(True) for r in regs]
        out = ops.center_loss(z, rs, heatmap, inds, mask, target, code_w, CLS_W, LOC_W)
        out[which].backward()
        if which == 0:
            assert float((z.grad.double() - gz_ref).abs().max()) <= 5e-5 * float(gz_ref.abs().max())
            assert all(r.grad is None or not bool(r.grad.any()) for r in rs)
        else:
            assert z.grad is None or not bool(z.grad.any())
            for a, b in zip(rs, rs64):
                assert float((a.grad.double() - b.grad).abs().max()) <= 1e-5 * max(1e-6, float(b.grad.abs().max()))


def test_fused_center_loss_takes_non_contiguous_channel_slices():
    run_loss("d16", sliced=True)
    run_loss("last_cell", sliced=True)


# ------------------------------------------------------------------------------- rotated overlap and IoU
def pairwise(fn, a, b):
    """fn on the matrix entry point, read on the diagonal: pair i is (a[i], b[i])."""
    return fn(dev(a), dev(b)).cpu().numpy().astype(np.float64).diagonal()


@pytest.mark.parametrize("which", [0, 1])
def test_overlap_and_iou_closed_forms(which):
    from toda_amd import ops

    shift = E.SHIFTS[which]                                     # the centre of the random pairs of PAIR_OFFSETS[which]
    tol_area, tol_iou = (E.KERNEL_FACTOR * t for t in E.ORACLE_ERR[E.PAIR_OFFSETS[which]])
    a, b, area, iou = E.closed_form_batch(shift)
    for x, y in ((a, b), (b, a)):
        got_area, got_iou = pairwise(ops.boxes_overlap_bev, x, y), pairwise(ops.boxes_iou_bev, x, y)
        for i, c in enumerate(E.CLOSED_FORMS):
            print(f"{c[0]} at {shift}: area {got_area[i]:.8g} ({area[i]:.8g}), IoU {got_iou[i]:.8g} ({iou[i]:.8g})")
        assert np.abs(got_area - area).max() <= tol_area, np.abs(got_area - area)
        assert np.abs(got_iou - iou).max() <= tol_iou, np.abs(got_iou - iou)
    for p, q, q_reduced in E.WRAPPED:         # a heading outside [-pi, pi] and its reduced angle: equal areas
        p, q, q_reduced = E.shifted(p, shift), E.shifted(q, shift), E.shifted(q_reduced, shift)
        got = pairwise(ops.boxes_overlap_bev, np.concatenate([p, p]), np.concatenate([q, q_reduced]))
        want = np.array([E.clip_area(p[0], q[0]), E.clip_area(p[0], q_reduced[0])])
        tol = tol_area
        print(f"wrapped heading {q[0, 6]:.3f} at {shift}: {got[0]:.8g} and {got[1]:.8g} ({want[0]:.8g}, {want[1]:.8g})")
        assert np.abs(got - want).max() <= tol and abs(got[0] - got[1]) <= 2 * tol + abs(want[0] - want[1])


@pytest.mark.parametrize("offset", E.PAIR_OFFSETS)
def test_overlap_and_iou_random_pairs_against_the_exact_clip(offset):
    from toda_amd import ops

    a, b = E.random_pairs(offset)
    area = np.array([E.clip_area(p, q) for p, q in zip(a, b)])
    iou = np.array([E.clip_iou(p, q) for p, q in zip(a, b)])
    for x, y in ((a, b), (b, a)):
        got_area, got_iou = pairwise(ops.boxes_overlap_bev, x, y), pairwise(ops.boxes_iou_bev, x, y)
        err_area, err_iou = float(np.abs(got_area - area).max()), float(np.abs(got_iou - iou).max())
        print(f"offset {offset}: kernel area error {err_area:.3e}, IoU error {err_iou:.3e}; the oracle's: {E.ORACLE_ERR[offset]}")
        assert err_area <= E.KERNEL_FACTOR * E.ORACLE_ERR[offset][0]
        assert err_iou <= E.KERNEL_FACTOR * E.ORACLE_ERR[offset][1]


def test_overlap_and_iou_matrix_shapes():
    from toda_amd import ops

    pa, pb = E.random_pairs(0.0)
    rng = np.random.default_rng(9)
    wide = np.concatenate([pb, pb[:1]])                        # 3 x 257 = 771 pairs: three full blocks of 256 and three more
    tol_area, tol_iou = (E.KERNEL_FACTOR * t for t in E.ORACLE_ERR[0.0])
    exact3 = E.exact_matrix(pa[:3], wide)
    for fn, want, tol in ((ops.boxes_overlap_bev, exact3[0], tol_area), (ops.boxes_iou_bev, exact3[1], tol_iou)):
        one = fn(dev(pa[:1]), dev(pb[:1]))
        assert one.shape == (1, 1) and abs(float(one) - want[0, 0]) <= tol
        got = fn(dev(pa[:3]), dev(wide)).cpu().numpy()
        assert got.shape == (3, 257)
        # accuracy on the entries that are pairs of the separated set - (i, i) and the repeated first partner in column 256 ...
        for i, j in ((0, 0), (1, 1), (2, 2), (0, 256)):
            assert abs(got[i, j] - want[i, j]) <= tol, (i, j)
        # ... and every entry bit-equal to the same pair computed as a diagonal entry of a square launch: the (row, column)
        # arithmetic of the flat thread index and the partly filled last block
        diag = fn(dev(np.repeat(pa[:3], 257, 0)), dev(np.tile(wide, (3, 1)))).diagonal().reshape(3, 257).cpu().numpy()
        assert np.array_equal(got, diag)
        flipped = fn(dev(wide), dev(pa[:3])).cpu().numpy()     # (257, 3)
        diag = fn(dev(np.tile(wide, (3, 1))), dev(np.repeat(pa[:3], 257, 0))).diagonal().reshape(3, 257).cpu().numpy()
        assert flipped.shape == (257, 3) and np.array_equal(flipped.T, diag)
        for i, j in ((0, 0), (1, 1), (2, 2), (0, 256)):
            assert abs(flipped[j, i] - want[i, j]) <= tol, (j, i)
        # 9 columns (velocity, class) are ignored; a non-contiguous view gives what its copy gives
        nine = np.concatenate([pa[:3], rng.standard_normal((3, 2)).astype(np.float32)], 1)
        assert torch.equal(fn(dev(nine), dev(wide)), fn(dev(pa[:3]), dev(wide)))
        big = dev(np.concatenate([wide, wide + 1], 1))          # [257, 14]
        strided, rows = big[:, :7], dev(np.repeat(pa[:3], 2, 0))[::2]
        assert not strided.is_contiguous() and not rows.is_contiguous()
        assert torch.equal(fn(rows, strided), fn(dev(pa[:3]), dev(wide)))
        for na, nb in ((0, 5), (5, 0), (0, 0)):                 # nothing to launch
            out = fn(dev(pa[:na]), dev(pb[:nb]))
            assert out.shape == (na, nb) and out.dtype == torch.float32


# ------------------------------------------------------------------------------- NMS
def nms(boxes, thresh):
    from toda_amd import ops

    keep, n_keep = ops.nms_rotated(dev(boxes), thresh)
    n = int(n_keep.item())
    return keep[:n].cpu().numpy(), n          # the tail of `keep` is unspecified


@pytest.mark.parametrize("n", [65, 129, 4160])
def test_nms_keeps_every_box_of_a_bare_lattice(n):
    keep, n_keep = nms(E.lattice(n), 0.5)
    assert n_keep == n and np.array_equal(keep, np.arange(n))


def test_nms_late_duplicates_across_word_64():
    boxes, want = E.late_duplicates()
    keep, n_keep = nms(boxes, 0.5)
    assert n_keep == len(want) and np.array_equal(keep, want)


def test_nms_all_identical_keeps_the_first():
    keep, n_keep = nms(np.repeat(E.lattice(1), 200, 0), 0.5)
    assert n_keep == 1 and keep.tolist() == [0]


@pytest.mark.parametrize("triple", E.CHAIN_TRIPLES)
def test_nms_chain_keeps_a_and_c(triple):
    boxes, want = E.chain(triple)
    keep, n_keep = nms(boxes, E.CHAIN_THRESH)
    assert triple[0] in keep and triple[2] in keep and triple[1] not in keep
    assert n_keep == len(want) and np.array_equal(keep, want)


def test_nms_empty_input_and_thresholds_outside_zero_one():
    keep, n_keep = nms(E.lattice(0), 0.5)
    assert n_keep == 0 and len(keep) == 0
    boxes, _ = E.late_duplicates()
    keep, n_keep = nms(boxes[:200], 1.5)                        # no IoU exceeds a threshold above 1: duplicates stay too
    assert n_keep == 200 and np.array_equal(keep, np.arange(200))
    keep, n_keep = nms(E.lattice(129), -1.0)                    # every IoU, 0 included, exceeds a negative threshold
    assert n_keep == 1 and keep.tolist() == [0]


def test_nms_pairwise_mask_is_the_strict_upper_triangle():
    """The workspace after toda_nms_rotated holds the pairwise pass's words, documented as bit j of word [row, col_block] =
    IoU(row, 64 col_block + j) > thresh for boxes after `row` only: no box marks itself or an earlier one."""
    from toda_amd import lib as L

    boxes, _ = E.chain((62, 63, 64), n=129)
    boxes[128] = boxes[0]
    lib = L.load()
    b = dev(boxes)
    n, cb = 129, 3
    ws_bytes = lib.toda_nms_workspace_bytes(n)
    assert ws_bytes >= n * cb * 8
    ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device="cuda")
    keep = torch.empty((n,), dtype=torch.int64, device="cuda")
    n_keep = torch.zeros((1,), dtype=torch.int32, device="cuda")
    L.check(lib.toda_nms_rotated(L.ptr(b), n, 0.5, L.ptr(keep), L.ptr(n_keep), L.ptr(ws), ws_bytes, L.stream()), "toda_nms_rotated")
    words = ws[:n * cb * 8].cpu().numpy().view(np.uint64).reshape(n, cb)
    assert np.array_equal(words, E.mask_words(E.aabb_iou(boxes), 0.5))
    assert int(n_keep.item()) == 127


def test_nms_wrappers_index_the_callers_arrays():
    from toda_amd.pcdet.config import AttrDict
    from toda_amd.pcdet.models.model_utils import model_nms_utils

    boxes, _ = E.chain((10, 100, 190))                          # sorted order: A = 10 removes B = 100, C = 190 stays
    n = len(boxes)
    perm = np.random.default_rng(4).permutation(n)              # position perm[r] of the caller's array holds the box of rank r
    scores = np.empty(n, np.float32)
    scores[perm] = np.linspace(0.99, 0.2, n, dtype=np.float32)
    shuffled = np.empty_like(boxes)
    shuffled[perm] = boxes
    want = perm[[i for i in range(n) if i != 100]]
    keep, _ = model_nms_utils.nms_gpu(dev(shuffled), dev(scores), 0.5)
    assert np.array_equal(keep.cpu().numpy(), want)             # indices into the unsorted input, in descending score order
    keep, _ = model_nms_utils.nms_gpu(dev(shuffled), dev(scores), 0.5, pre_maxsize=100)
    assert np.array_equal(keep.cpu().numpy(), perm[:100])       # cut before suppression: B's rank is 100, nothing is removed

    cfg = AttrDict(dict(NMS_TYPE="nms_gpu", NMS_THRESH=0.5, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=150))
    sel, sel_scores = model_nms_utils.class_agnostic_nms(dev(scores), dev(shuffled), cfg)
    assert np.array_equal(sel.cpu().numpy(), want[:150]) and torch.equal(sel_scores, dev(scores)[sel])
    thresh = float(scores[perm[199]])                           # ranks 0..199 pass the score threshold
    sel, sel_scores = model_nms_utils.class_agnostic_nms(dev(scores), dev(shuffled), cfg, score_thresh=thresh)
    want_masked = perm[[i for i in range(200) if i != 100]][:150]
    assert np.array_equal(sel.cpu().numpy(), want_masked)       # indices of the unmasked input
    assert torch.equal(sel_scores, dev(scores)[sel])
    cfg.NMS_PRE_MAXSIZE = 100
    sel, _ = model_nms_utils.class_agnostic_nms(dev(scores), dev(shuffled), cfg, score_thresh=thresh)
    assert np.array_equal(sel.cpu().numpy(), perm[:100])
    sel, sel_scores = model_nms_utils.class_agnostic_nms(dev(scores), dev(shuffled), cfg, score_thresh=2.0)
    assert sel.numel() == 0 and sel_scores.numel() == 0 and sel.dtype == torch.int64
