"""The sparse gather-GEMMs and weight gradients (csrc/spconv.hip, csrc/spconv_split.cuh; reference call sites
pcdet/models/backbones_3d/spconv_backbone.py:77-160) on the tables the other small tests do not use: strided and inverse tables, whose
gathered and produced row counts DIFFER, the (3, 1, 1) kernel, tables with empty offsets or one pair, and site sets of one residue
class for the class-sorted data gradient.  tests/test_gpu_spconv_edges.py and tests/test_gpu_spconv_routes.py pin the row-count edges on
submanifold K = 27 tables only; everything else was checked at 1100 rows or more, where no tile, queue or chunk is ragged.

Tables come from tests/spconv_table_cases.py (checked on the host by tests/test_spconv_tables_host.py).  Every result is compared with an fp64
evaluation of the same sums on the device (test_gpu_split.exact_sums / exact_wgrad) at the tolerances of the existing tests named at each
check.  Result buffers handed to the C ABI are pre-filled with NaN: what stays NaN was not written."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import spconv_table_cases as C
from tests.test_gpu_parity import CONV_GEOMS
from tests.test_gpu_split import dev, exact_sums, exact_wgrad, paths  # noqa: F401  (paths is a fixture)
from tests.test_gpu_spconv_routes import ROUTES, stats_partials

pytestmark = pytest.mark.gpu

NAN = float("nan")


def nans(shape, dtype=torch.float32):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


def no_nan(t):
    return not bool(torch.isnan(t).any())


# ---- the C ABI into NaN-filled result buffers -----------------------------------------------------------------------------------------
def gg(ops, x, wp, nbr, cp, bias=None, order=None):
    lib, L = ops.L.load(), ops.L
    K, n = nbr.shape
    out = nans((n, cp))
    L.check(lib.toda_spconv_gather_gemm_ordered(L.ptr(x), x.shape[0], x.shape[1], L.ptr(wp), L.ptr(nbr), n, K, cp, L.ptr(bias), L.ptr(out),
                                                L.ptr(order), L.stream()), "toda_spconv_gather_gemm_ordered")
    return out


def gg_classed(ops, x, wp, nbr, cp, order, cls, rb):
    lib, L = ops.L.load(), ops.L
    K, n = nbr.shape
    out = nans((n, cp))
    ks, st, pd = (L.host_i32(v) for v in (rb.ksize, rb.geom["stride"], rb.geom["padding"]))
    L.check(lib.toda_spconv_gather_gemm_classed(L.ptr(x), x.shape[0], x.shape[1], L.ptr(wp), L.ptr(nbr), n, K, cp, None, L.ptr(out), L.ptr(order),
                                                L.ptr(cls), L.hptr(ks), L.hptr(st), L.hptr(pd), L.stream()), "toda_spconv_gather_gemm_classed")
    return out


def class_order(ops, rb):
    """toda_rulebook_class_order into buffers pre-filled with -1 / 255."""
    lib, L = ops.L.load(), ops.L
    order = torch.full((rb.n_in,), -1, dtype=torch.int32, device="cuda")
    cls = torch.full((rb.n_in,), 255, dtype=torch.uint8, device="cuda")
    st, pd = L.host_i32(rb.geom["stride"]), L.host_i32(rb.geom["padding"])
    L.check(lib.toda_rulebook_class_order(L.ptr(rb.in_indices), rb.n_in, L.hptr(st), L.hptr(pd), L.ptr(order), L.ptr(cls), L.stream()),
            "toda_rulebook_class_order")
    return order, cls


def wg_bytes(ops, n_out, K, cin, cout):
    return int(ops.L.load().toda_spconv_wgrad_workspace_bytes(n_out, K, cin, cout))


def wg(ops, x, g, nbr, cin, cout):
    """toda_spconv_wgrad -> [cout, K, cin]; dw and the workspace (exactly the size the library asks for) start as NaN."""
    lib, L = ops.L.load(), ops.L
    K, n = nbr.shape
    dw = nans((cout, K, cin))
    nbytes = wg_bytes(ops, n, K, cin, cout)
    assert nbytes % 4 == 0
    ws = nans((max(nbytes // 4, 4),))
    L.check(lib.toda_spconv_wgrad(L.ptr(x), x.shape[0], L.ptr(g), L.ptr(nbr), n, K, cin, cout, L.ptr(dw), L.ptr(ws), nbytes, L.stream()),
            "toda_spconv_wgrad")
    return dw


def cg(ops, x, w, nbr, cp, bias=None, transpose=False, flip_k=False, stats=None):
    """toda_spconv_gather_gemm_compact[_stats]; stats: None | "folded" | "partials" -> out | (out, sums) | (out, sums, blocks)."""
    lib, L = ops.L.load(), ops.L
    K, n = nbr.shape
    out = nans((n, cp))
    head = (L.ptr(x), x.shape[0], x.shape[1], L.ptr(w), w.shape[0], w.shape[-1], int(transpose), int(flip_k), L.ptr(nbr), n, K, cp, L.ptr(bias), L.ptr(out))
    if stats is None:
        L.check(lib.toda_spconv_gather_gemm_compact(*head, L.stream()), "toda_spconv_gather_gemm_compact")
        return out
    nd = lib.toda_spconv_gather_gemm_compact_stats_doubles(n, cp)
    sums = nans((nd,), torch.float64)
    blocks = ctypes.c_int(-1)
    L.check(lib.toda_spconv_gather_gemm_compact_stats(*head, L.ptr(sums), nd, ctypes.addressof(blocks) if stats == "partials" else None, L.stream()),
            "toda_spconv_gather_gemm_compact_stats")
    return (out, sums, int(blocks.value)) if stats == "partials" else (out, sums)


# ---- operands, made once per shape and shared (read-only) -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows(n, c, seed=0):
    return dev(np.random.default_rng(10007 * n + 31 * c + seed).standard_normal((n, c)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def weights(K, cin, cout):
    rng = np.random.default_rng(1000 * cin + 10 * cout + K)
    w = (rng.standard_normal((cout,) + C.KSHAPE[K] + (cin,)) / np.sqrt(K * cin)).astype(np.float32)
    return dev(w), dev(rng.standard_normal(cout).astype(np.float32))


@functools.lru_cache(maxsize=None)
def hand(K, n_gather, n_produce, fill):
    """The table on the device and the produced rows that have no pair."""
    t = C.hand_table(K, n_gather, n_produce, fill, seed=17 * K + n_gather + C.FILLS.index(fill))
    return dev(np.array(t)), dev((t < 0).all(0))      # (a copy: the cases are read-only arrays)


@functools.lru_cache(maxsize=None)
def perm(n):
    return dev(np.random.default_rng(n).permutation(n).astype(np.int32))


def moments(out):
    o = out.double()
    return torch.cat([o.sum(0), (o * o).sum(0)]).cpu().numpy()


def close(got, ref, what, rtol=1e-4, atol=1e-4):
    np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=rtol, atol=atol, err_msg=str(what))


# ---- a. gather-GEMM on hand tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm,cin,cout", ROUTES)
def test_gather_gemm_on_hand_tables(mm, cin, cout, paths):
    """Every kernel family under both matrix paths (ROUTES), K = 27 and 3, five (gathered, produced) row counts, five fills: the forward
    operand with bias and the transposed operand (offsets in table order and reversed) against fp64 at the 1e-4 of test_gpu_spconv_edges;
    a produced row without a pair is the bias (or zero) exactly; every element is written; run twice: same bits; a permuted row order
    changes no bit; the statistics launch changes no bit, its sums are those of the stored output (tolerances of
    test_epilogue_moments_with_one_live_row_in_the_last_workgroup) and it writes exactly 2 cout partials per workgroup."""
    ops = paths
    ops.set_matrix_path(mm)
    with_stats = ops.gather_gemm_stats_supported(cin, cout)
    assert cout <= 16 or cout % 4 == 0      # the library's rule for a gathered side: every pair of ROUTES has a transposed operand
    for K in C.K_VOLS:
        w, bias = weights(K, cin, cout)
        wp = ops.pack_weight(w, False, False)
        wp_t = {flip: ops.pack_weight(w, True, flip) for flip in (False, True)}
        for n_g, n_p in C.SIZES:
            x, g = rows(n_g, cin), rows(n_g, cout, 1)
            for fill in C.FILLS:
                what = (mm, cin, cout, K, n_g, n_p, fill)
                nbr, bare = hand(K, n_g, n_p, fill)
                out = gg(ops, x, wp, nbr, cout, bias)
                assert no_nan(out), what
                close(out, exact_sums(x, w, nbr, False, False) + bias.double(), what)
                assert torch.equal(out[bare], bias.expand(int(bare.sum()), cout)), what
                assert torch.equal(gg(ops, x, wp, nbr, cout, bias), out), what
                assert torch.equal(gg(ops, x, wp, nbr, cout, bias, order=perm(n_p)), out), what
                plain = gg(ops, x, wp, nbr, cout)
                assert no_nan(plain) and not bool(plain[bare].any()), what      # no pair, no bias: zeros
                for flip in (False, True):
                    d = gg(ops, g, wp_t[flip], nbr, cin)
                    assert no_nan(d), what + (flip,)
                    close(d, exact_sums(g, w, nbr, True, flip), what + (flip,))
                    assert not bool(d[bare].any()), what + (flip,)
                    assert torch.equal(gg(ops, g, wp_t[flip], nbr, cin, order=perm(n_p)), d), what + (flip,)
                if not with_stats:
                    continue
                want = moments(out)
                out_s, folded = ops.gather_gemm_with_stats(x, wp, nbr, cout, bias)
                assert torch.equal(out_s, out), what
                np.testing.assert_allclose(folded[:2 * cout].cpu().numpy(), want, rtol=1e-5, atol=1e-3, err_msg=str(what))
                out_p, part, blocks = stats_partials(ops, x, wp, nbr, cout, bias)
                assert torch.equal(out_p, out), what
                written = ~torch.isnan(part[2 * cout:])
                assert blocks >= 1 and 2 * cout * (1 + blocks) <= part.numel(), what
                assert int(written.sum()) == 2 * cout * blocks and bool(written[:2 * cout * blocks].all()), what + (blocks, int(written.sum()))
                np.testing.assert_allclose(part[2 * cout:2 * cout * (1 + blocks)].view(2 * cout, blocks).sum(1).cpu().numpy(), want, rtol=1e-5, atol=1e-3,
                                           err_msg=str(what))


# ---- b. weight gradient on hand tables -----------------------------------------------------------------------------------------------
def check_wgrad(ops, x, g, nbr_h, nbr, cin, cout, what):
    K = nbr.shape[0]
    ref = exact_wgrad(x, g, nbr, cout, cin)
    scale = max(float(ref.pow(2).mean().sqrt()), 1.0)
    dw = wg(ops, x, g, nbr, cin, cout)
    assert no_nan(dw), what
    close(dw, ref, what, rtol=1e-4, atol=1e-4 * scale)      # the tolerance of test_gpu_spconv_edges
    for k in range(K):
        if not (nbr_h[k] >= 0).any():
            assert not bool(dw[:, k, :].any()), what + (k,)
    assert torch.equal(wg(ops, x, g, nbr, cin, cout), dw), what


@pytest.mark.parametrize("mm,cin,cout", ROUTES)
def test_wgrad_on_hand_tables(mm, cin, cout, paths):
    """Queues that never fill a round, that hold one pair, that take every row of the chunk from ONE gathered row, and offsets without a
    pair, with the gathered rows fewer and more than the produced ones."""
    ops = paths
    ops.set_matrix_path(mm)
    for K in C.K_VOLS:
        for n_g, n_p in ((1, 129), (129, 1), (300, 257)):
            x, g = rows(n_g, cin), rows(n_p, cout, 2)
            for fill in C.FILLS:
                nbr, _ = hand(K, n_g, n_p, fill)
                check_wgrad(ops, x, g, nbr.cpu().numpy(), nbr, cin, cout, (mm, cin, cout, K, n_g, n_p, fill))


WGRAD_EDGE = {27: 4096, 3: 2048}      # wgrad_plan: the first produced-row count that takes two chunks


@pytest.mark.parametrize("K", [27, 3])
@pytest.mark.parametrize("mm,cin,cout", [("native", 16, 16), ("native", 64, 64), ("split", 64, 64), ("native", 128, 128), ("split", 128, 128)])
def test_wgrad_at_the_chunk_edge(mm, cin, cout, K, paths):
    """One row below, at and one above the produced-row count where the plan goes from one chunk to two (the second chunk's slab, the
    fold over two slabs, a last chunk of one row less / the same / 16 rows less than the first).  The workspace grows by exactly one slab
    there - the edge is where this test believes it is."""
    ops = paths
    ops.set_matrix_path(mm)
    edge, slab = WGRAD_EDGE[K], K * cin * cout * 4
    assert slab % 256 == 0
    assert [wg_bytes(ops, n, K, cin, cout) for n in (edge - 1, edge, edge + 1)] == [slab, 2 * slab, 2 * slab]
    n_g = 1000
    x = rows(n_g, cin)
    for n_p in (edge - 1, edge, edge + 1):
        g = rows(n_p, cout, 2)
        for fill in ("sparse", "full"):
            nbr, _ = hand(K, n_g, n_p, fill)
            check_wgrad(ops, x, g, nbr.cpu().numpy(), nbr, cin, cout, (mm, cin, cout, K, n_p, fill))


# ---- c. the compacting narrow kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_g", [1, 40])
@pytest.mark.parametrize("c_g,c_p", [(5, 16), (16, 16), (16, 32), (32, 16), (18, 16)])      # every <Q, VEC> instantiation
def test_compacting_kernel_on_hand_tables(c_g, c_p, n_g):
    """gather_gemm_compact_kernel (256 rows per workgroup, 64 per wave, LDS queue of depth 3) around one wave, one workgroup and one
    row, with the gathered rows fewer than / different from the produced ones (same_row and n_g = 1: 64 pairs of one offset and wave on
    ONE gathered row, four compacted tiles).  Tolerances of test_compacting_narrow_gather_gemm_matches_the_output_stationary_kernel."""
    from toda_amd import ops

    K = 27
    w, bias = weights(K, c_g, c_p)
    x, g = rows(n_g, c_g), rows(n_g, c_p, 1)
    assert ops.gather_gemm_compact_supported(c_g, c_p, K)
    for n_p in (1, 63, 64, 65, 255, 256, 257):
        for fill in C.FILLS:
            what = (c_g, c_p, n_g, n_p, fill)
            nbr, bare = hand(K, n_g, n_p, fill)
            ref = exact_sums(x, w, nbr, False, False) + bias.double()
            out = cg(ops, x, w, nbr, c_p, bias)
            assert no_nan(out), what
            close(out, ref, what, rtol=0, atol=1e-4 * float(ref.abs().max()))
            assert torch.equal(out[bare], bias.expand(int(bare.sum()), c_p)), what
            assert torch.equal(cg(ops, x, w, nbr, c_p, bias), out), what
            if c_g % 4 == 0:      # the transposed operand gathers c_p channels and produces c_g (a multiple of 4)
                for flip in (False, True):
                    ref_t = exact_sums(g, w, nbr, True, flip)
                    d = cg(ops, g, w, nbr, c_g, None, True, flip)
                    assert no_nan(d), what + (flip,)
                    close(d, ref_t, what + (flip,), rtol=0, atol=1e-4 * float(ref_t.abs().max()))
                    assert torch.equal(cg(ops, g, w, nbr, c_g, None, True, flip), d), what + (flip,)
            want = moments(out)
            out_s, part, blocks = cg(ops, x, w, nbr, c_p, bias, stats="partials")
            assert torch.equal(out_s, out) and blocks == (n_p + 255) // 256, what + (blocks,)
            written = ~torch.isnan(part[2 * c_p:])
            assert int(written.sum()) == 2 * c_p * blocks and bool(written[:2 * c_p * blocks].all()), what
            np.testing.assert_allclose(part[2 * c_p:2 * c_p * (1 + blocks)].view(2 * c_p, blocks).sum(1).cpu().numpy(), want, rtol=1e-6, atol=1e-4,
                                       err_msg=str(what))
            out_f, folded = cg(ops, x, w, nbr, c_p, bias, stats="folded")
            assert torch.equal(out_f, out), what
            np.testing.assert_allclose(folded[:2 * c_p].cpu().numpy(), want, rtol=1e-6, atol=1e-4, err_msg=str(what))


# ---- d. the class-sorted data gradient on geometric sets ---------------------------------------------------------------------------
CLASSED = [("native", 16, 32), ("native", 64, 64), ("split", 64, 64), ("native", 32, 32), ("split", 32, 32)]


def strided(ops, sites, shape, geom):
    ks, st, pd = geom
    return ops.build_conv_rulebook(dev(np.array(sites)), C.BATCH, list(shape), ks, st, pd)[2]


def classed_equals_plain(ops, rb, geom, cin, cout, what):
    """The data gradient of the strided layer (gathers cout channels of the produced sites, produces cin for the input sites): plain,
    against fp64, and over class-sorted rows."""
    ks = geom[0]
    K = int(np.prod(ks))
    w, _ = weights(K, cin, cout)
    g = rows(rb.n_out, cout, 3)
    wp_t = ops.pack_weight(w, True, False)
    plain = gg(ops, g, wp_t, rb.nbr_bwd, cin)
    assert no_nan(plain), what
    close(plain, exact_sums(g, w, rb.nbr_bwd, True, False), what)
    order, cls = class_order(ops, rb)
    got = gg_classed(ops, g, wp_t, rb.nbr_bwd, cin, order, cls, rb)
    assert torch.equal(got, plain), what
    return order, cls


@pytest.mark.parametrize("mm,cin,cout", CLASSED)
@pytest.mark.parametrize("ks,st,pd", CONV_GEOMS)
def test_classed_dgrad_on_sets_of_one_class(ks, st, pd, mm, cin, cout, paths, monkeypatch):
    """1, 33 and 129 input sites of ONE residue class, every class of the geometry (the class with one candidate offset - the split
    kernel's stage loop over a single offset - and the class with eight among them): every wave and workgroup holds live rows of one class and
    rows past the end.  gather_gemm_kernel<CLS> (native) / the `listed` branch of gg_split_kernel against the plain launch, bit for bit."""
    ops = paths
    ops.set_matrix_path(mm)
    monkeypatch.setattr(ops, "CLASS_DGRAD_MIN_ROWS", 0)
    monkeypatch.setattr(ops, "COMPACT", False)
    geom = (ks, st, pd)
    lists = C.class_offsets(ks, st)
    assert {len(v) for v in lists} >= ({1, 8} if st == (2, 2, 2) else {1, 2})
    for c, residue in enumerate(C.residues(st)):
        for n in C.ONE_CLASS_ROWS:
            what = (geom, mm, cin, cout, residue, n)
            sites = C.one_class(geom, residue, n)
            rb = strided(ops, sites, C.ONE_CLASS_SHAPE, geom)
            assert rb.n_in == n and rb.n_out >= 1
            order, cls = classed_equals_plain(ops, rb, geom, cin, cout, what)
            assert bool((cls == c).all()) and torch.equal(order, torch.arange(n, dtype=torch.int32, device="cuda")), what
            by_ops = rb.class_order()      # what the autograd path passes on (None below CLASS_DGRAD_MIN_ROWS)
            assert by_ops is not None and torch.equal(by_ops[0], order) and torch.equal(by_ops[1], cls), what
            # only the class's candidate offsets hold pairs
            used = (rb.nbr_bwd >= 0).any(1).cpu().numpy()
            assert set(np.nonzero(used)[0].tolist()) <= set(lists[c]), what


@pytest.mark.parametrize("ks,st,pd", CONV_GEOMS)
def test_class_order_at_the_block_edge(ks, st, pd, paths):
    """toda_rulebook_class_order at 8191, 8192 and 8193 rows (one block less a row, one block, a second block of ONE row): a
    permutation, the classes of the rows it names, blocks closed under it, classes ascending and rows of a class in their original order
    inside a block (the counting sort is stable)."""
    ops = paths
    geom = (ks, st, pd)
    for n in C.MIXED_ROWS:
        sites = C.mixed(geom, n)
        rb = strided(ops, sites, C.MIXED_SHAPE, geom)
        order, cls = class_order(ops, rb)
        order, cls = order.cpu().numpy().astype(np.int64), cls.cpu().numpy().astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(n)), n
        assert np.array_equal(cls, C.site_class(sites, st, pd)[order]), n
        for b0 in range(0, n, 8192):
            o, c = order[b0:b0 + 8192], cls[b0:b0 + 8192]
            assert o.min() == b0 and o.max() == min(n, b0 + 8192) - 1, (n, b0)
            assert (np.diff(c) >= 0).all(), (n, b0)
            for k in np.unique(c):
                assert (np.diff(o[c == k]) > 0).all(), (n, b0, k)


@pytest.mark.parametrize("mm,cin,cout", CLASSED)
@pytest.mark.parametrize("ks,st,pd", CONV_GEOMS)
def test_classed_dgrad_on_mixed_sets(ks, st, pd, mm, cin, cout, paths):
    """Class-sorted blocks of 8191, 8192 and 8193 rows of every class: waves of one class, waves that straddle two classes (they walk all
    K offsets) and the ragged last wave, against the plain launch bit for bit."""
    ops = paths
    ops.set_matrix_path(mm)
    geom = (ks, st, pd)
    for n in C.MIXED_ROWS:
        rb = strided(ops, C.mixed(geom, n), C.MIXED_SHAPE, geom)
        classed_equals_plain(ops, rb, geom, cin, cout, (geom, mm, cin, cout, n))


@pytest.mark.parametrize("mm,cin,cout", CLASSED)
@pytest.mark.parametrize("ks,st,pd", CONV_GEOMS)
def test_strided_conv_backward_on_sets_of_one_class(ks, st, pd, mm, cin, cout, paths, monkeypatch):
    """ops.sparse_conv forward and backward (the data gradient through the class-sorted kernel) on the 1, 33 and 129 site sets against the
    CPU oracle, tolerances of test_gpu_parity.test_strided_conv_fwd_dgrad_wgrad."""
    ops = paths
    ops.set_matrix_path(mm)
    monkeypatch.setattr(ops, "CLASS_DGRAD_MIN_ROWS", 0)
    monkeypatch.setattr(ops, "COMPACT", False)
    calls = []
    orig = ops.gather_gemm_classed
    monkeypatch.setattr(ops, "gather_gemm_classed", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    geom = (ks, st, pd)
    K = int(np.prod(ks))
    w_dev, _ = weights(K, cin, cout)
    w = w_dev.cpu().numpy()
    n_sets = 0
    for residue in C.residues(st):
        for n in C.ONE_CLASS_ROWS:
            what = (geom, mm, cin, cout, residue, n)
            sites = C.one_class(geom, residue, n)
            feat = rows(n, cin).cpu().numpy()
            _, _, o2i0, i2o0, _ = O.rulebook_conv(sites, C.BATCH, list(C.ONE_CLASS_SHAPE), ks, st, pd)
            g = rows(o2i0.shape[1], cout, 3).cpu().numpy()
            out0 = O.spconv_fwd(feat, w, o2i0)
            din0 = O.spconv_dgrad(g, w, i2o0, flip_k=False)
            dw0 = O.spconv_wgrad(feat, g, o2i0, w.shape)
            rb = strided(ops, sites, C.ONE_CLASS_SHAPE, geom)
            assert np.array_equal(rb.nbr_fwd.cpu().numpy(), o2i0) and np.array_equal(rb.nbr_bwd.cpu().numpy(), i2o0), what
            x, wt = dev(feat).requires_grad_(True), w_dev.clone().requires_grad_(True)
            out = ops.sparse_conv(x, wt, None, rb)
            out.backward(dev(g))
            n_sets += 1
            np.testing.assert_allclose(out.detach().cpu().numpy(), out0, rtol=1e-4, atol=1e-4, err_msg=str(what))
            np.testing.assert_allclose(x.grad.cpu().numpy(), din0, rtol=1e-4, atol=1e-4, err_msg=str(what))
            np.testing.assert_allclose(wt.grad.cpu().numpy(), dw0, rtol=1e-4, atol=1e-4 * np.abs(dw0).max(), err_msg=str(what))
    assert len(calls) == n_sets


# ---- e. inverse convolution ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("cin,cout", [(64, 32), (32, 16)])
def test_inverse_conv_at_one_and_33_sites(cin, cout, n):
    """spconv.SparseInverseConv3d over the tables of a strided layer with 1 and 33 input sites (fewer gathered rows than produced ones
    in the forward, more in the data gradient): the assertions of test_inverse_conv_forward_and_gradients_against_the_oracle."""
    from toda_amd import spconv

    shape, batch = list(C.ONE_CLASS_SHAPE), C.BATCH
    idx = C.clustered(n)
    feat_lo = rows(n, cout, 4)
    torch.manual_seed(cin)
    down = spconv.SparseConv3d(cout, cin, 3, stride=2, padding=1, bias=False, indice_key="spconv2").cuda()
    up = spconv.SparseInverseConv3d(cin, cout, 3, indice_key="spconv2", bias=False).cuda()
    x = spconv.SparseConvTensor(feat_lo, dev(np.array(idx)), shape, batch)
    mid = down(x)
    hi = mid.features.detach().clone().requires_grad_(True)
    out = up(mid.replace_feature(hi))
    assert out.spatial_shape == shape and torch.equal(out.indices, x.indices) and out.features.shape == (n, cout)

    idx_out, _, o2i, i2o, _ = O.rulebook_conv(idx, batch, shape, 3, 2, 1)
    assert np.array_equal(idx_out, mid.indices.cpu().numpy()) and len(idx_out) != n
    w = up.weight.detach().cpu().numpy()
    f = hi.detach().cpu().numpy()
    ref = O.spconv_fwd(f, w, i2o)
    np.testing.assert_allclose(out.features.detach().cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    g = np.random.default_rng(1).standard_normal(ref.shape).astype(np.float32)
    out.features.backward(dev(g))
    np.testing.assert_allclose(hi.grad.cpu().numpy(), O.spconv_dgrad(g, w, o2i, flip_k=False), rtol=1e-4, atol=1e-4)
    dw = O.spconv_wgrad(f, g, i2o, w.shape)
    np.testing.assert_allclose(up.weight.grad.cpu().numpy(), dw, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(dw).max())))


# ---- f. empty tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [27, 3])
@pytest.mark.parametrize("mm,cin,cout", [("native", 16, 16), ("native", 64, 64), ("split", 64, 64), ("native", 128, 128), ("split", 128, 128)])
def test_empty_tables(mm, cin, cout, K, paths):
    ops = paths
    ops.set_matrix_path(mm)
    lib, L = ops.L.load(), ops.L
    w, bias = weights(K, cin, cout)
    wp = ops.pack_weight(w, False, False)
    x = rows(7, cin)
    # no produced rows: success, and not one element behind the (empty) result is touched
    guard = nans((4, cout))
    none = torch.empty((K, 0), dtype=torch.int32, device="cuda")
    L.check(lib.toda_spconv_gather_gemm_ordered(L.ptr(x), 7, cin, L.ptr(wp), L.ptr(none), 0, K, cout, L.ptr(bias), L.ptr(guard), None, L.stream()),
            "toda_spconv_gather_gemm_ordered")
    assert bool(torch.isnan(guard).all())
    # no gathered rows: zeros without a bias, the documented refusal with one
    nobody = torch.empty((0, cin), dtype=torch.float32, device="cuda")
    absent = torch.full((K, 33), -1, dtype=torch.int32, device="cuda")
    out = gg(ops, nobody, wp, absent, cout)
    assert out.shape == (33, cout) and not bool(out.any()) and no_nan(out)
    with pytest.raises(RuntimeError, match="empty input with bias"):
        gg(ops, nobody, wp, absent, cout, bias)
    # weight gradient without rows on either side: zeros, whatever the workspace holds
    g33, g0 = rows(33, cout, 2), torch.empty((0, cout), dtype=torch.float32, device="cuda")
    for xx, gg_, tab in ((nobody, g33, absent), (x, g0, none)):
        dw = wg(ops, xx, gg_, tab, cin, cout)
        assert dw.shape == (cout, K, cin) and not bool(dw.any()) and no_nan(dw)


@pytest.mark.parametrize("c_g,c_p", [(5, 16), (16, 32)])
def test_empty_tables_compacting_kernel(c_g, c_p):
    from toda_amd import ops

    lib, L = ops.L.load(), ops.L
    w, bias = weights(27, c_g, c_p)
    x = rows(7, c_g)
    guard = nans((4, c_p))
    none = torch.empty((27, 0), dtype=torch.int32, device="cuda")
    L.check(lib.toda_spconv_gather_gemm_compact(L.ptr(x), 7, c_g, L.ptr(w), c_p, c_g, 0, 0, L.ptr(none), 0, 27, c_p, L.ptr(bias), L.ptr(guard), L.stream()),
            "toda_spconv_gather_gemm_compact")
    assert bool(torch.isnan(guard).all())
    # a table without a pair over 7 gathered rows: the bias alone, or zeros
    absent = torch.full((27, 65), -1, dtype=torch.int32, device="cuda")
    assert torch.equal(cg(ops, x, w, absent, c_p, bias), bias.expand(65, c_p))
    assert not bool(cg(ops, x, w, absent, c_p).any())
