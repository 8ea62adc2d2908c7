"""The routing of the sparse gather-GEMM and weight-gradient launchers (csrc/spconv.hip: gather_route / gather_gemm_impl, toda_spconv_wgrad),
pinned at the row counts where the tile and grid arithmetic can go wrong: 1, one 16-row tile and one row more, two tiles and one row
more, one wave of the 64-row contract and one row more, and 257 rows = the first count that needs a second 256-thread workgroup of
two-row-tile waves (a partial tile AND a second per-workgroup statistics partial).  One channel pair per kernel family and matrix path.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

N_OUT = [1, 16, 17, 33, 64, 65, 257]
NATIVE = [(5, 16), (16, 16), (64, 32), (32, 64), (64, 64), (128, 64), (64, 128), (128, 128)]
SPLIT = [(32, 32), (64, 64), (32, 128), (128, 128)]
ROUTES = [("native", ci, co) for ci, co in NATIVE] + [("split", ci, co) for ci, co in SPLIT]
SHAPE, BATCH = [3, 10, 10], 1


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@pytest.fixture
def paths():
    """Switches the library's matrix path inside a test and puts the session's path back afterwards."""
    from toda_amd import ops

    before = ops.matrix_path()
    yield ops
    ops.set_matrix_path(before)


@functools.lru_cache(maxsize=None)
def table(n):
    """The first n cells (z, y, x row-major) of a 3 x 10 x 10 grid in a fixed shuffled order: every site has neighbours.  Computed once
    per row count and shared (read-only) by all tests: sites, the oracle's SubM table and a row permutation."""
    rng = np.random.default_rng(1000 + n)
    lin = np.arange(n)
    z, rem = np.divmod(lin, SHAPE[1] * SHAPE[2])
    y, x = np.divmod(rem, SHAPE[2])
    idx = np.stack([np.zeros_like(z), z, y, x], 1).astype(np.int32)[rng.permutation(n)]
    nbr0, _ = O.rulebook_subm(idx, BATCH, SHAPE)
    perm = rng.permutation(n).astype(np.int32)
    for a in (idx, nbr0, perm):
        a.setflags(write=False)
    return idx, nbr0, perm


def operands(cin, cout, n):
    rng = np.random.default_rng(cin * 131 + cout * 7 + n)
    feat = rng.standard_normal((n, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, 3, 3, 3, cin)) / np.sqrt(27 * cin)).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    return feat, w, bias


def stats_partials(ops, x, wp, nbr, cout, bias):
    """toda_spconv_gather_gemm_stats_partials into a statistics buffer of exactly the contract's size, pre-filled with NaN: what
    stays NaN was not written."""
    lib, L = ops.L.load(), ops.L
    K, n = nbr.shape
    out = torch.empty((n, cout), dtype=torch.float32, device=x.device)
    nd = lib.toda_spconv_gather_gemm_stats_doubles(n, cout)
    sums = torch.full((nd,), float("nan"), dtype=torch.float64, device=x.device)
    blocks = ctypes.c_int(0)
    rc = lib.toda_spconv_gather_gemm_stats_partials(L.ptr(x), x.shape[0], x.shape[1], L.ptr(wp), L.ptr(nbr), n, K, cout, L.ptr(bias), L.ptr(out),
                                                    L.ptr(sums), nd, ctypes.addressof(blocks), L.stream())
    L.check(rc, "toda_spconv_gather_gemm_stats_partials")
    return out, sums, int(blocks.value)


@pytest.mark.parametrize("mm,cin,cout", ROUTES)
def test_forward_routes(mm, cin, cout, paths):
    """Forward with bias against the oracle at the unchanged 1e-4; a permuted row order and the statistics launch change no bit of the
    output; folded moments = unfolded partials + the finalise-fold, bit for bit; `blocks` = the partial rows the kernel wrote."""
    ops = paths
    ops.set_matrix_path(mm)
    lib, L = ops.L.load(), ops.L
    assert bool(lib.toda_spconv_split_supported(cin, cout)) or mm == "native"
    with_stats = ops.gather_gemm_stats_supported(cin, cout)
    for n in N_OUT:
        idx, nbr0, perm = table(n)
        feat, w, bias = operands(cin, cout, n)
        rb, _ = ops.build_subm_rulebook(dev(idx), BATCH, SHAPE)
        assert rb.n_out == n and np.array_equal(rb.nbr_fwd.cpu().numpy(), nbr0)
        x, bt = dev(feat), dev(bias)
        wp = ops.pack_weight(dev(w), False, False)
        out = ops.gather_gemm(x, wp, rb.nbr_fwd, cout, bt)
        np.testing.assert_allclose(out.cpu().numpy(), O.spconv_fwd(feat, w, nbr0, bias), rtol=1e-4, atol=1e-4, err_msg=f"n_out {n}")
        assert torch.equal(ops.gather_gemm(x, wp, rb.nbr_fwd, cout, bt, order=dev(perm)), out), n
        if not with_stats:
            continue
        out_s, folded = ops.gather_gemm_with_stats(x, wp, rb.nbr_fwd, cout, bt)
        assert torch.equal(out_s, out), n
        out_p, part, blocks = stats_partials(ops, x, wp, rb.nbr_fwd, cout, bt)
        assert torch.equal(out_p, out), n
        # the scratch behind the 2 c result slots is [2 c][blocks]: exactly those entries were written, inside the contract's size
        written = ~torch.isnan(part[2 * cout:])
        assert blocks >= 1 and 2 * cout * (1 + blocks) <= part.numel(), (n, blocks, part.numel())
        assert int(written.sum()) == 2 * cout * blocks and bool(written[:2 * cout * blocks].all()), (n, blocks, int(written.sum()))
        # every output row is in exactly one partial: the partial sums add up to the column sums of the output
        np.testing.assert_allclose(part[2 * cout:2 * cout * (1 + blocks)].view(2 * cout, blocks).sum(1)[:cout].cpu().numpy(),
                                   out.double().sum(0).cpu().numpy(), rtol=1e-5, atol=1e-4, err_msg=f"n_out {n}")
        st = torch.empty((4, cout), dtype=torch.float32, device=x.device)
        rc = lib.toda_bn_finalize_partials(L.ptr(part), blocks, n, cout, None, None, None, None, 0.1, 1e-5, L.ptr(st[0]), L.ptr(st[1]), L.ptr(st[2]),
                                           L.ptr(st[3]), L.stream())
        L.check(rc, "toda_bn_finalize_partials")
        assert torch.equal(part[:2 * cout], folded[:2 * cout]), n      # same partials, same fixed fold order


@pytest.mark.parametrize("mm,cin,cout", ROUTES)
def test_wgrad_routes(mm, cin, cout, paths):
    """The weight gradient of every family at one row and at 257 rows against the oracle (tolerance of test_gpu_split)."""
    ops = paths
    ops.set_matrix_path(mm)
    for n in (1, 257):
        idx, nbr0, _ = table(n)
        feat, _, _ = operands(cin, cout, n)
        g = np.random.default_rng(n + cout).standard_normal((n, cout)).astype(np.float32)
        rb, _ = ops.build_subm_rulebook(dev(idx), BATCH, SHAPE)
        wshape = (cout, 3, 3, 3, cin)
        dw0 = O.spconv_wgrad(feat, g, nbr0, wshape)
        scale = float(np.sqrt((dw0.astype(np.float64) ** 2).mean()))
        dw = ops.wgrad(dev(feat), dev(g), rb.nbr_fwd, wshape)
        np.testing.assert_allclose(dw.cpu().numpy(), dw0, rtol=1e-4, atol=1e-4 * max(scale, 1.0), err_msg=f"n_out {n}")
