"""The row passes and scatters of csrc/dense.hip without a GPU: the float64 references of tests/rows_cases.py against torch's
float64 autograd, the seeds of its case table, the size queries against their documented plans, and the argument checks that
return -1 with a message before anything is launched or dereferenced."""
import ctypes

import numpy as np
import pytest
import torch

from tests import rows_cases as R
from toda_amd import lib as L

FAKE = 4096        # a non-null "device pointer" for arguments a refused call must not touch


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def refused(rc, *words):
    msg = L.load().toda_last_error().decode()
    return rc == -1 and all(w in msg for w in words)


# ------------------------------------------------------------------------------- references against torch float64
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("n,c", [(n, c) for n in (2, 65, 513) for c in (4, 128)])
def test_references_match_torch_float64_autograd(n, c, train, relu, residual):
    case = R.Case(n, c, residual, False, seed=1000 * c + n + 7919 * R.find_bump(n, c, residual, False))
    rng = np.random.default_rng(n + c)
    rm0, rv0 = rng.uniform(-0.2, 0.2, c), rng.uniform(0.5, 2.0, c)
    bn = torch.nn.BatchNorm1d(c, eps=R.EPS, momentum=R.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(case.gamma.astype(np.float64)))
        bn.bias.copy_(torch.from_numpy(case.beta.astype(np.float64)))
        bn.running_mean.copy_(torch.from_numpy(rm0))
        bn.running_var.copy_(torch.from_numpy(rv0))
    bn.train(train)
    x = torch.from_numpy(case.x).double().requires_grad_(True)
    r = torch.from_numpy(case.res).double().requires_grad_(True) if residual else None
    pre = bn(x) + r if residual else bn(x)
    y = torch.relu(pre) if relu else pre
    y.backward(torch.from_numpy(case.dy).double())

    x64 = case.x.astype(np.float64)
    sums = np.concatenate([x64.sum(0), (x64 * x64).sum(0)])
    mean, invstd, scale, shift, rm1, rv1 = R.finalize(sums, n, case.gamma, case.beta, rm0, rv0, R.MOMENTUM, R.EPS, train)
    mine = x64 * scale + shift + (case.res.astype(np.float64) if residual else 0.0)
    assert rel(mine, pre.detach().numpy()) < 1e-12
    assert rel(rm1, bn.running_mean.numpy()) < 1e-12 and rel(rv1, bn.running_var.numpy()) < 1e-12
    if not train:
        assert np.array_equal(rm1, rm0) and np.array_equal(rv1, rv0) and np.array_equal(mean, rm0)
        return
    # the case's own float32 stats are this float64 result, cast
    np.testing.assert_allclose(case.stats, np.stack([mean, invstd, scale, shift]), rtol=1e-6, atol=1e-7)
    # the float32 mask is the float64 mask on this seed
    assert np.abs(pre.detach().numpy()).min() > 1e-4
    assert np.array_equal(case.pre32() > 0, pre.detach().numpy() > 0)
    assert np.array_equal(case.pre32() > 0, case.pre64() > 0)
    dz, dbeta, dgamma, dx = R.bn_bwd(case.dy, case.x, case.res, np.stack([mean, invstd, scale, shift]), case.gamma, relu)
    assert rel(dx, x.grad.numpy()) < 1e-12
    assert rel(dbeta, bn.bias.grad.numpy()) < 1e-12 and rel(dgamma, bn.weight.grad.numpy()) < 1e-12
    if residual:
        assert rel(dz, r.grad.numpy()) < 1e-12


def test_finalize_reference_for_one_row_uses_the_biased_variance():
    _, _, _, _, rm, rv = R.finalize(np.array([3.0, 10.0]), 1, None, None, np.array([0.0]), np.array([1.0]), 0.5, 1e-3, True)
    assert rm[0] == 1.5 and rv[0] == 0.5 + 0.5 * (10.0 - 9.0)


@pytest.mark.parametrize("c", R.ROW_C)
def test_case_table_seeds_keep_every_pre_activation_away_from_zero(c):
    """What lets the GPU tests compare every element of the small cases: on the table's seeds no pre-activation lies within 1e-4
    of zero, for either mean and with or without the shortcut, so float32 and float64 agree on the whole ReLU mask."""
    small = [(n, cc) for n, cc in R.ROW_CASES if cc == c and n * cc <= R.SMALL]
    assert small
    for n, _ in small:
        for residual in (False, True):
            for shifted in (False, True):
                case = R.Case(n, c, residual, shifted)
                assert np.abs(case.pre64()).min() > 1e-4, (n, c, residual, shifted)
                assert np.array_equal(case.pre32() > 0, case.pre64() > 0)


def test_case_tables_reach_the_edges_they_are_meant_for():
    for c in R.ROW_C:
        rp = 1024 // c
        assert {rp - 1, rp, rp + 1, 2 * rp, 2 * rp + 1, 255, 256, 257, 513} - {0} <= set(R.row_counts(c))
    (n0, c0), (n1, c1), (n2, c2) = R.CAPPED
    assert -(-n0 // 256) > 2048 and -(-n1 // 256) > 2048                      # the row grid is capped, rows_per_block grows
    assert R.reduce_plan(n0) == (2048, 257) and 2047 * 257 >= n0              # ... and the last blocks have an empty stripe
    assert n0 * c0 // 4 > 2048 * 256 and n2 * c2 // 4 > 2048 * 256             # the elementwise grid is capped
    for n, c in R.AFFINE_CASES:
        assert c % 4 == 0 and (n < 300 or 0 < n * c // 4 - 2048 * 256 <= c // 4)
    assert any(1024 % c for c in R.AFFINE_C)
    for n, c in R.CAPPED:
        assert 8e6 <= n * c * 4 <= 17e6


# ------------------------------------------------------------------------------- size queries
@pytest.mark.parametrize("c", [4, 8, 64, 128])
def test_reduce_doubles_follows_its_documented_plan(c):
    lib = L.load()
    for n in (0, 1, 256, 257, 524288, 524289, 2 ** 30):
        want = 2 * c * (1 + min(2048, -(-max(n, 1) // 256)))
        assert lib.toda_rows_reduce_doubles(n, c) == want == R.reduce_doubles(n, c), (n, c)


@pytest.mark.parametrize("c", [4, 8, 12, 20, 64, 96, 100, 128, 384, 1000, 1024])
def test_colsum_doubles_follows_its_documented_plan(c):
    lib = L.load()
    for n in (-1, 0):
        assert lib.toda_rows_bn_bwd_colsum_doubles(n, c) == 1 == R.colsum_doubles(n, c)
        assert R.ew_blocks(n, c) == R.ew_blocks(1, c) >= 1                  # no rows: still the one (rounded-up) block of the plan
    for n in (1, 3, 255, 256, 257, 1023, 16385, 2048 * 256 * 4 // c, 2048 * 256 * 4 // c + 1, 524289, 2 ** 21):
        g = min(2048, -(-(n * c // 4) // 256))
        while g * 1024 % c:
            g += 1
        assert lib.toda_rows_bn_bwd_colsum_doubles(n, c) == c * g == c * R.ew_blocks(n, c) == R.colsum_doubles(n, c), (n, c)


# ------------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize("c", [0, 2, 12, 20, 256])
def test_row_reductions_refuse_channel_counts_outside_their_plan(c):
    lib = L.load()
    assert refused(lib.toda_rows_moments(FAKE, 10, c, FAKE, None), "rows_moments", "got %d" % c)
    assert refused(lib.toda_rows_bn_bwd(FAKE, FAKE, FAKE, FAKE, 10, c, 1, FAKE, FAKE, None), "rows_bn_bwd", "got %d" % c)
    assert refused(lib.toda_rows_bn_bwd_res(FAKE, FAKE, FAKE, FAKE, FAKE, 10, c, 1, FAKE, FAKE, FAKE, None), "rows_bn_bwd", "got %d" % c)


def test_affine_act_refuses_bad_channels_and_accepts_no_rows():
    lib = L.load()
    for c in (2, 6, 1028):
        assert refused(lib.toda_rows_affine_act(FAKE, FAKE, FAKE, None, 10, c, 1, FAKE, None), "rows_affine_act", "got %d" % c)
    for c in (4, 12, 1024):
        assert lib.toda_rows_affine_act(FAKE, FAKE, FAKE, FAKE, 0, c, 1, FAKE, None) == 0


def test_bn_finalize_refuses_bad_sizes_before_it_launches():
    lib = L.load()
    args = (FAKE, FAKE, FAKE, FAKE, R.MOMENTUM, R.EPS)
    outs = (FAKE, FAKE, FAKE, FAKE, None)
    for c in (0, 257):
        assert refused(lib.toda_bn_finalize(FAKE, 10, c, *args, 1, *outs), "bn_finalize", "got %d" % c)
    assert refused(lib.toda_bn_finalize(FAKE, 10, 64, FAKE, FAKE, None, None, R.MOMENTUM, R.EPS, 0, *outs), "eval mode")
    assert refused(lib.toda_bn_finalize(FAKE, 10, 64, FAKE, FAKE, FAKE, None, R.MOMENTUM, R.EPS, 0, *outs), "eval mode")
    # training mode divides the sums by n: no rows is an argument error, as in toda_bn_finalize_partials
    for n in (0, -3):
        assert refused(lib.toda_bn_finalize(FAKE, n, 64, *args, 1, *outs), "bn_finalize", "rows")


def test_bn_finalize_partials_refuses_bad_sizes_before_it_launches():
    lib = L.load()
    tail = (R.MOMENTUM, R.EPS, FAKE, FAKE, FAKE, FAKE, None)
    assert refused(lib.toda_bn_finalize_partials(FAKE, 0, 10, 64, FAKE, FAKE, FAKE, FAKE, *tail), "bn_finalize_partials")
    assert refused(lib.toda_bn_finalize_partials(FAKE, 4, 0, 64, FAKE, FAKE, FAKE, FAKE, *tail), "bn_finalize_partials")
    assert refused(lib.toda_bn_finalize_partials(FAKE, 4, 10, 257, FAKE, FAKE, FAKE, FAKE, *tail), "bn_finalize_partials", "got 257")
    assert refused(lib.toda_bn_finalize_partials(FAKE, 4, 10, 64, FAKE, FAKE, FAKE, None, *tail), "go together")
    assert refused(lib.toda_bn_finalize_partials(FAKE, 4, 10, 64, FAKE, FAKE, None, FAKE, *tail), "go together")
    assert refused(lib.toda_bn_finalize_partials(None, 4, 10, 64, FAKE, FAKE, FAKE, FAKE, *tail), "null")


def test_bn_bwd_colsum_needs_workspace_and_result_together():
    lib = L.load()
    for ws, out in ((FAKE, None), (None, FAKE)):
        rc = lib.toda_rows_bn_bwd_res_colsum(FAKE, FAKE, None, FAKE, FAKE, 10, 64, 1, FAKE, FAKE, None, ws, out, None)
        assert refused(rc, "go together")


def test_scatters_refuse_empty_channel_or_batch_dimensions():
    lib = L.load()
    shape = L.host_i32(R.DENSE_SHAPE)
    for c, batch in ((0, 1), (4, 0), (-1, 2)):
        for fn in (lib.toda_sparse_to_dense_fwd, lib.toda_sparse_to_dense_bwd):
            assert refused(fn(FAKE, FAKE, 5, c, batch, L.hptr(shape), FAKE, None), "bad sizes")
        for fn in (lib.toda_pillar_scatter_fwd, lib.toda_pillar_scatter_bwd):
            assert refused(fn(FAKE, FAKE, 5, c, batch, R.PILLAR_NY, R.PILLAR_NX, FAKE, None), "bad sizes")
    assert refused(lib.toda_sparse_to_dense_fwd(FAKE, FAKE, -1, 4, 1, L.hptr(shape), FAKE, None), "bad sizes")


def test_fused_path_keeps_single_rows_and_unsupported_channels_away():
    """ops.bn_rows_supported is the gate in front of the kernels: one row (no batch statistics worth the name; n - 1 = 0) and channel
    counts outside the row reductions' plan take the module's own path."""
    from toda_amd import ops

    def on_gpu(n, c):
        """x as the predicate sees it, without a device: a meta tensor (shape, dtype, dim, stride) that reports is_cuda"""
        class Rows(torch.Tensor):
            is_cuda = True
        return torch.empty((n, c), dtype=torch.float32, device="meta").as_subclass(Rows)

    bn = lambda c: torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)    # noqa: E731
    assert ops.bn_rows_supported(on_gpu(2, 64), bn(64)) and ops.bn_rows_supported(on_gpu(2, 4), bn(4))
    assert not ops.bn_rows_supported(on_gpu(1, 64), bn(64)) and not ops.bn_rows_supported(on_gpu(0, 64), bn(64))
    for c in (12, 256):
        assert not ops.bn_rows_supported(on_gpu(100, c), bn(c))


# ------------------------------------------------------------------------------- the references' own helpers
def test_fold_order_reference_is_a_sum_in_the_documented_order():
    rng = np.random.default_rng(3)
    for blocks in (1, 2, 255, 256, 257, 513):
        p = rng.standard_normal((3, blocks)) * 1e3
        got, exact = R.fold_order(p), R.exact_sum(p)
        assert np.all(np.abs(got - exact) <= blocks * 2.0 ** -53 * np.abs(p).sum(-1))
    # thread 0 adds p[0] + p[256] = 2^-52 before the tree meets thread 1's 1.0; in index order both halves would be rounded away
    p = np.zeros(257)
    p[0], p[1], p[256] = 2.0 ** -53, 1.0, 2.0 ** -53
    assert (p[0] + p[1]) + p[256] == 1.0 and R.fold_order(p) == 1.0 + 2.0 ** -52


def test_scatter_cases_hold_the_corner_cells_and_consistent_features():
    for n in R.SCATTER_N:
        for batch in R.SCATTER_BATCH:
            for shape in (R.DENSE_SHAPE, [1, R.PILLAR_NY, R.PILLAR_NX]):
                idx, feat = R.scatter_case(n, 5, batch, shape, seed=n + batch)
                assert idx.shape == (n, 4) and feat.shape == (n, 5) and idx.dtype == np.int32
                if n == 0:
                    continue
                rows = {tuple(r) for r in idx.tolist()}
                assert (batch - 1, shape[0] - 1, shape[1] - 1, shape[2] - 1) in rows and (n == 1 or (0, 0, 0, 0) in rows)
                assert len(rows) == min(n, batch * int(np.prod(shape)))
                for r in rows:      # rows of one cell carry one feature row
                    assert len({feat[i].tobytes() for i in range(n) if tuple(idx[i]) == r}) == 1
                assert not np.array_equal(idx, idx[np.lexsort(idx.T[::-1])]) or n < 3
    g = np.random.default_rng(0).standard_normal((3, 5, R.PILLAR_NY, R.PILLAR_NX)).astype(np.float32)
    idx, _ = R.scatter_case(65, 5, 3, [1, R.PILLAR_NY, R.PILLAR_NX], seed=1)
    want = np.stack([g[b, :, y, x] for b, z, y, x in idx])
    assert np.array_equal(R.pillar_bwd(g, idx), want)
    assert ctypes.sizeof(ctypes.c_int32) * 4 == idx.strides[0]
