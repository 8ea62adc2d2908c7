"""The bandwidth kernels of csrc/dense.hip at their edges: row counts around the rows-per-iteration and rows-per-block boundaries
of the reductions, the capped grids, channel counts that do not divide a block of the elementwise passes, one and two threads per
row, the partial-sum fold at 1 .. 513 partials, the scatters around their 64-row x 32-channel tile.  The C ABI is called directly;
every output lies between NaN guard bands which must survive; the references are the float64 ones of tests/rows_cases.py.

Bounds.  Moments: a thread adds at most T = ceil(rows_per_block / (1024 / c)) float32 terms and everything above a thread is
float64, so sum x lies within T 2^-24 sum |x| of the float64 sum (and the squares likewise).  Affine pass, ReLU mask and shortcut
gradient: bit for bit, the operations are single float32 roundings in a fixed order.  dx / dgamma / dbeta: 1e-4 of the tensor's
scale, the tolerance of test_gpu_fullsize_backward.py.  Folds: the documented order, bit for bit.  Finalize: rtol 1e-6, a handful
of float32 roundings, on inputs whose shift and running mean do not cancel."""
import numpy as np
import pytest
import torch

from tests import rows_cases as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 64


def rel(a, b):
    """max |a - b| over the scale of b"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


class Guarded:
    """`numel` elements between two NaN guard bands of at least PAD elements (and two rows of a [n, c] tensor); .t is the contiguous view
    the kernel gets."""

    def __init__(self, shape, dtype=torch.float32, pad=PAD, fill=NAN):
        if len(shape) == 2:
            pad = max(pad, 2 * int(shape[1]))       # rows: the bands hold two whole rows
        self.numel, self.pad = int(np.prod(shape)), pad
        self.full = torch.full((self.numel + 2 * pad,), NAN, dtype=dtype, device="cuda")
        self.t = self.full[pad:pad + self.numel].view(*shape)
        if fill == fill:
            self.t.fill_(fill)

    @classmethod
    def of(cls, array, pad=PAD):
        """an input inside guard bands: a read past its end brings NaN into the result"""
        array = np.ascontiguousarray(array)
        g = cls(array.shape, dtype=torch.from_numpy(array[:0].reshape(-1)).dtype, pad=pad)
        g.t.copy_(torch.from_numpy(array))
        return g

    def intact(self):
        return bool(torch.isnan(self.full[:self.pad]).all()) and bool(torch.isnan(self.full[self.pad + self.numel:]).all())

    def np(self):
        return self.t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at flat index {i}: got {got.ravel()[i]!r} "
                             f"(0x{int(bits(got).ravel()[i]) & 0xFFFFFFFFFFFFFFFF:x}), want {want.ravel()[i]!r} "
                             f"(0x{int(bits(want).ravel()[i]) & 0xFFFFFFFFFFFFFFFF:x})")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def lib():
    from toda_amd import lib as L

    return L.load()


def P(t):
    from toda_amd import lib as L

    return L.ptr(t.t if isinstance(t, Guarded) else t)


def ok(rc, what):
    from toda_amd import lib as L

    L.check(rc, what)


def stream():
    from toda_amd import lib as L

    return L.stream()


# ================================================================================================ a. moments
def run_moments(lib, x, n, c):
    total = lib.toda_rows_reduce_doubles(n, c)
    assert total == R.reduce_doubles(n, c)
    sums = Guarded((total,), torch.float64)
    ok(lib.toda_rows_moments(P(x), n, c, P(sums), stream()), "rows_moments")
    return sums


def check_moments(lib, x_np, n, c):
    x = Guarded.of(x_np)
    sums = run_moments(lib, x, n, c)
    s = sums.np()
    blocks, rpb = R.reduce_plan(n)
    assert np.isfinite(s[:2 * c]).all()
    assert np.isfinite(s[2 * c:]).all(), "the per-block scratch [2c][blocks] is not fully written"
    assert sums.intact(), "written outside toda_rows_reduce_doubles(n, c) doubles"
    scratch = s[2 * c:].reshape(2 * c, blocks)
    assert_same_bits(s[:2 * c], R.fold_order(scratch), "result slots vs the fixed-order sum of their scratch rows")
    sx, sq, sabs, sx2 = R.moments(x_np)
    T = -(-rpb // (1024 // c))
    assert T == R.thread_terms(n, c) and T >= 1
    ex, eq = np.abs(s[:c] - sx), np.abs(s[c:2 * c] - sq)
    print(f"moments n={n} c={c} blocks={blocks} rpb={rpb} T={T}: err/bound sum {float((ex / (T * R.U24 * sabs)).max()):.3g} "
          f"squares {float((eq / (T * R.U24 * sx2)).max()):.3g}")
    assert (ex <= T * R.U24 * sabs).all(), float((ex / (T * R.U24 * sabs)).max())
    assert (eq <= T * R.U24 * sx2).all(), float((eq / (T * R.U24 * sx2)).max())
    again = run_moments(lib, x, n, c)
    assert torch.equal(again.t, sums.t) and again.intact()


def row_x(n, c, seed):
    return (np.random.default_rng(seed).standard_normal((n, c)) * 1.3 + 0.1).astype(np.float32)


@pytest.mark.parametrize("n,c", R.ROW_CASES + R.CAPPED)
def test_moments_at_the_stripe_and_block_edges(lib, n, c):
    check_moments(lib, row_x(n, c, 1000 * c + n), n, c)


def test_moments_of_an_offset_column_keep_the_one_pass_bound(lib):
    """x = 15 + 0.5 randn: sum x^2 is ~ 900 x the variance's share of it; the one-pass form is as well conditioned as its
    float32 partial sums allow, and that is the same bound"""
    x = (np.random.default_rng(7).standard_normal((513, 16)) * 0.5 + 15).astype(np.float32)
    check_moments(lib, x, 513, 16)


@pytest.mark.parametrize("c", [4, 128])
def test_moments_of_no_rows_are_zero(lib, c):
    sums = Guarded((R.reduce_doubles(0, c),), torch.float64)
    ok(lib.toda_rows_moments(None, 0, c, P(sums), stream()), "rows_moments")
    s = sums.np()
    assert (s[:2 * c] == 0).all() and np.isnan(s[2 * c:]).all() and sums.intact()


# ================================================================================================ b. affine + activation
def check_affine(lib, n, c, seed):
    rng = np.random.default_rng(seed)
    x_np = (rng.standard_normal((n, c)) * 1.3 + 0.1).astype(np.float32)
    res_np = rng.standard_normal((n, c)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    shift = rng.standard_normal(c).astype(np.float32)
    x, res, sc, sh = Guarded.of(x_np), Guarded.of(res_np), Guarded.of(scale), Guarded.of(shift)
    for residual in (False, True):
        for relu in (0, 1):
            y = Guarded((n, c))
            ok(lib.toda_rows_affine_act(P(x), P(sc), P(sh), P(res) if residual else None, n, c, relu, P(y), stream()), "rows_affine_act")
            assert y.intact(), "written outside y"
            want = R.affine_act(x_np, scale, shift, res_np if residual else None, relu)
            assert_same_bits(y.np(), want, f"affine n={n} c={c} relu={relu} residual={residual} (ew grid {R.ew_blocks(n, c)})")


@pytest.mark.parametrize("n,c", R.AFFINE_CASES + [nc for nc in R.CAPPED if nc not in R.AFFINE_CASES])
def test_affine_act_is_the_float32_expression_bit_for_bit(lib, n, c):
    check_affine(lib, n, c, 77 * c + n)


def test_affine_act_of_no_rows_writes_nothing(lib):
    y = Guarded((4, 12))
    ok(lib.toda_rows_affine_act(None, None, None, None, 0, 12, 1, P(y), stream()), "rows_affine_act")
    assert bool(torch.isnan(y.full).all())


# ================================================================================================ c. BatchNorm backward
class Uploaded:
    def __init__(self, case):
        self.case = case
        self.x, self.dy, self.stats, self.gamma = Guarded.of(case.x), Guarded.of(case.dy), Guarded.of(case.stats), Guarded.of(case.gamma)
        self.res = Guarded.of(case.res) if case.res is not None else None


def call_bn_bwd(lib, up, relu, dres_mode, colsum):
    """One call of the entry point that serves (shortcut, dres_mode): -> (sums, dx, dres, cs, ws), all guarded."""
    case = up.case
    n, c = case.n, case.c
    sums = Guarded((lib.toda_rows_reduce_doubles(n, c),), torch.float64)
    dx = Guarded((n, c))
    dres = Guarded((n, c)) if dres_mode == "out" else None
    cs = ws = None
    res_p, dres_p = (P(up.res) if up.res is not None else None), (P(dres) if dres is not None else None)
    if colsum:
        assert lib.toda_rows_bn_bwd_colsum_doubles(n, c) == R.colsum_doubles(n, c)
        ws = Guarded((R.colsum_doubles(n, c),), torch.float64)
        cs = Guarded((c,))
        rc = lib.toda_rows_bn_bwd_res_colsum(P(up.dy), P(up.x), res_p, P(up.stats), P(up.gamma), n, c, relu, P(sums), P(dx), dres_p,
                                             P(ws), P(cs), stream())
    elif up.res is None:
        rc = lib.toda_rows_bn_bwd(P(up.dy), P(up.x), P(up.stats), P(up.gamma), n, c, relu, P(sums), P(dx), stream())
    else:
        rc = lib.toda_rows_bn_bwd_res(P(up.dy), P(up.x), res_p, P(up.stats), P(up.gamma), n, c, relu, P(sums), P(dx), dres_p, stream())
    ok(rc, "rows_bn_bwd")
    for g, what in ((sums, "sums"), (dx, "dx"), (dres, "dres"), (cs, "dx_colsum"), (ws, "colsum workspace")):
        assert g is None or g.intact(), f"written outside {what}"
    return sums, dx, dres, cs, ws


def check_bn_bwd(lib, case, shifted, every_element):
    """All of (c) for one set of tensors: relu x dres modes, the three entry points, forward / backward mask agreement."""
    n, c = case.n, case.c
    up = Uploaded(case)
    pre32, pre64 = case.pre32(), case.pre64()
    mask32 = pre32 > 0
    # the forward pass on the same tensors: its output is positive exactly where the backward's mask is set
    y = Guarded((n, c))
    ok(lib.toda_rows_affine_act(P(up.x), P(up.stats.t[2]), P(up.stats.t[3]), P(up.res) if up.res is not None else None, n, c, 1, P(y),
                                stream()), "rows_affine_act")
    y_np = y.np()
    assert y.intact()
    assert_same_bits(y_np, np.where(mask32, pre32, np.float32(0)), "forward output")
    assert np.array_equal(y_np > 0, mask32)
    if every_element:
        assert np.abs(pre64).min() > 1e-4 or (pre64 == 0).any()     # rows_cases' seeds (or the exact zeros of the zero case)
        keep = np.ones((n, c), bool)
    else:
        keep = np.abs(pre64) > 2e-5
        assert keep.mean() >= 0.9999
    assert np.array_equal(mask32[keep], (pre64 > 0)[keep])
    for relu in (0, 1):
        # the float64 mask; where entries were left out above, the float32 one (equal on every kept entry): a left-out entry still
        # counts in the column sums, on the side of zero the float32 pre-activation falls
        dz, dbeta, dgamma, dx_ref = R.bn_bwd(case.dy, case.x, case.res, case.stats, case.gamma, relu, mask=None if every_element else mask32)
        sel = keep if relu else np.ones((n, c), bool)
        dres_want = np.where(mask32, case.dy, np.float32(0)) if relu else case.dy      # a masked entry is +0
        for dres_mode in (("out", "null") if case.res is not None else ("none",)):
            what = f"n={n} c={c} relu={relu} shortcut={case.res is not None} dres={dres_mode} shifted={shifted}"
            sums, dx, dres, _, _ = call_bn_bwd(lib, up, relu, dres_mode, colsum=False)
            s, dx_np = sums.np(), dx.np()
            assert np.isfinite(s[:2 * c]).all() and np.isfinite(dx_np).all(), what
            if dres is not None:
                assert_same_bits(dres.np(), dres_want, "dres " + what)
            f32 = s[2 * c:3 * c].view(np.float32)
            assert_same_bits(f32, s[:2 * c].astype(np.float32), "float32 copies of the sums " + what)
            errs = (rel(dx_np[sel], dx_ref[sel]), rel(s[:c], dbeta), rel(s[c:2 * c], dgamma), rel(f32[:c], dbeta), rel(f32[c:], dgamma))
            print("bn_bwd", what, "rel dx / dbeta / dgamma / their float32 copies:", " ".join(f"{e:.2e}" for e in errs))
            assert max(errs) < 1e-4, (what, errs)
            # the column-sum variant: the same bits, plus the sums of its own dx over the rows
            sums1, dx1, dres1, cs, _ = call_bn_bwd(lib, up, relu, dres_mode, colsum=True)
            assert torch.equal(dx1.t, dx.t) and torch.equal(sums1.t[:3 * c], sums.t[:3 * c]), what
            assert dres is None or torch.equal(dres1.t, dres.t), what
            want = dx1.t.double().sum(0).cpu().numpy()
            noise = dx1.t.double().abs().sum(0).cpu().numpy() * 2e-7 + 1e-30
            got = cs.np().astype(np.float64)
            assert (np.abs(got - want) <= noise).all(), (what, float((np.abs(got - want) / noise).max()))
            if shifted and n > 100:
                assert float(np.abs(want).min()) > 1e2 * float(noise.max()), what      # channel sums far from zero
        # a second call gives the same bits everywhere
        sums2, dx2, dres2, cs2, _ = call_bn_bwd(lib, up, relu, dres_mode, colsum=True)
        assert torch.equal(dx2.t, dx1.t) and torch.equal(sums2.t[:3 * c], sums1.t[:3 * c]) and torch.equal(cs2.t, cs.t)
        assert dres1 is None or torch.equal(dres2.t, dres1.t)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("n,c", R.ROW_CASES + R.CAPPED)
def test_bn_backward_entry_points_at_the_edges(lib, n, c, residual):
    for shifted in (False, True):
        check_bn_bwd(lib, R.Case(n, c, residual, shifted), shifted, every_element=n * c <= R.SMALL)


@pytest.mark.parametrize("residual", [False, True])
def test_relu_mask_is_closed_at_exactly_zero_in_every_pass(lib, residual):
    """Pre-activations that are exactly 0.0 (x == +-0 under a zero shift, the shortcut 0 there): the forward gives 0, and both
    backward passes must leave these entries out - `pre > 0`, not `>=`, in the reduction and in the apply pass alike."""
    n, c = 257, 16
    case = R.Case(n, c, residual, True)
    case.stats[3, ::2] = 0.0
    case.x[::3, ::2] = 0.0
    case.x[1::6, ::4] = -0.0
    if residual:
        case.res[::3, ::2] = 0.0
        case.res[1::6, ::4] = 0.0
    pre = case.pre32()
    assert (pre == 0).sum() >= n * c // 8 and np.array_equal(pre == 0, case.pre64() == 0)
    assert np.abs(case.pre64()[pre != 0]).min() > 1e-5
    assert np.abs(case.dy[pre == 0]).min() > 0
    check_bn_bwd(lib, case, False, every_element=True)


@pytest.mark.parametrize("c", [4, 128])
def test_bn_backward_of_no_rows_zeroes_its_results_and_touches_nothing(lib, c):
    sums = Guarded((R.reduce_doubles(0, c),), torch.float64)
    cs, ws = Guarded((c,)), Guarded((1,), torch.float64)
    rc = lib.toda_rows_bn_bwd_res_colsum(None, None, None, None, None, 0, c, 1, P(sums), None, None, P(ws), P(cs), stream())
    ok(rc, "rows_bn_bwd")
    s = sums.np()
    assert (s[:3 * c] == 0).all() and np.isnan(s[3 * c:]).all() and sums.intact()
    assert (cs.np() == 0).all() and cs.intact() and bool(torch.isnan(ws.full).all())


# ================================================================================================ d. finalize
def finalize_inputs(c, n, seed):
    """Synthetic totals with |mean| in [0.1, 2], var in [0.01, 3] and, for every third channel, E[x^2] - mean^2 a little below
    zero (the clamp); beta and the running mean carry signs that keep shift and the running update free of cancellation."""
    rng = np.random.default_rng(seed)
    sign = rng.choice([-1.0, 1.0], c)
    s0 = n * sign * rng.uniform(0.1, 2.0, c)
    m = s0 / n
    s1 = n * (m * m + rng.uniform(0.01, 3.0, c))
    s1[::3] = n * (m[::3] * m[::3]) * (1 - 1e-13)
    gamma = rng.uniform(0.5, 1.5, c).astype(np.float32)
    beta = (-sign * rng.uniform(0.05, 0.5, c)).astype(np.float32)
    rm = (sign * rng.uniform(0.05, 0.3, c)).astype(np.float32)
    rv = rng.uniform(0.5, 2.0, c).astype(np.float32)
    return np.concatenate([s0, s1]), gamma, beta, rm, rv


def run_finalize(lib, sums_t, n, c, gamma, beta, rm, rv, training, partial_blocks=None):
    """-> ([mean, invstd, scale, shift] as numpy, rm', rv'), every buffer guarded and checked"""
    outs = [Guarded((c,)) for _ in range(4)]
    g, b = (Guarded.of(gamma) if gamma is not None else None), (Guarded.of(beta) if beta is not None else None)
    rmg, rvg = (Guarded.of(rm) if rm is not None else None), (Guarded.of(rv) if rv is not None else None)
    ptr = lambda t: None if t is None else P(t)      # noqa: E731
    if partial_blocks is None:
        rc = lib.toda_bn_finalize(P(sums_t), n, c, ptr(g), ptr(b), ptr(rmg), ptr(rvg), R.MOMENTUM, R.EPS, training, *[P(o) for o in outs], stream())
    else:
        rc = lib.toda_bn_finalize_partials(P(sums_t), partial_blocks, n, c, ptr(g), ptr(b), ptr(rmg), ptr(rvg), R.MOMENTUM, R.EPS,
                                           *[P(o) for o in outs], stream())
    ok(rc, "bn_finalize")
    for t in outs + [g, b, rmg, rvg]:
        assert t is None or t.intact()
    assert g is None or (np.array_equal(g.np(), gamma) and np.array_equal(b.np(), beta))
    return [o.np() for o in outs], (rmg.np() if rmg is not None else None), (rvg.np() if rvg is not None else None)


def assert_finalize_close(outs, rm1, rv1, sums, n, gamma, beta, rm, rv, training):
    want = R.finalize(sums, n, gamma, beta, rm, rv, R.MOMENTUM, R.EPS, training)
    for got, ref, name in zip(outs, want[:4], ("mean", "invstd", "scale", "shift")):
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0, err_msg=name)
    if rm is not None:
        np.testing.assert_allclose(rm1, want[4], rtol=1e-6, atol=0, err_msg="running_mean")
        np.testing.assert_allclose(rv1, want[5], rtol=1e-6, atol=0, err_msg="running_var")


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("n", [1, 2, 20011])
@pytest.mark.parametrize("c", [1, 3, 64, 255, 256])
def test_bn_finalize_matches_batchnorm_bookkeeping(lib, c, n, training):
    sums, gamma, beta, rm, rv = finalize_inputs(c, n, 31 * c + n)
    mean = sums[:c] / n
    assert ((sums[c:] / n - mean * mean) < 0).any()                       # the clamp runs
    sums_t = Guarded.of(sums)
    for affine in (True, False):
        for running in ((True, False) if training else (True,)):
            ga, be = (gamma, beta) if affine else (None, None)
            r0, v0 = (rm, rv) if running else (None, None)
            outs, rm1, rv1 = run_finalize(lib, sums_t, n, c, ga, be, r0, v0, training)
            assert sums_t.intact() and np.array_equal(sums_t.np(), sums)
            assert_finalize_close(outs, rm1, rv1, sums, n, ga, be, r0, v0, training)
            if not training:
                assert np.array_equal(rm1, rm) and np.array_equal(rv1, rv) and np.array_equal(outs[0], rm)


@pytest.mark.parametrize("blocks", [1, 2, 255, 256, 257, 513])
@pytest.mark.parametrize("c", [1, 3, 64, 255, 256])
def test_bn_finalize_partials_is_the_fold_followed_by_finalize(lib, c, blocks):
    rng = np.random.default_rng(1000 * c + blocks)
    for n in (1, 2, 20011):
        totals, gamma, beta, rm, rv = finalize_inputs(c, n, 17 * c + blocks + n)
        w = rng.uniform(0.5, 1.5, (2 * c, blocks))
        part = totals[:, None] * w / w.sum(1, keepdims=True)              # random partials behind NaN result slots
        buf = np.concatenate([np.full(2 * c, NAN), part.ravel()])
        for affine, running in ((True, True), (False, False), (True, False), (False, True)):
            ga, be = (gamma, beta) if affine else (None, None)
            r0, v0 = (rm, rv) if running else (None, None)
            sums_t = Guarded.of(buf)
            outs, rm1, rv1 = run_finalize(lib, sums_t, n, c, ga, be, r0, v0, 1, partial_blocks=blocks)
            s = sums_t.np()
            assert sums_t.intact()
            assert_same_bits(s[2 * c:], part.ravel(), "the partials are read, not written")
            assert_same_bits(s[:2 * c], R.fold_order(part), f"folded totals c={c} blocks={blocks}")
            assert (np.abs(s[:2 * c] - R.exact_sum(part)) <= blocks * 2.0 ** -53 * np.abs(part).sum(1)).all()
            # == toda_bn_finalize on the folded totals, bit for bit
            folded = Guarded.of(s[:2 * c].copy())
            outs0, rm0, rv0 = run_finalize(lib, folded, n, c, ga, be, r0, v0, 1)
            for a, b, name in zip(outs, outs0, ("mean", "invstd", "scale", "shift")):
                assert_same_bits(a, b, name)
            if running:
                assert_same_bits(rm1, rm0, "running_mean")
                assert_same_bits(rv1, rv0, "running_var")
            assert_finalize_close(outs, rm1, rv1, s[:2 * c], n, ga, be, r0, v0, 1)


# ================================================================================================ e. ops.bn_rows at small n
def small_bn_case(n, c, train, shortcut):
    """The first seed from 500 c + n upwards on which no float64 pre-activation lies within 1e-4 of zero."""
    for seed in range(500 * c + n, 500 * c + n + 4000):
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal((n, c)) * 1.3 + 0.1).astype(np.float32)
        r = (rng.standard_normal((n, c)) * 0.8).astype(np.float32) if shortcut else None
        g = rng.standard_normal((n, c)).astype(np.float32)
        ref = torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01).double()
        with torch.no_grad():
            ref.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, c)))
            ref.bias.copy_(torch.from_numpy(rng.uniform(-0.5, 0.5, c)))
            ref.running_mean.copy_(torch.from_numpy(rng.uniform(-0.2, 0.2, c)))
            ref.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, c)))
        state = {k: v.clone() for k, v in ref.state_dict().items()}
        ref.train(train)
        xr = torch.from_numpy(x).double().requires_grad_(True)
        rr = torch.from_numpy(r).double().requires_grad_(True) if shortcut else None
        pre = ref(xr) + rr if shortcut else ref(xr)
        if float(pre.detach().abs().min()) > 1e-4:
            torch.relu(pre).backward(torch.from_numpy(g).double())
            return x, r, g, ref, state, xr, rr, pre.detach()
    raise AssertionError("no seed found")


@pytest.mark.parametrize("shortcut", [False, True])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("n,c", [(n, c) for n in (2, 3, 65, 257) for c in (4, 8, 128)])
def test_ops_bn_rows_at_small_row_counts_matches_batchnorm1d(n, c, train, shortcut):
    """Every element, the tolerances of test_gpu_parity.py's two BatchNorm1d tests."""
    from toda_amd import ops

    x, r, g, ref, state, xr, rr, pre = small_bn_case(n, c, train, shortcut)
    assert float(pre.abs().min()) > 1e-4
    mine = torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)
    mine.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in state.items()})
    mine = mine.cuda().train(train)
    xm = dev(x).requires_grad_(True)
    rm = dev(r).requires_grad_(True) if shortcut else None
    assert ops.bn_rows_supported(xm, mine)
    colsum = train and (n, c) == (65, 8)
    ym = ops.bn_rows(xm, mine, True, residual=rm, colsum=colsum)
    ym.backward(dev(g))
    if colsum and ops.BN_BWD_COLSUM:
        (gx, cs, _), = ops._DX_COLSUM.values()
        want, noise = gx.double().sum(0), gx.double().abs().sum(0) * 2e-7 + 1e-30
        assert bool(((cs.double() - want).abs() <= noise).all())
        ops._DX_COLSUM.clear()
    yr = torch.relu(pre).numpy()
    t = dict(y=(1e-4, 2e-5), dx=(2e-3, 2e-4), wb=(1e-3, 2e-2)) if shortcut else dict(y=(1e-4, 1e-5), dx=(1e-3, 1e-5), wb=(1e-4, 1e-3))
    np.testing.assert_allclose(ym.detach().cpu().numpy(), yr, rtol=t["y"][0], atol=t["y"][1])
    np.testing.assert_allclose(xm.grad.cpu().numpy(), xr.grad.numpy(), rtol=t["dx"][0], atol=t["dx"][1])
    np.testing.assert_allclose(mine.weight.grad.cpu().numpy(), ref.weight.grad.numpy(), rtol=t["wb"][0], atol=t["wb"][1])
    np.testing.assert_allclose(mine.bias.grad.cpu().numpy(), ref.bias.grad.numpy(), rtol=t["wb"][0], atol=t["wb"][1])
    if shortcut:
        np.testing.assert_allclose(rm.grad.cpu().numpy(), rr.grad.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(mine.running_mean.cpu().numpy(), ref.running_mean.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(mine.running_var.cpu().numpy(), ref.running_var.numpy(), rtol=1e-5, atol=1e-6)
    assert int(mine.num_batches_tracked) == int(ref.num_batches_tracked) == (1 if train else 0)


# ================================================================================================ f. scatters
def scatter_calls(lib, pillar, n, c, batch):
    from toda_amd import lib as L

    if pillar:
        shape = [1, R.PILLAR_NY, R.PILLAR_NX]
        geom = (R.PILLAR_NY, R.PILLAR_NX)
        return shape, (lambda f, i, d: lib.toda_pillar_scatter_fwd(f, i, n, c, batch, *geom, d, stream())), \
            (lambda g, i, f: lib.toda_pillar_scatter_bwd(g, i, n, c, batch, *geom, f, stream()))
    shape = R.DENSE_SHAPE
    sh = L.host_i32(shape)
    return shape, (lambda f, i, d: lib.toda_sparse_to_dense_fwd(f, i, n, c, batch, L.hptr(sh), d, stream())), \
        (lambda g, i, f: lib.toda_sparse_to_dense_bwd(g, i, n, c, batch, L.hptr(sh), f, stream()))


@pytest.mark.parametrize("c", R.SCATTER_C)
@pytest.mark.parametrize("n", R.SCATTER_N)
def test_scatters_around_the_row_and_channel_tile(lib, n, c):
    for pillar in (False, True):
        for batch in R.SCATTER_BATCH:
            what = f"{'pillar' if pillar else 'dense'} n={n} c={c} batch={batch}"
            shape, fwd, bwd = scatter_calls(lib, pillar, n, c, batch)
            idx_np, feat_np = R.scatter_case(n, c, batch, shape, seed=100 * n + c + batch)
            idx = torch.from_numpy(idx_np).cuda()
            feat = Guarded.of(feat_np)
            dense = Guarded((batch, c, *shape))
            ok(fwd(P(feat), P(idx), P(dense)), "scatter forward " + what)
            want = R.pillar_fwd(feat_np, idx_np, batch, shape[1], shape[2]).reshape(batch, c, *shape) if pillar else \
                R.dense_fwd(feat_np, idx_np, batch, shape)
            assert dense.intact(), "forward wrote outside the dense tensor: " + what
            assert_same_bits(dense.np(), want, "forward " + what)
            assert np.count_nonzero(dense.np()) == np.count_nonzero(want) <= n * c
            # backward: a random dense gradient, NaN guard rows behind row n of the feature gradient
            g_np = np.random.default_rng(n + c).standard_normal((batch, c, *shape)).astype(np.float32)
            gdense = Guarded.of(g_np)
            gfeat = Guarded((n, c))
            ok(bwd(P(gdense), P(idx), P(gfeat)), "scatter backward " + what)
            gather = R.pillar_bwd(g_np[:, :, 0], idx_np) if pillar else R.dense_bwd(g_np, idx_np, shape)
            assert gfeat.intact(), "backward wrote outside rows [0, n): " + what
            assert_same_bits(gfeat.np(), np.ascontiguousarray(gather, np.float32).reshape(n, c), "backward " + what)
            assert_same_bits(gdense.np(), g_np, "the dense gradient is read only")


@pytest.mark.parametrize("pillar", [False, True])
def test_scatters_take_a_non_contiguous_feature_view(pillar):
    """ops.sparse_to_dense / ops.pillar_scatter on every other column of a wider tensor: the .contiguous() in front of the kernel,
    and a random gradient back through the view."""
    from toda_amd import ops

    n, c, batch = 65, 33, 3
    shape = [1, R.PILLAR_NY, R.PILLAR_NX] if pillar else R.DENSE_SHAPE
    idx_np, _ = R.scatter_case(n, c, batch, shape, seed=9)
    wide_np = np.random.default_rng(10).standard_normal((n, 2 * c)).astype(np.float32)
    for r in range(n):                       # rows of one cell carry one feature row
        wide_np[r] = wide_np[np.flatnonzero((idx_np == idx_np[r]).all(1))[0]]
    wide = dev(wide_np).requires_grad_(True)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    feat_np = wide_np[:, ::2]
    g_np = np.random.default_rng(11).standard_normal((batch, c, *(shape[1:] if pillar else shape))).astype(np.float32)
    if pillar:
        out = ops.pillar_scatter(view, dev(idx_np), batch, R.PILLAR_NY, R.PILLAR_NX)
        want, gather = R.pillar_fwd(feat_np, idx_np, batch, R.PILLAR_NY, R.PILLAR_NX), R.pillar_bwd(g_np, idx_np)
    else:
        out = ops.sparse_to_dense(view, dev(idx_np), batch, shape)
        want, gather = R.dense_fwd(feat_np, idx_np, batch, shape), R.dense_bwd(g_np, idx_np, shape)
    assert_same_bits(out.detach().cpu().numpy(), want, "forward through the view")
    out.backward(dev(g_np))
    grad = wide.grad.cpu().numpy()
    assert_same_bits(np.ascontiguousarray(grad[:, ::2]), np.ascontiguousarray(gather, np.float32), "gradient through the view")
    assert (grad[:, 1::2] == 0).all()
