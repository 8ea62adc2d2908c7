"""The single-pass BatchNorm2d kernels of csrc/bn2d.hip without a GPU: the routing restatement of tests/bn2d_cases.py against the
library's own host query, the set of kernel instantiations the launchers can reach and that the case lists reach every one of them,
the float64 references against torch's float64 autograd, the bound formulas against a float32 restatement of the kernels' arithmetic,
the threshold-channel builder, and the argument checks that return TODA_EINVAL before anything is launched."""
import numpy as np
import pytest
import torch

from tests import bn2d_cases as B
from toda_amd import lib as L

FAKE = 4096        # a non-null "device pointer" for arguments a refused call must not touch


# ------------------------------------------------------------------------------- routing
def test_restatement_equals_the_library_query():
    lib = L.load()
    for c in (0, 1, 4096, 4097):
        for batch in range(6):
            got = [lib.toda_bn2d_supported(batch, c, hw) for hw in range(1, 36871)]
            want = [B.supported(batch, c, hw) for hw in range(1, 36871)]
            assert got == want, (c, batch, next(hw + 1 for hw in range(36870) if got[hw] != want[hw]))
    assert lib.toda_bn2d_supported(2, 1, 0) == 0 == B.supported(2, 1, 0)
    assert lib.toda_bn2d_sync_bytes() == B.MAX_SYNC_C * 4 * (16 + 4)


@pytest.fixture(scope="module")
def all_instantiations():
    return B.reachable(range(1, 36865))


def covered_by_the_case_lists():
    """instantiation -> the first case that launches it"""
    seen = {}
    cases = [(batch, B.SWEEP_C, hw) for hw, batch in B.SWEEP] + B.MAPPING_CASES
    for batch, c, hw in cases:
        for sync in (True, False):
            r = B.routes(batch, c, hw, sync)
            for d in ("fwd", "bwd"):
                if r[d] is not None:
                    seen.setdefault(B.instantiation(d, batch, r[d]), (batch, c, hw, "sync" if sync else "NULL"))
    return seen


def test_launchers_reach_66_instantiations_and_the_case_list_reaches_each(all_instantiations):
    count = lambda d, fam: sum(1 for i in all_instantiations if i[0] == d and i[1] == fam)      # noqa: E731
    assert (count("fwd", "channel"), count("bwd", "channel"), count("fwd", "split"), count("bwd", "split")) == (27, 27, 3, 9)
    assert len(all_instantiations) == 66
    seen = covered_by_the_case_lists()
    assert set(seen) == all_instantiations, sorted(all_instantiations - set(seen))
    for inst in sorted(seen):
        print(inst, "<-", seen[inst])
    # every (V, K) of the ladder, and K = 8 with whole k-slices past the end of the plane
    assert {(i[2], i[4]) for i in all_instantiations} == {(v, k) for v in (4, 1) for k in B.K_OF_V[v]}
    assert B.need_of(16388) == 5 and B.pick_k(16388 // 4, 4) == 8


def test_expected_routes_of_the_issue_table():
    def r(batch, hw, sync=True, c=3, d="bwd"):
        return B.routes(batch, c, hw, sync)[d]

    for hw, v, k in ((4100, 4, 2), (8196, 4, 3), (12292, 4, 4), (16384, 4, 4), (16388, 4, 8), (4097, 1, 9), (9215, 1, 9), (9217, 1, 18),
                     (18431, 1, 18), (18433, 1, 36), (36863, 1, 36), (32772, 4, 9), (36860, 4, 9), (36864, 4, 9)):
        assert r(1, hw)[1:3] == (v, k) and r(1, hw, d="fwd")[1:3] == (v, k), hw
    assert r(4, 8196) == ("split", 4, 3, 12) and r(4, 8196, sync=False) == ("channel", 4, 3, 48)
    for hw in (12292, 16384):
        assert r(4, hw) == ("split", 4, 4, 16) and r(4, hw, d="fwd") == ("channel", 4, 4, 64) and r(2, hw)[0] == "channel"
    assert r(2, 16388) == ("split", 4, 8, 32) and r(2, 16388, d="fwd") == ("channel", 4, 8, 64)
    assert r(4, 16388) == r(4, 16388, d="fwd") == ("split", 4, 8, 32)
    assert r(4, 16388, sync=False) is None and r(4, 16388, sync=False, d="fwd") is None
    for hw in (9217, 18431):
        assert r(4, hw) == ("split", 1, 18, 18) and r(4, hw, d="fwd") == ("channel", 1, 18, 72) and r(2, hw)[0] == "channel"
    assert r(4, 9215) == ("channel", 1, 9, 36)                           # 36 floats: not above the threshold
    for hw, v in ((18433, 1), (36863, 1), (32772, 4), (36860, 4), (36864, 4)):
        k = 36 // v
        assert r(2, hw) == ("split", v, k, 36) and r(2, hw, d="fwd") == ("channel", v, k, 72)
        assert r(4, hw) == r(4, hw, d="fwd") == ("split", v, k, 36)
        assert r(4, hw, sync=False) is None and r(2, hw, sync=False) == ("channel", v, k, 72)
    # TODA_BN2D_SPLIT=0: the per-channel backward wherever it exists
    for batch, c, hw in B.ENV_SPLIT_SHAPES:
        assert B.routes(batch, c, hw, True)["bwd"][0] == "split"
        assert B.routes(batch, c, hw, True, env_split=0)["bwd"] == B.routes(batch, c, hw, False)["bwd"] != None      # noqa: E711
    assert B.routes(4, 3, 16388, True, env_split=0)["bwd"][0] == "split"    # no per-channel kernel: the switch does not apply


def test_probe_shapes_take_the_routes_their_descriptions_name():
    fam = lambda batch, hw, d, c=3: B.routes(batch, c, hw, True)[d][0]      # noqa: E731
    # neighbours: whole k-slices past the end of the plane
    for hw in B.NEIGHBOUR_HW:
        v = B.vec_of(hw)
        assert B.pick_k(hw // v, v) > B.need_of(hw), hw
    assert [B.routes(1, 3, hw, True)["fwd"][1:3] for hw in B.NEIGHBOUR_HW] == [(4, 8), (1, 9), (1, 18), (1, 36), (1, 4)]
    # slices
    got = [(fam(b, hw, "fwd"), fam(b, hw, "bwd")) for b, hw in B.SLICE_SHAPES]
    assert got == [("channel", "channel"), ("channel", "channel"), ("channel", "split"), ("split", "split"), ("channel", "split")]
    assert B.vec_of(36863) == 1 and 36863 % 4 == 3
    # threshold channels
    assert [fam(b, hw, "bwd", c=B.THRESHOLD_CHANNELS) for b, hw in B.THRESHOLD_SHAPES] == ["channel"] * 3 + ["split"] * 2
    # spikes: the positions are inside the plane and include its first and last vector and the last k-slice's first
    for hw, batch in B.SPIKE_SHAPES:
        pos = B.spike_positions(hw)
        v = B.vec_of(hw)
        assert {0, hw - 1, hw - v, (B.need_of(hw) - 1) * v * 1024} <= set(pos) and max(pos) < hw
        assert B.routes(batch, 2, hw, True)["fwd"] is not None
    # degenerate / reuse / split-only
    for batch, hw in B.SPLIT_ONLY:
        assert B.floats_per_thread(batch, hw) == 0 and B.split_ok(batch, 3, hw) and not B.split_ok(batch, 4097, hw)
    for c, p in B.REUSE_SEQUENCE:
        assert fam(p, B.REUSE_HW, "bwd", c=c) == "split"
    assert len(set(B.REUSE_EPOCHS)) == len(B.REUSE_EPOCHS) == len(B.REUSE_SEQUENCE) and 0 not in B.REUSE_EPOCHS
    # the mapping cases run split kernels on both workgroup -> plane mappings
    assert all(fam(b, hw, "bwd", c=c) == "split" for b, c, hw in B.MAPPING_CASES) and {c & 7 for _, c, _ in B.MAPPING_CASES} == {0, 1}
    assert B.MISALIGNED and all(B.vec_of(hw) == 1 for hw, _ in B.MISALIGNED)


# ------------------------------------------------------------------------------- references against torch float64
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("batch,hw", [(1, 5), (2, 37), (4, 100)])
def test_references_match_torch_float64_autograd(batch, hw, relu):
    case = B.Case(batch, 3, hw)
    bn = torch.nn.BatchNorm2d(3, eps=B.EPS, momentum=B.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(case.gamma.astype(np.float64)))
        bn.bias.copy_(torch.from_numpy(case.beta.astype(np.float64)))
        bn.running_mean.copy_(torch.from_numpy(case.rm.astype(np.float64)))
        bn.running_var.copy_(torch.from_numpy(case.rv.astype(np.float64)))
    x = torch.from_numpy(case.x.astype(np.float64)).reshape(batch, 3, hw, 1).requires_grad_(True)
    pre = bn(x)
    y = torch.relu(pre) if relu else pre
    y.backward(torch.from_numpy(case.dy.astype(np.float64)).reshape(batch, 3, hw, 1))
    l1 = B.layer1(case.x, 4, case.rm, case.rv)
    save64 = np.stack([l1["mean"][0], l1["invstd"][0]])
    close = lambda a, b: np.testing.assert_allclose(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1), rtol=1e-11, atol=1e-11)   # noqa: E731
    close(l1["running_mean"][0], bn.running_mean.numpy())
    close(l1["running_var"][0], bn.running_var.numpy())
    z, y_ref, _ = B.layer2(case.x, case.gamma, case.beta, save64, relu)
    close(y_ref, y.detach().numpy())
    l3 = B.layer3(case.x, case.dy, case.gamma, save64, (z > 0) if relu else None, 4)
    close(l3["dx"][0], x.grad.numpy())
    close(l3["dbeta"][0], bn.bias.grad.numpy())
    close(l3["dgamma"][0], bn.weight.grad.numpy())


# ------------------------------------------------------------------------------- bounds against a float32 restatement
def restated(case, batch, hw, sync, relu):
    """The kernels' arithmetic in numpy float32 on every channel of a case, through the layer 1 - 3 bounds: worst err / bound."""
    r = B.routes(batch, case.c, hw, sync)
    worst = {}

    def note(name, value):
        worst[name] = max(worst.get(name, 0.0), value)

    save = np.zeros((2, case.c), np.float32)
    y = np.zeros_like(case.x)
    for ch in range(case.c):
        save[0, ch], save[1, ch], y[:, ch] = B.emulate_forward(case.x[:, ch], case.gamma[ch], case.beta[ch], r["fwd"], relu)
    for name, (ref, bound) in B.layer1(case.x, r["fwd"][3]).items():
        note(name, B.ratio(save[0] if name == "mean" else save[1], ref, bound))
    _, y_ref, bound = B.layer2(case.x, case.gamma, case.beta, save, relu)
    note("y", B.ratio(y, y_ref, bound))
    dx, dgamma, dbeta = np.zeros_like(case.x), np.zeros(case.c, np.float32), np.zeros(case.c, np.float32)
    for ch in range(case.c):
        dgamma[ch], dbeta[ch], dx[:, ch] = B.emulate_backward(case.x[:, ch], case.dy[:, ch], case.gamma[ch], case.beta[ch], save[0, ch],
                                                              save[1, ch], r["bwd"], relu)
    l3 = B.layer3(case.x, case.dy, case.gamma, save, (y > 0) if relu else None, r["bwd"][3])
    for name, got in (("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
        note(name, B.ratio(got, *l3[name]))
    return worst


@pytest.mark.parametrize("batch,hw,sync", [(1, 4100, False), (2, 36864, True), (4, 9217, True), (2, 4097, False), (4, 16384, True),
                                           (2, 5, False), (4, 16388, True)])
def test_bounds_leave_room_for_a_correct_kernel(batch, hw, sync):
    case = B.Case(batch, 3, hw)
    for relu in (0, 1):
        worst = restated(case, batch, hw, sync, relu)
        print(batch, hw, relu, {k: round(v, 3) for k, v in worst.items()})
        assert max(worst.values()) < 1.0, worst


def test_bounds_hold_for_a_far_offset_narrow_channel():
    """mean 1e4, sigma 0.01 at 1 x 36863 (V = 1, K = 36), a million standard deviations from zero, outside what the GPU cases hold
    (|mean| / sigma = 1000 there).  The kernels centre on their own mean, whose error delta (the layer 1 mean bound: float32 partial
    sums of values near 1e4) enters the variance as + delta^2.  The invstd bound of layer 1 leaves that term out - at
    |mean| / sigma = 1000 it is below 1e-10 of the variance - so here it is added: relative delta^2 / (2 (var + eps)).  On this seed the
    restatement sits at 1.04 of the plain bound; every other layer holds as it stands."""
    case = B.Case(1, 1, 36863, kinds="w")
    case.x[:] = (1e4 + 0.01 * np.random.default_rng(5).standard_normal((1, 1, 36863))).astype(np.float32)
    worst = restated(case, 1, 36863, False, 1)
    print(worst)
    l1 = B.layer1(case.x, 36)
    _, var, _ = B.stats64(case.x)
    widened = ((36 / 2 + 6) * B.U + l1["mean"][1] ** 2 / (2 * (var + B.EPS))) / ((36 / 2 + 6) * B.U)
    assert worst.pop("invstd") < float(widened[0]) and max(worst.values()) < 1.0, worst


def test_bounds_catch_a_dropped_and_a_duplicated_element():
    """What the GPU tests rely on: statistics that leave one element of a 36864-element plane out (or count it twice) miss the
    layer 1 bounds, at T = 36 and at T = 72."""
    rng = np.random.default_rng(9)
    x = (0.7 + 2 * rng.standard_normal((1, 1, 36864))).astype(np.float32)
    x[0, 0, -1] = 3.0
    for T in (36, 72):
        l1 = B.layer1(x, T)
        for wrong in (x[:, :, :-1], np.concatenate([x, x[:, :, -1:]], 2)):
            mu, var, _ = B.stats64(wrong)
            assert B.ratio(mu * wrong.shape[2] / 36864, *l1["mean"]) > 1.0
        # an element whose statistics are right but whose output was never written is caught by layer 2 (y stays NaN): ratio() -> inf
        assert B.ratio(np.float32("nan"), 0.0, 1.0) == np.inf


# ------------------------------------------------------------------------------- input builders
@pytest.mark.parametrize("batch,hw", B.THRESHOLD_SHAPES)
def test_threshold_channels_converge_and_straddle_the_zero_crossing(batch, hw):
    c = B.THRESHOLD_CHANNELS
    case = B.Case(batch, c, hw, kinds="t" * c)
    signs = set()
    for ch in range(c):
        assert 1 <= case.threshold_rounds[ch] <= B.THRESHOLD_ROUNDS and len(case.threshold_pos[ch]) == B.THRESHOLD_COUNT
        inside, positive = B.near_threshold(case.x[:, ch], case.gamma[ch], case.beta[ch])
        print(batch, hw, ch, "rounds", case.threshold_rounds[ch], "inside the bound", inside, "positive", positive)
        assert inside >= 100 and 0 < positive < inside
        signs.add((float(np.sign(case.x[0, ch, 0])), float(np.sign(case.gamma[ch])), float(np.sign(case.beta[ch]))))
    assert len(signs) == 8


@pytest.mark.parametrize("mask_expr", ["fma", "centred"])
def test_threshold_channels_catch_a_backward_that_decides_the_mask_differently(mask_expr):
    """The float32 restatement with the backward's mask taken from a contracted or a centred expression: some of the eight channels
    flip elements of the block, and layer 3 (mask = y > 0 of the forward, nothing excluded) misses its dx bound there; the kernels' own
    expression passes in every channel."""
    batch, hw = B.THRESHOLD_SHAPES[0]
    c = B.THRESHOLD_CHANNELS
    case = B.Case(batch, c, hw, kinds="t" * c)
    r = B.routes(batch, c, hw, True)
    caught = 0
    for ch in range(c):
        one = lambda a: a[:, ch:ch + 1]      # noqa: E731
        mean, invstd, y = B.emulate_forward(case.x[:, ch], case.gamma[ch], case.beta[ch], r["fwd"], 1)
        save = np.array([[mean], [invstd]], np.float32)
        ratios = {}
        for expr in ("forward", mask_expr):
            _, _, dx = B.emulate_backward(case.x[:, ch], case.dy[:, ch], case.gamma[ch], case.beta[ch], mean, invstd, r["bwd"], 1, expr)
            l3 = B.layer3(one(case.x), one(case.dy), case.gamma[ch:ch + 1], save, y[:, None] > 0, r["bwd"][3])
            ratios[expr] = B.ratio(dx[:, None], *l3["dx"])
        print(mask_expr, "channel", ch, ratios)
        assert ratios["forward"] < 1.0
        caught += ratios[mask_expr] > 1.0
    assert caught >= 1, caught


def test_case_inputs_are_what_the_issue_describes():
    case = B.Case(2, 3, 4100)
    mu, var, _ = B.stats64(case.x)
    assert abs(mu[0] - 0.7) < 0.1 and abs(var[0] - 4.0) < 0.3 and abs(abs(mu[1]) - 1000) < 0.1 and abs(var[1] - 1) < 0.1
    assert abs(abs(mu[2]) - 1000) < 1 and len(case.threshold_pos[2]) == B.THRESHOLD_COUNT
    assert ((0.5 <= case.gamma) & (case.gamma <= 1.5)).all() and (np.abs(case.beta) <= 0.5).all() and len(set(case.gamma)) == 3
    assert case.x.dtype == case.dy.dtype == case.gamma.dtype == case.rm.dtype == np.float32
    assert np.array_equal(case.x, B.Case(2, 3, 4100).x)                       # seeded
    tiny = B.Case(2, 3, 3)                                                     # too small for the block: plain data, no failure
    assert len(tiny.threshold_pos[2]) == 0 and np.isfinite(tiny.x).all()
    spike = B.spike_case(4, 4100, 3, 4099)
    assert (spike.x[3, :, 4099] == 1000).all() and (spike.dy[3, :, 4099] == 1000).all() and (np.abs(spike.x) > 100).sum() == spike.c


# ------------------------------------------------------------------------------- argument checks (nothing is launched)
def fwd(lib, batch, c, hw, sync=None, epoch=0, rm=FAKE, rv=FAKE):
    return lib.toda_bn2d_fwd(FAKE, batch, c, hw, FAKE, FAKE, rm, rv, B.MOMENTUM, B.EPS, 1, FAKE, FAKE, sync, epoch, None)


def bwd(lib, batch, c, hw, sync=None, epoch=0):
    return lib.toda_bn2d_bwd(FAKE, FAKE, batch, c, hw, FAKE, FAKE, FAKE, 1, FAKE, FAKE, FAKE, sync, epoch, None)


def test_unsupported_shapes_are_refused_before_anything_is_launched():
    lib = L.load()
    for call in (fwd, bwd):
        for batch, c, hw in ((3, 3, 100), (1, 3, 36865), (2, 3, 36868), (4, 3, 36868), (0, 3, 16), (2, 3, 0)):
            for sync, epoch in ((None, 0), (FAKE, 1)):
                assert call(lib, batch, c, hw, sync, epoch) == B.EINVAL and b"unsupported shape" in lib.toda_last_error(), (batch, c, hw)
        for batch, hw in B.SPLIT_ONLY:
            assert call(lib, batch, 3, hw, None, 1) == B.EINVAL and b"without a sync workspace" in lib.toda_last_error()
            assert call(lib, batch, 3, hw, FAKE, 0) == B.EINVAL and b"unsupported shape" in lib.toda_last_error()
            assert call(lib, batch, 4097, hw, FAKE, 1) == B.EINVAL and b"unsupported shape" in lib.toda_last_error()
    assert fwd(lib, 2, 3, 100, rm=None) == B.EINVAL and b"go together" in lib.toda_last_error()
    assert fwd(lib, 2, 3, 100, rv=None) == B.EINVAL and b"go together" in lib.toda_last_error()
    into = lambda ch, c0: lib.toda_bn2d_fwd_into(FAKE, 2, 3, 100, FAKE, FAKE, None, None, B.MOMENTUM, B.EPS, 1, FAKE, ch, c0, FAKE, None, 0, None)   # noqa: E731
    frm = lambda ch, c0: lib.toda_bn2d_bwd_from(FAKE, FAKE, ch, c0, 2, 3, 100, FAKE, FAKE, FAKE, 1, FAKE, FAKE, FAKE, None, 0, None)                # noqa: E731
    for call in (into, frm):
        for ch, c0 in ((7, 5), (2, 0), (7, -1), (3, 1)):
            assert call(ch, c0) == B.EINVAL and b"outside" in lib.toda_last_error(), (ch, c0)
