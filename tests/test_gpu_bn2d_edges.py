"""The single-pass BatchNorm2d kernels of csrc/bn2d.hip at their register-image edges: every (direction, family, V, batch, K)
instantiation the launchers can reach (tests/test_bn2d_host.py proves on the CPU that the case list of tests/bn2d_cases.py reaches all
66), the k-slices that lie past the end of a plane, the partner exchange of the per-plane kernels on both workgroup mappings, channel
slices, planes that start off a 16-byte boundary, and the ReLU mask contract (backward recomputes the forward's decision bit for bit).
The C ABI is called directly; every input and output lies between NaN guard bands which must survive bit for bit; every case runs
twice and must repeat bit for bit; after every launch that was given a sync workspace toda_device_fault() must be 0.

Bounds (tests/bn2d_cases.py, all derived, u = 2^-24, T = floats a thread adds in float32):
  layer 1  save and the running statistics against float64 of x:  |mean - mu| <= (T - 1) u mean|x| + u |mu|,  invstd within
           (T / 2 + 6) u relative, the running pair within momentum times these plus three roundings;
  layer 2  y against float64 arithmetic on x and the SAVED statistics:  4 u (|x s| + |mean s| + |beta|) per element;
  layer 3  dbeta, dgamma, dx against float64 arithmetic on x, dy, the saved statistics and the mask (y_kernel > 0) - no element is
           excluded anywhere: an element whose mask differs between forward and backward misses the dx bound by |s g|.
The worst error / bound per layer is printed by every test and once more for the whole module."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import bn2d_cases as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
PAD = 64            # floats: 256 bytes, so `off` alone decides the 16-byte alignment of a tensor
WORST = {}


class Guarded:
    """`numel` float32 elements between two NaN guard bands; .t is the contiguous view the kernel gets, starting `off` floats past a
    256-byte boundary."""

    def __init__(self, shape, off=0, fill=NAN):
        self.numel, self.start = int(np.prod(shape)), PAD + off
        self.full = torch.full((self.numel + 2 * PAD + 4,), NAN, dtype=torch.float32, device="cuda")
        self.t = self.full[self.start:self.start + self.numel].view(*shape)
        assert self.t.data_ptr() % 16 == 4 * (off % 4)
        if fill == fill:
            self.t.fill_(fill)

    @classmethod
    def of(cls, array, off=0):
        array = np.ascontiguousarray(array, np.float32)
        g = cls(array.shape, off)
        g.t.copy_(torch.from_numpy(array))
        return g

    def intact(self):
        return bool(torch.isnan(self.full[:self.start]).all()) and bool(torch.isnan(self.full[self.start + self.numel:]).all())

    def untouched(self):
        return bool(torch.isnan(self.full).all())

    def np(self):
        return self.t.cpu().numpy()


class Sync:
    """The partner workgroups' exchange area: zeroed once, every launch takes an epoch it has not seen."""

    def __init__(self, lib, epochs=None):
        self.ws = torch.zeros((lib.toda_bn2d_sync_bytes(),), dtype=torch.uint8, device="cuda")
        self.epochs, self.last = (iter(epochs) if epochs is not None else None), 0

    def take(self):
        self.last = next(self.epochs) if self.epochs is not None else self.last + 1
        return self.last


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at flat index {i}: got {got.ravel()[i]!r}, "
                             f"want {want.ravel()[i]!r}")


@pytest.fixture(scope="module")
def lib():
    from toda_amd import lib as L

    return L.load()


@pytest.fixture(scope="module")
def shared_sync(lib):
    return Sync(lib)


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print("\nbn2d edges, worst error / bound per layer over the module:", json.dumps({k: round(v, 4) for k, v in sorted(WORST.items())}))


def P(t):
    from toda_amd import lib as L

    return None if t is None else L.ptr(t.t if isinstance(t, Guarded) else t)


def stream():
    from toda_amd import lib as L

    return L.stream()


OUTPUTS = ("y", "save", "rm", "rv", "dx", "dgamma", "dbeta")


def sentinel(shape):
    return ((np.arange(int(np.prod(shape))) % 977) + 0.5).astype(np.float32).reshape(shape)


def run(lib, case, relu, sync=None, off=0, running=True, into=None, frm=None, backward=True):
    """One forward and one backward call on fresh guarded tensors.  into / frm: (channels, channel0) of the wider y / dy tensor the
    slice entry points get (y pre-filled with a sentinel pattern, the other channels of dy NaN).  -> namespace of return codes and
    numpy outputs; guard bands and read-only inputs are checked here."""
    b, c, hw = case.batch, case.c, case.hw
    x, gamma, beta = Guarded.of(case.x, off), Guarded.of(case.gamma), Guarded.of(case.beta)
    rm, rv = (Guarded.of(case.rm), Guarded.of(case.rv)) if running else (None, None)
    save = Guarded((2, c))
    ws = P(sync.ws) if sync is not None else None
    if into is None:
        y = Guarded((b, c, hw), off)
        rc_fwd = lib.toda_bn2d_fwd(P(x), b, c, hw, P(gamma), P(beta), P(rm), P(rv), B.MOMENTUM, B.EPS, relu, P(y), P(save), ws,
                                   sync.take() if sync else 0, stream())
    else:
        y = Guarded.of(sentinel((b, into[0], hw)), off)
        rc_fwd = lib.toda_bn2d_fwd_into(P(x), b, c, hw, P(gamma), P(beta), P(rm), P(rv), B.MOMENTUM, B.EPS, relu, P(y), into[0], into[1],
                                        P(save), ws, sync.take() if sync else 0, stream())
    out = types.SimpleNamespace(rc_fwd=rc_fwd, rc_bwd=None, guards=[x, gamma, beta, rm, rv, save, y], fwd_untouched=save.untouched())
    dx, dgamma, dbeta = Guarded((b, c, hw), off), Guarded((c,)), Guarded((c,))
    if backward:
        if frm is None:
            dy = Guarded.of(case.dy, off)
            out.rc_bwd = lib.toda_bn2d_bwd(P(x), P(dy), b, c, hw, P(gamma), P(beta), P(save), relu, P(dx), P(dgamma), P(dbeta), ws,
                                           sync.take() if sync else 0, stream())
        else:
            wide = np.full((b, frm[0], hw), NAN, np.float32)
            wide[:, frm[1]:frm[1] + c] = case.dy
            dy = Guarded.of(wide, off)
            out.rc_bwd = lib.toda_bn2d_bwd_from(P(x), P(dy), frm[0], frm[1], b, c, hw, P(gamma), P(beta), P(save), relu, P(dx), P(dgamma),
                                                P(dbeta), ws, sync.take() if sync else 0, stream())
        out.guards += [dy, dx, dgamma, dbeta]
        out.bwd_untouched = dx.untouched() and dgamma.untouched() and dbeta.untouched()
        assert np.array_equal(bits(dy.np()), bits(wide if frm is not None else case.dy)), "dy is read only"
    torch.cuda.synchronize()
    if sync is not None:
        assert lib.toda_device_fault() == 0, lib.toda_last_error()
    for g in out.guards:
        assert g is None or g.intact(), "a guard band was written"
    assert np.array_equal(bits(x.np()), bits(case.x)), "x is read only"
    assert np.array_equal(gamma.np(), case.gamma) and np.array_equal(beta.np(), case.beta)
    out.y, out.save, out.dx, out.dgamma, out.dbeta = y.np(), save.np(), dx.np(), dgamma.np(), dbeta.np()
    out.rm, out.rv = (rm.np(), rv.np()) if running else (None, None)
    out.y_untouched = y.untouched() if into is None else np.array_equal(bits(out.y), bits(sentinel(out.y.shape)))
    return out


def same_outputs(a, b, what, channels=None):
    for name in OUTPUTS:
        u, v = getattr(a, name), getattr(b, name)
        if u is None or v is None:
            continue
        if channels is not None:
            axis = {"y": 1, "dx": 1, "save": 1}.get(name, 0)
            u, v = np.take(u, channels, axis), np.take(v, channels, axis)
        assert_same_bits(u, v, f"{what}: {name}")


def note(worst, name, value, what):
    worst[name] = max(worst.get(name, 0.0), value)
    WORST[name] = max(WORST.get(name, 0.0), value)
    assert value <= 1.0, f"{what}: {name} misses its bound, error / bound = {value:.4g}"


def check_layers(case, res, relu, r, what, worst, y=None, l1=None):
    """Layers 1 - 3 of one result.  r: routes of the launch; y: the case's channels of the forward output (res.y by default)."""
    assert res.rc_fwd == 0 and res.rc_bwd in (0, None), what
    y = res.y if y is None else y
    l1 = l1 or B.layer1(case.x, r["fwd"][3], case.rm, case.rv)
    got = {"mean": res.save[0], "invstd": res.save[1], "running_mean": res.rm, "running_var": res.rv}
    for name, (ref, bound) in l1.items():
        if got[name] is not None:
            note(worst, "1 " + name, B.ratio(got[name], ref, bound), what)
    z, y_ref, bound = B.layer2(case.x, case.gamma, case.beta, res.save, relu)
    note(worst, "2 y", B.ratio(y, y_ref, bound), what)
    if relu:
        assert (y >= 0).all() and not np.signbit(y[y == 0]).any(), what
    if res.rc_bwd is None:
        return
    l3 = B.layer3(case.x, case.dy, case.gamma, res.save, (y > 0) if relu else None, r["bwd"][3])
    assert np.isfinite(res.dx).all(), what
    for name in ("dbeta", "dgamma", "dx"):
        note(worst, "3 " + name, B.ratio(getattr(res, name), *l3[name]), what)


def refused(lib, res, what):
    assert res.rc_fwd == B.EINVAL and res.rc_bwd == B.EINVAL, (what, res.rc_fwd, res.rc_bwd)
    assert res.fwd_untouched and res.y_untouched and res.bwd_untouched, what + ": a refused call wrote to its outputs"
    assert lib.toda_device_fault() == 0


def sweep_case(lib, case, shared_sync, off=0):
    """sync {given, NULL} x relu {0, 1}, each twice; the statistics reference is shared by the launches of one T"""
    batch, c, hw = case.batch, case.c, case.hw
    worst, l1 = {}, {}
    for given in (True, False):
        r = B.routes(batch, c, hw, given)
        for relu in (0, 1):
            what = f"batch={batch} c={c} hw={hw} sync={'given' if given else 'NULL'} relu={relu} off={off} routes={r}"
            res = run(lib, case, relu, shared_sync if given else None, off)
            if r["fwd"] is None:
                assert r["bwd"] is None
                refused(lib, res, what)
                assert np.array_equal(res.rm, case.rm) and np.array_equal(res.rv, case.rv)
                continue
            T = r["fwd"][3]
            if T not in l1:
                l1[T] = B.layer1(case.x, T, case.rm, case.rv)
            check_layers(case, res, relu, r, what, worst, l1=l1[T])
            same_outputs(run(lib, case, relu, shared_sync if given else None, off), res, "second run of " + what)
    print(f"batch={batch} c={c} hw={hw} off={off} err/bound:", " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))


# ================================================================================================ the case list
@pytest.mark.parametrize("hw,batch", B.SWEEP)
def test_every_instantiation_meets_the_float64_bounds(lib, shared_sync, hw, batch):
    sweep_case(lib, B.Case(batch, B.SWEEP_C, hw), shared_sync)


@pytest.mark.parametrize("batch,c,hw", B.MAPPING_CASES)
def test_split_routes_on_both_workgroup_mappings(lib, shared_sync, batch, c, hw):
    """C = 8: partners interleaved in groups of eight channels; C = 9: partners side by side"""
    sweep_case(lib, B.Case(batch, c, hw), shared_sync)


@pytest.mark.parametrize("hw,batch", B.MISALIGNED)
def test_dword_kernels_take_planes_off_a_16_byte_boundary(lib, shared_sync, hw, batch):
    """x, dy, y and dx each start one float past a 16-byte boundary; the results are those of the aligned run, bit for bit"""
    case = B.Case(batch, B.SWEEP_C, hw)
    sweep_case(lib, case, shared_sync, off=1)
    same_outputs(run(lib, case, 1, shared_sync, off=1), run(lib, case, 1, shared_sync, off=0), f"off=1 against off=0, batch={batch} hw={hw}")


# ================================================================================================ probes
@pytest.mark.parametrize("hw,batch", B.SPIKE_SHAPES)
def test_position_spikes_are_counted_exactly_once(lib, shared_sync, hw, batch):
    """one element of x and one of dy set to 1000, one position per launch: dropped or duplicated, it misses layers 1 - 3 by orders
    of magnitude"""
    worst = {}
    r = B.routes(batch, 2, hw, True)
    for plane in sorted({0, batch - 1}):
        for pos in B.spike_positions(hw):
            case = B.spike_case(batch, hw, plane, pos)
            what = f"spike at plane {plane} position {pos}, batch={batch} hw={hw} routes={r}"
            res = run(lib, case, 1, shared_sync)
            check_layers(case, res, 1, r, what, worst)
    print(f"spikes batch={batch} hw={hw} err/bound:", " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("hw", B.NEIGHBOUR_HW)
def test_a_poisoned_neighbour_channel_changes_nothing(lib, shared_sync, hw):
    """channel 1 of x and dy all NaN, then all +inf: channels 0 and 2 of every output equal the run on ordinary data bit for bit -
    k-slices past the end of a plane read zeros, never the next plane"""
    for batch in B.BATCHES:
        case = B.Case(batch, 3, hw)
        for relu in (0, 1):
            want = run(lib, case, relu, shared_sync)
            assert want.rc_fwd == 0 and want.rc_bwd == 0
            for poison in (NAN, float("inf")):
                bad = B.Case(batch, 3, hw)
                bad.x[:, 1], bad.dy[:, 1] = poison, poison
                got = run(lib, bad, relu, shared_sync)
                assert got.rc_fwd == 0 and got.rc_bwd == 0
                same_outputs(got, want, f"poison {poison} batch={batch} hw={hw} relu={relu}", channels=[0, 2])


@pytest.mark.parametrize("batch,hw", B.SLICE_SHAPES)
def test_channel_slices_of_a_wider_tensor(lib, shared_sync, batch, hw):
    """toda_bn2d_fwd_into writes channels [2, 5) of a 7-channel y, toda_bn2d_bwd_from reads channels [2, 5) of a 7-channel dy whose
    other channels are NaN: the slice meets layers 1 - 3, every other channel is unchanged bit for bit"""
    case = B.Case(batch, 3, hw)
    r = B.routes(batch, 3, hw, True)
    worst = {}
    for relu in (0, 1):
        what = f"slice batch={batch} hw={hw} relu={relu} routes={r}"
        res = run(lib, case, relu, shared_sync, into=(7, 2), frm=(7, 2))
        keep = sentinel(res.y.shape)
        for ch in (0, 1, 5, 6):
            assert_same_bits(res.y[:, ch], keep[:, ch], f"{what}: channel {ch} of y")
        check_layers(case, res, relu, r, what, worst, y=res.y[:, 2:5])
        again = run(lib, case, relu, shared_sync, into=(7, 2), frm=(7, 2))
        same_outputs(again, res, "second run of " + what)
        # the slice entry points give the bits of the plain ones
        plain = run(lib, case, relu, shared_sync)
        assert_same_bits(res.y[:, 2:5], plain.y, what + ": y against toda_bn2d_fwd")
        for name in ("save", "rm", "rv", "dx", "dgamma", "dbeta"):
            assert_same_bits(getattr(res, name), getattr(plain, name), f"{what}: {name} against the plain entry points")
    print(f"slices batch={batch} hw={hw} err/bound:", " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("batch,hw", B.THRESHOLD_SHAPES)
def test_relu_mask_is_the_forwards_decision_bit_for_bit(lib, shared_sync, batch, hw):
    """Eight channels with 1025 elements each within +-32 ulp of the zero crossing: at least 100 of them per channel lie inside the
    layer 2 bound, where only the forward's own float32 expression decides the sign.  Backward against the mask y_kernel > 0 with no
    element left out: a backward that evaluates the expression differently (contracted, centred) flips some of them."""
    c = B.THRESHOLD_CHANNELS
    case = B.Case(batch, c, hw, kinds="t" * c)
    for ch in range(c):
        inside, positive = B.near_threshold(case.x[:, ch], case.gamma[ch], case.beta[ch])
        assert inside >= 100 and 0 < positive < inside
    r = B.routes(batch, c, hw, True)
    worst = {}
    what = f"threshold batch={batch} hw={hw} routes={r}"
    res = run(lib, case, 1, shared_sync)
    check_layers(case, res, 1, r, what, worst)
    # the block is split by the mask in every channel, and the gradient of a masked element is exactly the common part
    for ch in range(c):
        flat = res.y[:, ch].ravel()[case.threshold_pos[ch]]
        assert 0 < (flat > 0).sum() < flat.size, (what, ch)
    same_outputs(run(lib, case, 1, shared_sync), res, "second run of " + what)
    print(f"threshold batch={batch} hw={hw} err/bound:", " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))


def constant_case(batch, hw, planes):
    """channel 0: the constant planes[b] per sample; channel 1: ordinary data"""
    case = B.Case(batch, 2, hw, kinds="ww")
    for b in range(batch):
        case.x[b, 0] = planes[b]
    return case


@pytest.mark.parametrize("batch,hw", [(1, 4100), (2, 5), (2, 16388), (4, 16388), (4, 9217)])
def test_a_constant_channel_has_zero_variance(lib, shared_sync, batch, hw):
    """var = 0, invstd = 1 / sqrt(eps) exactly (3.0: every partial sum is exact; 0.7: the variance is some 1e-15, far below half an
    ulp of eps), y within the layer 2 bound of beta, dx finite and within layer 3"""
    want = np.float32(1) / np.sqrt(np.float32(B.EPS))
    r = B.routes(batch, 2, hw, True)
    for value in (3.0, 0.7):
        case = constant_case(batch, hw, [value] * batch)
        for relu in (0, 1):
            what = f"constant {value} batch={batch} hw={hw} relu={relu} routes={r}"
            res = run(lib, case, relu, shared_sync)
            assert res.save[1, 0] == want and (value != 3.0 or res.save[0, 0] == 3.0), (what, res.save[:, 0])
            check_layers(case, res, relu, r, what, {})
            assert np.isfinite(res.dx).all()


@pytest.mark.parametrize("batch,hw", [(2, 4100), (2, 16388), (4, 16388), (2, 1), (2, 3), (4, 18433)])
def test_per_plane_constants_merge_to_the_channel_variance(lib, shared_sync, batch, hw):
    """x = a in the even samples and b in the odd ones: mean (a + b) / 2, var (a - b)^2 / 4 - the merge of the planes' moments (in the
    per-plane forward the Chan update, batch 4) against its closed form; hw 1 and 3 with batch 2"""
    a, b = 1.5, -2.25
    case = constant_case(batch, hw, [a, b] * (batch // 2))
    r = B.routes(batch, 2, hw, True)
    for relu in (0, 1):
        what = f"planes {a} / {b} batch={batch} hw={hw} relu={relu} routes={r}"
        res = run(lib, case, relu, shared_sync)
        check_layers(case, res, relu, r, what, {})
        inv = 1.0 / np.sqrt((a - b) ** 2 / 4 + B.EPS)
        assert res.save[0, 0] == np.float32((a + b) / 2) and abs(res.save[1, 0] / inv - 1) <= (r["fwd"][3] / 2 + 6) * B.U, what


@pytest.mark.parametrize("batch,hw", [(2, 4100), (4, 16388), (1, 5)])
def test_running_statistics_are_nullable_together(lib, shared_sync, batch, hw):
    case = B.Case(batch, 3, hw)
    for relu in (0, 1):
        with_stats = run(lib, case, relu, shared_sync)
        without = run(lib, case, relu, shared_sync, running=False)
        assert without.rc_fwd == 0 and without.rc_bwd == 0
        same_outputs(without, with_stats, f"running statistics NULL, batch={batch} hw={hw}")
    x, gamma, beta, rm = Guarded.of(case.x), Guarded.of(case.gamma), Guarded.of(case.beta), Guarded.of(case.rm)
    for first, second in ((rm, None), (None, rm)):
        y, save = Guarded((batch, 3, hw)), Guarded((2, 3))
        rc = lib.toda_bn2d_fwd(P(x), batch, 3, hw, P(gamma), P(beta), P(first), P(second), B.MOMENTUM, B.EPS, 1, P(y), P(save), P(shared_sync.ws),
                               shared_sync.take(), stream())
        torch.cuda.synchronize()
        assert rc == B.EINVAL and y.untouched() and save.untouched() and rm.intact() and np.array_equal(rm.np(), case.rm)
    assert lib.toda_device_fault() == 0


def test_refusals_return_einval_and_write_nothing(lib, shared_sync):
    small = B.Case(2, 3, 8)

    def attempt(batch, c, hw, sync, epoch, into=None, frm=None, what=""):
        """fwd and bwd with NaN-filled outputs; the inputs are never read, so small ones stand in for any shape"""
        x, dy, par = Guarded.of(small.x), Guarded.of(small.dy), Guarded.of(small.gamma)
        rm, rv, save_in = Guarded.of(small.rm), Guarded.of(small.rv), Guarded.of(np.ones((2, 3), np.float32))
        outs = [Guarded((48,)) for _ in range(5)]
        y, save, dx, dgamma, dbeta = outs
        ws = P(sync.ws) if sync is not None else None
        ych, y0 = into or (c, 0)
        gch, g0 = frm or (c, 0)
        rc_f = lib.toda_bn2d_fwd_into(P(x), batch, c, hw, P(par), P(par), P(rm), P(rv), B.MOMENTUM, B.EPS, 1, P(y), ych, y0, P(save), ws, epoch,
                                      stream())
        rc_b = lib.toda_bn2d_bwd_from(P(x), P(dy), gch, g0, batch, c, hw, P(par), P(par), P(save_in), 1, P(dx), P(dgamma), P(dbeta), ws, epoch,
                                      stream())
        torch.cuda.synchronize()
        assert rc_f == B.EINVAL and rc_b == B.EINVAL, (what, rc_f, rc_b)
        assert all(o.untouched() for o in outs), what
        assert np.array_equal(rm.np(), small.rm) and np.array_equal(rv.np(), small.rv) and rm.intact() and rv.intact(), what
        assert lib.toda_device_fault() == 0, what

    for given in (False, True):
        sync, epoch = (shared_sync, shared_sync.take()) if given else (None, 0)
        attempt(3, 3, 8, sync, epoch, what="batch 3")
        attempt(2, 3, 36865, sync, epoch, what="hw 36865")
        attempt(2, 3, 36868, sync, epoch, what="hw 36868")
    for batch, hw in B.SPLIT_ONLY:
        attempt(batch, 3, hw, None, 0, what="split-only shape without a workspace")
        attempt(batch, 3, hw, shared_sync, 0, what="split-only shape with epoch 0")
        attempt(batch, 4097, hw, shared_sync, shared_sync.take(), what="split-only shape with 4097 channels")
    attempt(2, 3, 8, None, 0, into=(7, 5), frm=(7, 5), what="channel0 + c > channels")
    attempt(2, 3, 8, None, 0, into=(7, -1), frm=(7, -1), what="negative channel0")


def test_one_workspace_serves_mixed_split_launches(lib):
    """One zeroed workspace per direction, launches with mixed (C, P) and epochs up to 0xFFFFFFFF, never one twice, one stream: every
    result equals the same call on a fresh workspace with epoch 1 bit for bit"""
    ws_fwd, ws_bwd = Sync(lib, []), Sync(lib, [])
    for (c, p), epoch in zip(B.REUSE_SEQUENCE, B.REUSE_EPOCHS):
        case = B.Case(p, c, B.REUSE_HW)
        r = B.routes(p, c, B.REUSE_HW, True)
        assert r["bwd"][0] == "split"
        fresh = run(lib, case, 1, Sync(lib))                      # epochs 1 (forward) and 2 (backward) on a workspace of its own
        fresh_b = reuse_backward(lib, case, fresh.save, Sync(lib, [1]))
        assert_same_bits(fresh_b.dx, fresh.dx, "backward with epoch 1 against epoch 2 on fresh workspaces")
        if r["fwd"][0] == "split":
            ws_fwd.epochs = iter([epoch])
            got = run(lib, case, 1, ws_fwd, backward=False)
            for name in ("y", "save", "rm", "rv"):
                assert_same_bits(getattr(got, name), getattr(fresh, name), f"forward (C, P) = {(c, p)} epoch {epoch:#x}: {name}")
        ws_bwd.epochs = iter([epoch])
        got = reuse_backward(lib, case, fresh.save, ws_bwd)
        for name in ("dx", "dgamma", "dbeta"):
            assert_same_bits(getattr(got, name), getattr(fresh, name), f"backward (C, P) = {(c, p)} epoch {epoch:#x}: {name}")


def reuse_backward(lib, case, save_np, sync):
    b, c, hw = case.batch, case.c, case.hw
    x, dy, gamma, beta, save = Guarded.of(case.x), Guarded.of(case.dy), Guarded.of(case.gamma), Guarded.of(case.beta), Guarded.of(save_np)
    dx, dgamma, dbeta = Guarded((b, c, hw)), Guarded((c,)), Guarded((c,))
    rc = lib.toda_bn2d_bwd(P(x), P(dy), b, c, hw, P(gamma), P(beta), P(save), 1, P(dx), P(dgamma), P(dbeta), P(sync.ws), sync.take(), stream())
    torch.cuda.synchronize()
    assert rc == 0 and lib.toda_device_fault() == 0, lib.toda_last_error()
    assert dx.intact() and dgamma.intact() and dbeta.intact()
    return types.SimpleNamespace(dx=dx.np(), dgamma=dgamma.np(), dbeta=dbeta.np())


_ENV_SPLIT_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from tests import bn2d_cases as B
from tests import test_gpu_bn2d_edges as E
from toda_amd import lib as L
lib = L.load()
out = []
for batch, c, hw in json.loads(sys.argv[2]):
    case = B.Case(batch, c, hw)
    sync = E.Sync(lib)
    r = B.routes(batch, c, hw, True, env_split=0)
    for relu in (0, 1):
        given, null = E.run(lib, case, relu, sync), E.run(lib, case, relu, None)
        E.same_outputs(given, null, "sync given against NULL")
        worst = {}
        E.check_layers(case, given, relu, r, "TODA_BN2D_SPLIT=0 batch=%d hw=%d relu=%d" % (batch, hw, relu), worst)
        out.append(worst)
print("RESULT", json.dumps(out))
"""


def test_env_switch_keeps_the_per_channel_backward():
    """TODA_BN2D_SPLIT=0 (read once per process: a child): backward with a workspace runs the per-channel kernel - the bits of the call
    without one - and meets the layer 3 bounds at that kernel's T"""
    for batch, c, hw in B.ENV_SPLIT_SHAPES:
        assert B.routes(batch, c, hw, True, env_split=0)["bwd"][0] == "channel" and B.routes(batch, c, hw, True)["bwd"][0] == "split"
    env = dict(os.environ, TODA_BN2D_SPLIT="0")
    p = subprocess.run([sys.executable, "-c", _ENV_SPLIT_CHILD, ROOT, json.dumps(B.ENV_SPLIT_SHAPES)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    worst = json.loads(p.stdout.strip().split("RESULT")[-1])
    print("TODA_BN2D_SPLIT=0 err/bound:", worst)
    assert len(worst) == 4 and all(v <= 1.0 for w in worst for v in w.values())
