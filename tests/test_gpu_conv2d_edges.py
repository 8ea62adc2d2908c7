"""The dense neck and head convolutions at their tile, split and path edges, against torch.nn.functional.conv2d /
conv_transpose2d in float64:
  * the pixel-GEMMs of gemm2d.hip (stride-2 conv, deconv s = 1, 2) under BOTH matrix paths in one process: every kernel variant
    (native 64 / 128, split, the stride-2 data gradient's parity classes), fast and slow accessors, every weight-gradient split regime;
  * the Winograd F(4x4,3x3) stream-K forward / data gradient / weight gradient of conv2d.hip at its tile, grid, gang and unit edges,
    the two full-size neck shapes, the workspace invariants, the TODA_WINO_VARIANT=0 kernel and the output transform the two
    forward kernels share;
  * the narrow output convolutions of conv2d_narrow.hip at their limits, and the torch fallback beyond them.
Which route each case takes is restated in tests/conv2d_routes.py; tests/test_conv2d_routes.py checks on the CPU that the case lists
below reach every route.  Routes are asserted only on a 256-CU device; values are compared everywhere.  Every case runs twice and must
repeat bit for bit (fixed summation orders: conv2d.hip, gemm2d.hip)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import conv2d_routes as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------------------ case lists
# stride-2 3x3 conv (b, cin, cout, h, w)
S2_CASES = [
    (2, 129, 129, 314, 314),   # native-128 forward and data gradient, slow wgrad accessors, 26 splits (tail of the slab fold)
    (1, 3, 33, 2, 40),         # Ho = 1, cin 9 < PG_K, one split
    (2, 1, 3, 30, 2),          # Wo = 1, a contraction of 9
    (2, 33, 64, 8, 66),        # fast: Wo = 33, Ho Wo = 132 (% 4 == 0, not % 32), B = 2, one split
    (3, 64, 129, 24, 64),      # fast: Wo = 32, 4 splits
    (2, 3, 33, 104, 66),       # fast: Wo = 33, 13 splits, the last one empty
    (1, 40, 24, 18, 10),       # slow, 2 splits
]
# ConvTranspose2d(k = s, stride s) (b, cin, cout, h, w, s)
DECONV_CASES = [
    (2, 129, 129, 157, 157, 1),   # native-128 forward and data gradient, slow accessors, 128 splits
    (3, 1, 33, 1, 40, 1),         # H = 1, a contraction of 1
    (1, 33, 3, 37, 1, 1),         # W = 1
    (2, 33, 3, 6, 22, 1),         # fast: H W = 132, B = 2, one split
    (2, 3, 33, 52, 33, 1),        # fast: 13 splits, the last one empty
    (1, 16, 24, 25, 41, 1),       # slow, 4 splits
    (2, 129, 33, 157, 157, 2),    # native-128 forward and data gradient, slow accessors
    (2, 5, 3, 1, 7, 2),           # H = 1
    (1, 33, 129, 9, 1, 2),        # W = 1
    (2, 33, 3, 4, 33, 2),         # fast: W = 33, H W = 132, B = 2, one split
    (3, 64, 33, 12, 32, 2),       # fast: W = 32, 4 splits
    (2, 3, 32, 52, 33, 2),        # fast: 13 splits, the last one empty
    (1, 17, 7, 30, 35, 2),        # slow (H W % 4 != 0), 4 splits
]
# Winograd conv3x3 (b, cin, cout, h, w): forward, data gradient (roles swapped), weight and bias gradient
WINO_CASES = [
    (1, 32, 32, 1, 2),         # one partial tile, 4 steps
    (2, 32, 64, 2, 4),
    (3, 64, 32, 3, 6),
    (1, 32, 96, 5, 6),         # H % 4 == 1, 3 channel blocks (no gang)
    (33, 32, 32, 4, 4),        # one tile per image: a tile block spans 32 images, the last block holds one tile
    (2, 32, 32, 9, 2),         # H % 4 == 1, W = 2
    (1, 256, 32, 64, 64),      # forward 256 steps on 256 workgroups; data gradient in gangs of 8
    (1, 32, 32, 180, 184),     # 260 steps (just above the grid)
    (1, 32, 512, 40, 40),      # gangs of 16; data gradient: 32 produced from 512 contracted, a unit across 64 workgroups
    (1, 32, 512, 8, 8),        # swapped roles on one tile block
    (1, 64, 256, 40, 40),      # gangs of 8
    (2, 512, 64, 20, 20),      # gangs of 1
    (1, 256, 64, 40, 40),      # gangs of 2
    (2, 64, 320, 13, 30),      # 10 channel blocks: no gang
    (1, 544, 544, 8, 8),       # weight gradient: 289 units (> the grid), one step each
]
NECK_SHAPES = [(2, 128, 128, 188, 188), (2, 256, 256, 94, 94)]
# narrow output convs (b, cin, h, w, couts): 8 branches of up to NW_CO channels
NARROW_CASES = [
    (1, 1, 1, 4, [4, 1, 4, 2, 4, 3, 4, 4]),
    (2, 3, 7, 256, [4, 4, 4, 4, 4, 4, 4, 4]),
    (1, 65, 9, 4, [4, 2, 4, 1, 3, 4, 4, 2]),
    (3, 65, 17, 256, [4, 4, 1, 4, 4, 3, 4, 4]),
    (2, 3, 9, 256, [1, 4]),
]
# shapes the narrow kernels refuse (b, cin, h, w, cout): the head must fall back to torch and still be right
NARROW_UNSUPPORTED = [(2, 64, 9, 260, 2), (2, 64, 9, 6, 3), (2, 64, 10, 12, 5)]
# TODA_PG_WG_TARGET in a child: (kind, shape, target)
# (a single split over 131 k pixels is a plain fp32 running sum: 1.0-1.2e-5 of the fp64 answer, so target 1 runs on maps of 13 default splits)
SPLIT_TARGET_CASES = [("deconv", (2, 3, 32, 52, 33, 2), 1), ("deconv", (2, 3, 32, 256, 256, 2), 4096),
                      ("s2", (2, 3, 33, 104, 66), 1), ("s2", (2, 3, 33, 512, 512), 4096)]

PG_TOL = {"y": 2e-6, "dx": 2e-6, "dw": 5e-6}
WINO_TOL = {"y": 2e-5, "dx": 5e-5, "dw": 5e-5, "db": 5e-5}
NARROW_TOL = 2e-5
GATE_MIN_OUTPUTS = 10_000


def _full_chip():
    return torch.cuda.get_device_properties(0).multi_processor_count == R.N_CU


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))


def _ref_device(*shape):
    n = 1
    for d in shape:
        n *= d
    return "cuda" if n > 4_000_000 else "cpu"


@pytest.fixture
def paths():
    """Switches the library's matrix path inside a test and puts the session's path back afterwards."""
    from toda_amd import ops

    before = ops.matrix_path()
    yield ops
    ops.set_matrix_path(before)


# ------------------------------------------------------------------------------------------------------------ pixel-GEMMs
def _pg_run(ops, kind, shape, x, wt, gy):
    xa, wa = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y = ops.conv3x3s2(xa, wa) if kind == "s2" else ops.deconv(xa, wa, shape[5])
    y.backward(gy)
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": xa.grad, "dw": wa.grad}


def _pg_inputs(kind, shape):
    g = torch.Generator().manual_seed(sum(shape))
    if kind == "s2":
        b, cin, cout, h, w = shape
        x = torch.randn(b, cin, h, w, generator=g)
        wt = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (9 * cin)) ** 0.5
        gy = torch.randn(b, cout, h // 2, w // 2, generator=g)
    else:
        b, cin, cout, h, w, s = shape
        x = torch.randn(b, cin, h, w, generator=g)
        wt = torch.randn(cin, cout, s, s, generator=g) * (1.0 / cin) ** 0.5
        gy = torch.randn(b, cout, h * s, w * s, generator=g)
    return x.cuda(), wt.cuda(), gy.cuda()


def _pg_reference(kind, shape, x, wt, gy):
    dev = _ref_device(*shape[:5])
    xr = x.detach().to(dev, torch.float64).requires_grad_(True)
    wr = wt.detach().to(dev, torch.float64).requires_grad_(True)
    yr = F.conv2d(xr, wr, stride=2, padding=1) if kind == "s2" else F.conv_transpose2d(xr, wr, stride=shape[5])
    yr.backward(gy.to(dev, torch.float64))
    return {"y": yr.detach().cuda(), "dx": xr.grad.cuda(), "dw": wr.grad.cuda()}


def _err_stats(got, ref):
    d = got.double() - ref
    return float(d.square().mean().sqrt()), float(d.abs().max())


@pytest.mark.parametrize("kind,shape", [("s2", s) for s in S2_CASES] + [("deconv", s) for s in DECONV_CASES])
def test_pixel_gemm_both_paths_match_fp64(kind, shape, paths):
    """Forward, data gradient and weight gradient under the native and the split matrix path in one process: each path within the fp64
    bounds and bit-reproducible; the split path's rms / max error at most 1.5 x / 2.5 x the native kernel's (the gate of the sparse
    gather-GEMMs, test_gpu_split.py) on every tensor of 10^4 values or more."""
    ops = paths
    x, wt, gy = _pg_inputs(kind, shape)
    ref = _pg_reference(kind, shape, x, wt, gy)
    got = {}
    for path in ("native", "split"):
        ops.set_matrix_path(path)
        a = _pg_run(ops, kind, shape, x, wt, gy)
        b = _pg_run(ops, kind, shape, x, wt, gy)
        for name in a:
            assert a[name].shape == ref[name].shape, name
            assert torch.equal(a[name], b[name]), (path, name, "not bit-reproducible")
            err = _rel(a[name], ref[name])
            assert err < PG_TOL[name], (path, name, err)
        got[path] = a
    for name in got["native"]:
        if ref[name].numel() < GATE_MIN_OUTPUTS:
            continue
        n_rms, n_max = _err_stats(got["native"][name], ref[name])
        s_rms, s_max = _err_stats(got["split"][name], ref[name])
        assert s_rms <= 1.5 * n_rms + 1e-8 and s_max <= 2.5 * n_max + 1e-7, (name, n_rms, s_rms, n_max, s_max)


def test_pixel_gemm_paths_really_differ(paths):
    """The matrix-path switch routes the pixel-GEMMs: on a large case the two paths' results are not the same bits."""
    ops = paths
    for kind, shape in (("s2", S2_CASES[0]), ("deconv", DECONV_CASES[0])):
        x, wt, gy = _pg_inputs(kind, shape)
        ops.set_matrix_path("native")
        a = _pg_run(ops, kind, shape, x, wt, gy)
        ops.set_matrix_path("split")
        b = _pg_run(ops, kind, shape, x, wt, gy)
        for name in a:
            assert not torch.equal(a[name], b[name]), (kind, shape, name)


_SPLIT_TARGET_CHILD = r"""
import sys, json, torch
import torch.nn.functional as F
sys.path.insert(0, sys.argv[1])
from toda_amd import ops, lib
from tests import conv2d_routes as R
kind, shape, target = json.loads(sys.argv[2])
torch.manual_seed(4)
L = lib.load()
full = torch.cuda.get_device_properties(0).multi_processor_count == R.N_CU
out = {}
for path in ("native", "split"):
    ops.set_matrix_path(path)
    if kind == "s2":
        b, cin, cout, h, w = shape
        x = torch.randn(b, cin, h, w, device="cuda"); wt = torch.randn(cout, cin, 3, 3, device="cuda") * 0.2
        gy = torch.randn(b, cout, h // 2, w // 2, device="cuda")
        route = R.s2_routes(path, *shape, target=target)
        nb, want = L.toda_conv3x3s2_wgrad_workspace_bytes(*shape), R.s2_wgrad_workspace_bytes(*shape, target=target)
        wa = wt.clone().requires_grad_(True); ops.conv3x3s2(x, wa).backward(gy)
        wr = wt.double().requires_grad_(True); F.conv2d(x.double(), wr, stride=2, padding=1).backward(gy.double())
    else:
        b, cin, cout, h, w, s = shape
        x = torch.randn(b, cin, h, w, device="cuda"); wt = torch.randn(cin, cout, s, s, device="cuda") * 0.5
        gy = torch.randn(b, cout, h * s, w * s, device="cuda")
        route = R.deconv_routes(path, *shape, target=target)
        nb, want = L.toda_deconv_wgrad_workspace_bytes(*shape), R.deconv_wgrad_workspace_bytes(*shape, target=target)
        wa = wt.clone().requires_grad_(True); ops.deconv(x, wa, s).backward(gy)
        wr = wt.double().requires_grad_(True); F.conv_transpose2d(x.double(), wr, stride=s).backward(gy.double())
    err = float((wa.grad.double() - wr.grad).abs().max() / wr.grad.abs().max())
    out[path] = {"err": err, "splits": route["splits"], "ws_ok": (nb == want) or not full}
print("RESULT", json.dumps(out))
"""


@pytest.mark.parametrize("kind,shape,target", SPLIT_TARGET_CASES)
def test_weight_gradient_split_count_switch(kind, shape, target):
    """TODA_PG_WG_TARGET (read once per process: a child) drives the weight gradients' contraction splits to 1 and to their cap of
    512; both paths stay within the fp64 bound."""
    import json

    env = dict(os.environ, TODA_PG_WG_TARGET=str(target))
    p = subprocess.run([sys.executable, "-c", _SPLIT_TARGET_CHILD, ROOT, json.dumps([kind, list(shape), target])], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().split("RESULT")[-1])
    for path, r in out.items():
        assert r["err"] < PG_TOL["dw"], (path, r)
        assert r["ws_ok"], (path, r)
        assert r["splits"] == (1 if target == 1 else R.PG_MAX_SPLITS), r


# ------------------------------------------------------------------------------------------------------------ Winograd
def _wino_inputs(shape, seed):
    b, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, cin, h, w), generator=g).cuda()
    wt = (torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5).cuda()
    bias = torch.randn((cout,), generator=g).cuda()
    gy = torch.randn((b, cout, h, w), generator=g).cuda()
    return x, wt, bias, gy


def _wino_run(ops, x, wt, bias, gy):
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, wt, bias))
    y = ops.conv3x3(xa, wa, ba)
    y.backward(gy)
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": xa.grad, "dw": wa.grad, "db": ba.grad}


def _wino_reference(x, wt, bias, gy):
    dev = _ref_device(x.shape[0], max(x.shape[1], wt.shape[0]), x.shape[2], x.shape[3])
    xr, wr, br = (t.detach().to(dev, torch.float64).requires_grad_(True) for t in (x, wt, bias))
    yr = F.conv2d(xr, wr, br, padding=1)
    yr.backward(gy.to(dev, torch.float64))
    return {"y": yr.detach().cuda(), "dx": xr.grad.cuda(), "dw": wr.grad.cuda(), "db": br.grad.cuda()}


def _check_streamk_state(ops, device):
    from toda_amd import lib

    L = lib.load()
    assert L.toda_device_fault() == 0, L.toda_last_error()
    ws = ops._conv3x3_workspace(device)
    flag_bytes = L.toda_conv3x3_workspace_bytes() - R.WS_MAX_GRID * R.WN_COUT * R.WN_TILES * 16 * 4
    assert flag_bytes == 4096
    assert int(ws[:flag_bytes].count_nonzero()) == 0, "stream-K flags left raised"


@pytest.mark.parametrize("shape", WINO_CASES)
def test_winograd_edges_match_fp64(shape):
    """Forward, data gradient, weight and bias gradient of the Winograd convolution at tile, grid, gang and unit edges, against fp64;
    bit-reproducible; the stream-K workspace flags lowered and no device fault after every call."""
    from toda_amd import ops

    if _full_chip():
        fwd, dgd, wgd = R.wino_routes(*shape), R.wino_routes(*shape, direction="dgrad"), R.wino_wgrad_routes(*shape)
        assert 0 < fwd["grid"] <= R.N_CU and 0 < dgd["grid"] <= R.N_CU and 0 < wgd["grid"] <= R.N_CU, (fwd, dgd, wgd)
    x, wt, bias, gy = _wino_inputs(shape, sum(shape))
    ref = _wino_reference(x, wt, bias, gy)
    a = _wino_run(ops, x, wt, bias, gy)
    _check_streamk_state(ops, x.device)
    b = _wino_run(ops, x, wt, bias, gy)
    _check_streamk_state(ops, x.device)
    for name in a:
        assert torch.equal(a[name], b[name]), (name, "not bit-reproducible")
        err = _rel(a[name], ref[name])
        assert err < WINO_TOL[name], (name, err)


@pytest.mark.parametrize("shape", NECK_SHAPES)
def test_winograd_neck_shapes_match_fp64(shape):
    """The two full-size neck layers (2 x 128 x 188 x 188: 556 units, ~35 steps per workgroup, gangs of 4; 2 x 256 x 94 x 94: gangs
    of 2): forward, dx, dw, db against fp64 on the device, bit-reproducible, flags lowered."""
    from toda_amd import ops

    x, wt, bias, gy = _wino_inputs(shape, 11)
    a = _wino_run(ops, x, wt, bias, gy)
    _check_streamk_state(ops, x.device)
    b = _wino_run(ops, x, wt, bias, gy)
    _check_streamk_state(ops, x.device)
    ref = _wino_reference(x, wt, bias, gy)
    for name in a:
        assert torch.equal(a[name], b[name]), (name, "not bit-reproducible")
        err = _rel(a[name], ref[name])
        assert err < WINO_TOL[name], (name, err)


def test_winograd_results_survive_a_shape_change():
    """A call at one shape, then at others (different grids, gangs, unit lengths), then the first again: the same bits - nothing a
    launch leaves in the shared workspace changes the next one."""
    from toda_amd import ops

    first = _wino_inputs(WINO_CASES[8], 1)
    a = _wino_run(ops, *first)
    for shape in (WINO_CASES[7], WINO_CASES[0], WINO_CASES[4]):
        _wino_run(ops, *_wino_inputs(shape, 2))
        _check_streamk_state(ops, first[0].device)
    b = _wino_run(ops, *first)
    _check_streamk_state(ops, first[0].device)
    for name in a:
        assert torch.equal(a[name], b[name]), name


_VARIANT0_CHILD = r"""
import sys, json, torch
import torch.nn.functional as F
sys.path.insert(0, sys.argv[1])
from toda_amd import ops
worst = {"y": 0.0, "dx": 0.0}
for (B, ci, co, H, W) in json.loads(sys.argv[2]):
    g = torch.Generator().manual_seed(B + ci + co + H + W)
    x = torch.randn(B, ci, H, W, generator=g).cuda().requires_grad_(True)
    w = (torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5).cuda()
    b = torch.randn(co, generator=g).cuda()
    gy = torch.randn(B, co, H, W, generator=g).cuda()
    y = ops.conv3x3(x, w, b)
    y.backward(gy)
    y2 = ops.conv3x3(x.detach(), w, b)
    assert torch.equal(y, y2)
    xr = x.detach().double().cpu().requires_grad_(True)
    ref = F.conv2d(xr, w.double().cpu(), b.double().cpu(), padding=1)
    ref.backward(gy.double().cpu())
    worst["y"] = max(worst["y"], float((y.detach().double().cpu() - ref).abs().max() / ref.abs().max()))
    worst["dx"] = max(worst["dx"], float((x.grad.double().cpu() - xr.grad).abs().max() / xr.grad.abs().max()))
print("WORST", json.dumps(worst))
"""


def test_winograd_variant0_fallback_at_the_edges():
    """TODA_WINO_VARIANT=0 (the kernel without inter-workgroup hand-offs that toda_conv3x3_fwd's fault message points to; read once
    per process: a child) on the tile and role edges: forward and data gradient against fp64."""
    import json

    cases = [WINO_CASES[i] for i in (0, 1, 2, 3, 4, 5, 9, 13)]
    env = dict(os.environ, TODA_WINO_VARIANT="0")
    p = subprocess.run([sys.executable, "-c", _VARIANT0_CHILD, ROOT, json.dumps(cases)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    worst = json.loads(p.stdout.strip().split("WORST")[-1])
    assert worst["y"] < WINO_TOL["y"] and worst["dx"] < WINO_TOL["dx"], worst


_EPILOGUE_CHILD = r"""
import sys, json, torch
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_conv2d_edges import _epilogue_outputs
torch.save(_epilogue_outputs(json.loads(sys.argv[2])), sys.argv[3])
"""
# (b, cin, cout, h, w): a ragged two-column row, rows of six columns (a full and a half tile), the 16-byte store
EPILOGUE_CASES = [(1, 8, 32, 1, 2), (2, 8, 64, 5, 6), (3, 8, 32, 8, 8)]


def _epilogue_outputs(cases):
    """y of toda_conv3x3_fwd with bias on 8 input channels (the raw entry point takes Cin % 8), on the CPU."""
    from toda_amd import ops

    out = []
    for shape in cases:
        x, wt, bias, _ = _wino_inputs(tuple(shape), sum(shape))
        out.append(ops.conv3x3_run(x, ops.conv3x3_transform_weight(wt, 0), bias, shape[2]).cpu())
    return out


def test_winograd_both_forward_kernels_share_one_output_transform(tmp_path):
    """With 8 input channels a unit is one chunk: no stream-K hand-off, the same MFMA order in wino_fwd_ws_kernel and in the
    TODA_WINO_VARIANT=0 kernel (a child), and one output transform with bias behind both: the same bits."""
    import json

    out = str(tmp_path / "variant0.pt")
    p = subprocess.run([sys.executable, "-c", _EPILOGUE_CHILD, ROOT, json.dumps(EPILOGUE_CASES), out],
                       env=dict(os.environ, TODA_WINO_VARIANT="0"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    for shape, y, y0 in zip(EPILOGUE_CASES, _epilogue_outputs(EPILOGUE_CASES), torch.load(out)):
        assert y.shape == (shape[0], shape[2], shape[3], shape[4]) and bool(y.abs().sum() > 0), shape
        assert torch.equal(y, y0), (shape, float((y - y0).abs().max()))


# ------------------------------------------------------------------------------------------------------------ narrow convs
def _narrow_modules(cin, couts, seed):
    g = torch.Generator().manual_seed(seed)
    convs = []
    for co in couts:
        c = torch.nn.Conv2d(cin, co, 3, padding=1, bias=True)
        c.weight.data = torch.randn(c.weight.shape, generator=g) * (2.0 / (9 * cin)) ** 0.5
        c.bias.data = torch.randn(co, generator=g)
        convs.append(c.cuda())
    return convs, g


@pytest.mark.parametrize("geom", NARROW_CASES)
@pytest.mark.parametrize("fused", [False, True])
def test_narrow_output_convs_at_their_limits(geom, fused):
    """toda_conv3x3_narrow_{fwd,dgrad,wgrad} with up to NW_MAX_BRANCH branches of up to NW_CO channels, W at 4 and 256, H around the
    wgrad band of 8 rows, cin 1 / 3 / 65; separate inputs and channel slices of one tensor; every output against fp64, bit-reproducible."""
    import copy

    from toda_amd import ops

    b, cin, h, w, couts = geom
    n = len(couts)
    convs, g = _narrow_modules(cin, couts, b + cin + h + w)
    wide = torch.randn((b, n * cin, h, w), generator=g).cuda()
    gys = [torch.randn((b, co, h, w), generator=g).cuda() for co in couts]

    def run():
        cs = [copy.deepcopy(c) for c in convs]
        if fused:
            xa = wide.clone().requires_grad_(True)
            assert all(ops.conv3x3_narrow_supported(xa[:, :cin], c) for c in cs)
            ys = ops.conv3x3_narrow_group_fused(xa, cs)
            torch.autograd.backward(ys, gys)
            dxs = [xa.grad[:, i * cin:(i + 1) * cin] for i in range(n)]
        else:
            xs = [wide[:, i * cin:(i + 1) * cin].contiguous().requires_grad_(True) for i in range(n)]
            assert all(ops.conv3x3_narrow_supported(x, c) for x, c in zip(xs, cs))
            ys = ops.conv3x3_narrow_group(xs, cs)
            torch.autograd.backward(ys, gys)
            dxs = [x.grad for x in xs]
        torch.cuda.synchronize()
        return [(y.detach(), dx, c.weight.grad, c.bias.grad) for y, dx, c in zip(ys, dxs, cs)]

    a, bb = run(), run()
    for i, (c, gy) in enumerate(zip(convs, gys)):
        xd = wide[:, i * cin:(i + 1) * cin].double().cpu().requires_grad_(True)
        wd = c.weight.detach().double().cpu().requires_grad_(True)
        bd = c.bias.detach().double().cpu().requires_grad_(True)
        ref = F.conv2d(xd, wd, bd, padding=1)
        ref.backward(gy.double().cpu())
        for name, got, again, want in zip(("y", "dx", "dw", "db"), a[i], bb[i], (ref.detach(), xd.grad, wd.grad, bd.grad)):
            assert torch.equal(got, again), (i, name, "not bit-reproducible")
            err = float((got.double().cpu() - want).abs().max() / want.abs().max())
            assert err < NARROW_TOL, (i, name, err)


@pytest.mark.parametrize("geom", NARROW_UNSUPPORTED)
def test_head_beyond_the_narrow_limits_falls_back_and_matches_fp64(geom):
    """W = 260 (above 256), W = 6 (not a multiple of 4) and 5 output channels (above NW_CO): conv3x3_narrow_supported says no, and a
    SeparateHead of those shapes still gives the fp64 answer through its branch-by-branch path."""
    import copy

    from toda_amd import lib, ops
    from toda_amd.pcdet.models.dense_heads.center_head import SeparateHead

    b, cin, h, w, cout = geom
    torch.manual_seed(sum(geom))
    x = torch.randn(b, cin, h, w, device="cuda")
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1).cuda()
    assert not ops.conv3x3_narrow_supported(x, conv)
    assert not lib.load().toda_conv3x3_narrow_supported(b, cin, cout, h, w)
    head = SeparateHead(cin, {"a": dict(out_channels=cout, num_conv=2), "b": dict(out_channels=2, num_conv=2)}).cuda().eval()
    ref = copy.deepcopy(head).double()
    with torch.no_grad():
        out = head(x)
        want = ref(x.double())
    for name in ("a", "b"):
        err = float((out[name].double() - want[name]).abs().max() / want[name].abs().max())
        # (the fallback's last layer is torch's own fp32 convolution behind a Winograd hidden layer and BatchNorm: 1e-4 of the output scale)
        assert out[name].shape == want[name].shape and err < 1e-4, (name, err)
