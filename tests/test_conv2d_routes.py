"""CPU checks of tests/conv2d_routes.py (the launch decisions of gemm2d.hip and conv2d.hip restated in Python): the restatement
agrees with every host-side query of the library that exposes the same rule, and the case lists of test_gpu_conv2d_edges.py
reach every kernel variant, accessor, split regime, stream-K and gang edge they are meant to.  A change to the kernels'
thresholds or to the case lists that drops a route fails here, on any host."""
import os

import pytest

from tests import conv2d_routes as R
from tests import test_gpu_conv2d_edges as E
from toda_amd import lib as L

TARGET = int(os.environ.get("TODA_PG_WG_TARGET", R.PG_WG_TARGET))     # what the library in this process reads


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_pg_split_rule_matches_the_workspace_queries(lib):
    """toda_conv3x3s2_wgrad_workspace_bytes / toda_deconv_wgrad_workspace_bytes are sized by pg_splits: equal on every GPU case and on a
    sweep that crosses the length cap, the target and the 512 cap."""
    shapes_s2 = list(E.S2_CASES) + [(b, ci, co, h, w) for b in (1, 3) for ci in (1, 14, 15, 200) for co in (1, 128, 129, 700)
                                    for h, w in ((2, 2), (64, 66), (300, 2), (512, 512))]
    for s in shapes_s2:
        assert lib.toda_conv3x3s2_supported(*s) == 1, s
        assert lib.toda_conv3x3s2_wgrad_workspace_bytes(*s) == R.s2_wgrad_workspace_bytes(*s, target=TARGET), s
    shapes_dc = list(E.DECONV_CASES) + [(b, ci, co, h, w, st) for b in (1, 2) for ci in (1, 128, 129) for co in (1, 32, 33, 300)
                                        for h, w in ((1, 1), (16, 16), (256, 256), (700, 1)) for st in (1, 2)]
    for s in shapes_dc:
        assert lib.toda_deconv_supported(*s) == 1, s
        assert lib.toda_deconv_wgrad_workspace_bytes(*s) == R.deconv_wgrad_workspace_bytes(*s, target=TARGET), s
    for kind, s, _ in E.SPLIT_TARGET_CASES:
        assert (lib.toda_conv3x3s2_supported(*s) if kind == "s2" else lib.toda_deconv_supported(*s)) == 1


def test_support_rules_match_the_library(lib):
    for s in E.WINO_CASES + E.NECK_SHAPES:
        assert lib.toda_conv3x3_supported(*s) == 1 and R.wino_supported(*s), s
        cin, cout = s[1], s[2]
        assert lib.toda_conv3x3_wgrad_workspace_bytes(*s) == R.wino_wgrad_workspace_bytes(cin, cout), s
    for b, cin, h, w, couts in E.NARROW_CASES:
        assert len(couts) <= R.NW_MAX_BRANCH
        for co in couts:
            assert lib.toda_conv3x3_narrow_supported(b, cin, co, h, w) == 1 and R.narrow_supported(b, cin, co, h, w)
        # the fused entry point reads the branches as channel slices of one n x cin tensor
        assert lib.toda_conv3x3_narrow_supported(b, len(couts) * cin, 1, h, w) == 1
    for b, cin, h, w, co in E.NARROW_UNSUPPORTED:
        assert lib.toda_conv3x3_narrow_supported(b, cin, co, h, w) == 0 and not R.narrow_supported(b, cin, co, h, w)
    # the rules' own edges
    for s in [(1, 32, 32, 1, 3), (1, 16, 32, 4, 4), (1, 32, 48, 4, 4), (0, 32, 32, 4, 4), (1, 32, 32, 4, 1)]:
        assert lib.toda_conv3x3_supported(*s) == int(R.wino_supported(*s)) == 0, s
    for s in [(1, 1, 4, 1, 4), (1, 1, 5, 1, 4), (1, 1, 4, 1, 256), (1, 1, 4, 1, 260), (1, 1, 1, 1, 6), (1, 1, 1, 0, 4)]:
        assert lib.toda_conv3x3_narrow_supported(*s) == int(R.narrow_supported(*s)), s
    assert lib.toda_conv3x3s2_supported(1, 1, 1, 3, 4) == 0 and lib.toda_conv3x3s2_supported(1, 1, 1, 2, 2) == 1
    assert lib.toda_deconv_supported(1, 1, 1, 1, 1, 3) == 0


def _pg_routes():
    """Every (op, path) route the pixel-GEMM cases take, as (op, direction, label) triples, op in s2 / deconv1 / deconv2."""
    seen = set()
    for path in ("native", "split"):
        for s in E.S2_CASES:
            r = R.s2_routes(path, *s, target=TARGET)
            seen.add(("s2", "fwd", r["fwd"]))
            seen.add(("s2", "dgrad", r["dgrad"]))
            seen.add(("s2", "dgrad", f"{r['dgrad']}/{r['dgrad_classes']}classes"))
            seen.add(("s2", "wgrad", r["wgrad"]))
        for s in E.DECONV_CASES:
            r = R.deconv_routes(path, *s, target=TARGET)
            op = f"deconv{s[5]}"
            for d in ("fwd", "dgrad", "wgrad"):
                seen.add((op, d, r[d]))
    return seen


def _wgrad_regimes(op, cases, routes):
    seen = set()
    for s in cases:
        r = routes("native", *s, target=TARGET)
        b, h, w = s[0], s[3], s[4]
        ow = w // 2 if op == "s2" else w            # the row the wgrad's pixel chunks walk: output row of the conv, input row of the deconv
        hw = (h // 2) * (w // 2) if op == "s2" else h * w
        seen.add("fast" if r["fast"] else "slow")
        if r["splits"] == 1:
            seen.add("splits=1")
        elif r["splits"] < 8:
            seen.add("splits=2..7")
        elif r["splits"] % 8:
            seen.add("splits>=8,%8!=0")
        if r["empty"] > 0:
            seen.add("empty split")
        if r["fast"]:
            if ow in (32, 33) and (op != "deconv1"):
                seen.add(f"fast Wo={ow}")
            if hw % 4 == 0 and hw % 32:
                seen.add("fast hw%32!=0")
            if b > 1:
                seen.add("fast B>1")
            if r["splits"] > 1:
                seen.add("fast splits>1")
    return seen


PG_ROUTES = {(op, d, k) for op in ("s2", "deconv1", "deconv2") for d in ("fwd", "dgrad", "wgrad") for k in ("native64", "native128", "split")}
PG_ROUTES |= {("s2", "dgrad", f"{k}/4classes") for k in ("native64", "native128", "split")}
WGRAD_REGIMES = {"fast", "slow", "splits=1", "splits=2..7", "splits>=8,%8!=0", "empty split", "fast hw%32!=0", "fast B>1", "fast splits>1"}


def test_pixel_gemm_cases_reach_every_kernel_variant():
    missing = PG_ROUTES - _pg_routes()
    assert not missing, sorted(missing)


@pytest.mark.parametrize("op", ["s2", "deconv1", "deconv2"])
def test_pixel_gemm_cases_reach_every_weight_gradient_regime(op):
    if op == "s2":
        seen = _wgrad_regimes(op, E.S2_CASES, R.s2_routes)
    else:
        st = int(op[-1])
        seen = _wgrad_regimes(op, [s for s in E.DECONV_CASES if s[5] == st], R.deconv_routes)
    want = set(WGRAD_REGIMES)
    if op != "deconv1":            # the row length matters only where a row of the walked map is a cursor step (s2, deconv s = 2)
        want |= {"fast Wo=32", "fast Wo=33"}
    missing = want - seen
    assert not missing, (op, sorted(missing))


def test_pixel_gemm_cases_reach_the_shape_edges():
    s2 = E.S2_CASES
    assert any(h // 2 == 1 for _, _, _, h, _ in s2) and any(w // 2 == 1 for _, _, _, _, w in s2)
    for st in (1, 2):
        dc = [s for s in E.DECONV_CASES if s[5] == st]
        assert any(s[3] == 1 for s in dc) and any(s[4] == 1 for s in dc), st
    chans = {c for s in s2 for c in s[1:3]} | {c for s in E.DECONV_CASES for c in s[1:3]}
    assert {1, 3, 33, 129} <= chans
    assert any(s[1] * 9 < R.PG_K for s in s2)                                           # stride-2 conv contraction below one stage
    assert any(s[1] < R.PG_K for s in E.DECONV_CASES)                                   # deconv forward contraction
    assert any(s[2] * s[5] ** 2 < R.PG_K for s in E.DECONV_CASES)                       # deconv data-gradient contraction
    # a gate-sized case whose native and split kernels differ (the bitwise-difference test uses the first case of each list)
    for routes, case in ((R.s2_routes, s2[0]), (R.deconv_routes, E.DECONV_CASES[0])):
        r = routes("native", *case)
        assert r["fwd"] == "native128" and r["dgrad"] == "native128" and r["pixels"] >= E.GATE_MIN_OUTPUTS
    # contractions shorter than one stage stay on the fp32 kernels under the split path: the 3-channel deblocks whose forward broke the
    # split path's error gate (1.9-2.1 x the fp32 kernel's rms) before pg_launch looked at the contraction
    for case in (E.DECONV_CASES[4], E.DECONV_CASES[11]):
        assert case[1] < R.PG_K and R.deconv_routes("split", *case)["fwd"] == "native64", case
    # the split-count switch: the large target reaches the 512 cap, the small one a single split
    for kind, s, target in E.SPLIT_TARGET_CASES:
        r = R.s2_routes("native", *s, target=target) if kind == "s2" else R.deconv_routes("native", *s, target=target)
        assert r["splits"] == (1 if target == 1 else R.PG_MAX_SPLITS), (kind, s, target)


def _wino_all():
    fwd = [R.wino_routes(*s, n_cu=R.N_CU) for s in E.WINO_CASES + E.NECK_SHAPES]
    dgd = [R.wino_routes(*s, direction="dgrad", n_cu=R.N_CU) for s in E.WINO_CASES + E.NECK_SHAPES]
    wgd = [R.wino_wgrad_routes(*s, n_cu=R.N_CU) for s in E.WINO_CASES + E.NECK_SHAPES]
    return fwd, dgd, wgd


def test_winograd_cases_reach_the_tile_edges():
    hs = {s[3] for s in E.WINO_CASES}
    ws = {s[4] for s in E.WINO_CASES}
    assert {1, 2, 3, 5} <= hs and {2, 4, 6} <= ws
    one_tile = [R.wino_routes(*s) for s in E.WINO_CASES if s[0] == 33 and R.wino_tiles(1, s[3], s[4]) == 1]
    assert one_tile and one_tile[0]["tile_blocks"] > 1 and one_tile[0]["last_block_tiles"] == 1


def test_winograd_cases_reach_the_stream_k_edges():
    fwd, dgd, wgd = _wino_all()
    both = fwd + dgd
    assert any(r["grid"] < R.N_CU for r in both)
    assert any(r["steps"] == R.N_CU and r["gang"] == 0 for r in both)
    assert any(R.N_CU < r["steps"] <= R.N_CU + 8 for r in both)
    assert any(r["steps_per_wg"] > 30 and r["steps_per_wg"] != int(r["steps_per_wg"]) for r in both)
    assert any(r["max_wg_per_unit"] >= 3 for r in both)
    assert {0, 1, 2, 4, 8, 16} <= {r["gang"] for r in both}, sorted({r["gang"] for r in both})
    assert any(32 % r["cout_blocks"] for r in both)                          # a channel-block count that does not divide 32
    # data gradient with the roles swapped: 32 produced channels from 512 or more contracted ones
    assert any(r["cout_blocks"] == 1 and r["chunks"] * R.WN_KC >= 512 for r in dgd)
    # weight gradient
    assert any(r["steps_per_unit"] == 1 for r in wgd)
    assert any(r["units"] > R.N_CU for r in wgd)
    assert any(r["grid"] < R.N_CU for r in wgd) and any(r["grid"] == R.N_CU for r in wgd)
    assert any(r["max_wg_per_unit"] >= 3 for r in wgd)


def test_winograd_neck_shapes_take_their_documented_split():
    f128 = R.wino_routes(*E.NECK_SHAPES[0])
    assert f128["units"] == 556 and f128["gang"] == 4 and 34 < f128["steps_per_wg"] < 36, f128
    assert R.wino_routes(*E.NECK_SHAPES[1])["gang"] == 2


def test_narrow_cases_reach_the_limits():
    cases = E.NARROW_CASES
    assert any(len(c) == R.NW_MAX_BRANCH and all(co == R.NW_CO for co in c) for *_, c in cases)
    assert any(len(c) == R.NW_MAX_BRANCH for *_, c in cases)
    assert {4, R.NW_MAX_W} <= {w for _, _, _, w, _ in cases}
    assert {1, 7, 9, 17} <= {h for _, _, h, _, _ in cases}
    assert {1, 3, 65} <= {cin for _, cin, _, _, _ in cases}
    assert any(R.narrow_bands(b, h) * R.NW_BAND != b * h for b, _, h, _, _ in cases)   # a last band of fewer than 8 rows
    unsup = E.NARROW_UNSUPPORTED
    assert any(w > R.NW_MAX_W for _, _, _, w, _ in unsup) and any(w % 4 for _, _, _, w, _ in unsup)
    assert any(co > R.NW_CO for *_, co in unsup)
