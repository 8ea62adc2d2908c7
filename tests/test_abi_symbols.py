"""The C-ABI library loads on a GPU-less host and exports every symbol include/toda.h declares."""
import ctypes as C
import os
import re

import pytest

from toda_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "toda.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(toda_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_all_exported_and_bound():
    syms = declared_symbols()
    assert len(syms) >= 20
    lib = L.load()
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/toda.h but not exported"
        assert s in L.SIGNATURES, f"{s} has no ctypes prototype in toda_amd/lib.py"
    assert sorted(L.SIGNATURES) == syms
    assert lib.toda_abi_version() == 3


_vp, _i, _sz, _dbl, _f, _u, _ll = C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_float, C.c_uint, C.c_longlong

# written out by hand: one entry point per kind of declaration the header uses
EXPECTED = {
    "toda_last_error": (C.c_char_p, []),
    "toda_gridindex_bytes": (_sz, [_i, _vp]),
    "toda_bn2d_fwd": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _u, _vp]),
    "toda_conv3x3_narrow_fwd": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _ll, _vp, _vp]),
    "toda_points_sector": (_i, [_vp, _i, _vp, _i, _dbl, _dbl, _vp, _vp]),
    "toda_clip_adam_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _f, _f, _f, _f, _f, _f, _i, _vp]),
    "toda_conv3x3_transform_weight_batch": (_i, [_vp, _i, _vp]),
    "toda_anchor_assign": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "toda_anchor_assign_workspace_bytes": (_sz, [_i, _i]),
}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_prototypes_read_from_the_header(name):
    assert L.SIGNATURES[name] == EXPECTED[name]
    assert len(L.ARG_NAMES[name]) == len(EXPECTED[name][1])


def test_argument_names_and_limits_read_from_the_header():
    assert L.ARG_NAMES["toda_last_error"] == ()
    assert L.ARG_NAMES["toda_gridindex_bytes"] == ("batch", "shape_host")
    assert L.ARG_NAMES["toda_points_sector"] == ("points", "n", "n_dev", "c", "lo", "hi", "flags", "stream")
    assert set(L.ARG_NAMES) == set(L.SIGNATURES)
    limits = {"TODA_NUSC_MAX_PRED": 500, "TODA_NUSC_MAX_GT": 2048, "TODA_WAYMO_MAX_PRED": 512, "TODA_WAYMO_MAX_GT": 512,
              "TODA_WAYMO_CUTOFFS": 101, "TODA_LYFT_MAX_CUTOFFS": 16, "TODA_OK": 0, "TODA_EINVAL": -1, "TODA_FAULT_FPS": 4}
    assert {k: L.DEFINES[k] for k in limits} == limits
    assert "TODA_H_" not in L.DEFINES
    from toda_amd import ops
    assert (ops.NUSC_MAX_PRED, ops.NUSC_MAX_GT, ops.WAYMO_MAX_PRED, ops.WAYMO_MAX_GT, ops.WAYMO_CUTOFFS, ops.LYFT_MAX_CUTOFFS) == (500, 2048, 512, 512, 101, 16)


SYNTHETIC = """
/* toda_in_a_comment(int a); */
#ifndef X_H_
#define TODA_LIMIT 12   /* a limit */
#define TODA_NEGATIVE (-3)
#define TODA_BIT 4u
#define TODA_NOT_A_NUMBER (TODA_LIMIT + 1)
extern "C" {
typedef struct toda_entry { const float* w; int n; } toda_entry;
const char* toda_name(void);   // toda_in_a_line_comment(int a);
size_t toda_bytes(int batch, const int32_t* shape_host /*[3] D H W*/);
int toda_many(const float* const* rows_host, unsigned long long* cells, const toda_entry* entries,
              const int32_t shape[3], unsigned epoch, long long total,
              float eps, double lo, size_t ws_bytes, void* stream);
}
"""


def test_parser_on_a_synthetic_header():
    sig, names, defines = L.parse_header(SYNTHETIC)
    assert sig == {"toda_name": (C.c_char_p, []), "toda_bytes": (_sz, [_i, _vp]),
                   "toda_many": (_i, [_vp, _vp, _vp, _vp, _u, _ll, _f, _dbl, _sz, _vp])}
    assert names == {"toda_name": (), "toda_bytes": ("batch", "shape_host"),
                     "toda_many": ("rows_host", "cells", "entries", "shape", "epoch", "total", "eps", "lo", "ws_bytes", "stream")}
    assert defines == {"TODA_LIMIT": 12, "TODA_NEGATIVE": -3, "TODA_BIT": 4}


@pytest.mark.parametrize("decl, named", [
    ("int toda_short(short n);", "toda_short"),                          # a scalar type with no mapping
    ("int toda_wide(int n, int64_t total);", "toda_wide"),
    ("int32_t toda_ret(int n);", "toda_ret"),
    ("int toda_unnamed(int, int n);", "toda_unnamed"),
    ("int toda_callback(void (*done)(int), int n);", "toda_callback"),   # declarations the pattern does not cover
    ("TODA_API(int) toda_wrapped(int n);", "toda_wrapped"),
    ("int toda_twice(int n); int toda_twice(int n);", "3 times .* 2 prototypes"),      # counted with toda_fine
])
def test_parser_raises_on_what_it_does_not_understand(decl, named):
    with pytest.raises(RuntimeError, match=named):
        L.parse_header("int toda_fine(int n);\n" + decl)


def test_host_side_size_queries_need_no_gpu():
    lib = L.load()
    shape = L.host_i32([41, 1504, 1504])
    nbytes = lib.toda_gridindex_bytes(2, L.hptr(shape))
    cells = (2 * 41 * 1504 * 1504 + 31) // 32
    assert nbytes >= cells * 8
    assert lib.toda_spconv_packed_weight_floats(27, 16, 32) == 27 * 1 * 2 * 256          # fp32 fragment format only
    # a pair the split matrix path covers: the larger of the fp32 (4 B) and the three-plane bf16 (6 B per weight) formats
    assert lib.toda_spconv_packed_weight_floats(27, 64, 64) == 27 * 64 * 64 * 6 // 4
    assert lib.toda_spconv_split_supported(64, 64) == 1 and lib.toda_spconv_split_supported(16, 16) == 0
    assert lib.toda_matrix_path() in (0, 1) and lib.toda_set_matrix_path(7) != 0
    assert lib.toda_spconv_packed_weight_floats(27, 5, 16) == 27 * 256
    assert lib.toda_voxelize_workspace_bytes(180000, 150000) > 180000 * 4 * 5


def test_bad_arguments_fail_loudly_without_touching_the_device():
    lib = L.load()
    rc = lib.toda_spconv_gather_gemm(None, 0, 200, None, None, 0, 27, 16, None, None, None)
    assert rc == -1 and b"channels" in lib.toda_last_error()


def test_more_argument_checks_and_size_queries():
    """Every entry point validates before it launches: error code + message, nothing dereferenced."""
    import ctypes
    lib = L.load()
    assert lib.toda_spconv_wgrad(None, 10, None, None, 10, 27, 64, 200, None, None, 0, None) == -1 and b"channels" in lib.toda_last_error()
    need = lib.toda_spconv_wgrad_workspace_bytes(100000, 27, 64, 64)
    assert need >= 27 * 64 * 64 * 4
    assert lib.toda_spconv_wgrad(None, 10, None, None, 100000, 27, 64, 64, None, None, need - 1, None) != 0 and b"workspace" in lib.toda_last_error()
    assert lib.toda_nms_workspace_bytes(1000) >= 1000 * 16 * 8
    assert lib.toda_nms_rotated(None, 1000, 0.5, None, None, None, 8, None) != 0 and b"workspace" in lib.toda_last_error()
    assert lib.toda_rows_select_workspace_bytes(100000) >= 100000 * 4
    assert lib.toda_rows_select_append(None, 1000, None, 4, None, 1, 0, None, 10, None, None, 16, None) != 0 and b"workspace" in lib.toda_last_error()
    assert lib.toda_rows_moments(None, 10, 24, None, None) == -1 and b"channels" in lib.toda_last_error()           # 24 does not divide 256
    assert lib.toda_rows_reduce_doubles(389533, 64) >= 2 * 64 * 2
    edges = (ctypes.c_double * 40)()
    ep = ctypes.cast(edges, ctypes.c_void_p)
    assert lib.toda_points_polar_cell(None, 10, None, 4, 0.0, ep, 33, ep, 2, 0.0, 1.0, None, None) == -1 and b"bins" in lib.toda_last_error()
    assert lib.toda_points_in_boxes(None, 10, None, 4, None, 3, 7, 5, None, None) == -1 and b"mode" in lib.toda_last_error()
    assert lib.toda_points_in_boxes(None, 10, None, 2, None, 3, 7, 0, None, None) == -1                              # needs x, y, z
    assert lib.toda_timing_begin(0) == -1
    # zero-sized problems succeed without touching any pointer
    assert lib.toda_spconv_gather_gemm_ordered(None, 0, 64, None, None, 0, 27, 64, None, None, None, None) == 0
    assert lib.toda_points_sector(None, 0, None, 4, 0.0, 1.0, None, None) == 0
    assert lib.toda_boxes_overlap_bev(None, 0, None, 5, None, None) == 0


def test_host_tensors_are_refused():
    import pytest
    import torch
    from toda_amd import ops

    with pytest.raises(RuntimeError):
        ops.mean_vfe(torch.zeros(2, 3, 4), torch.ones(2))


def test_round3_entry_points_validate_before_they_launch():
    """The entry points added in round 3 (compacting gather-GEMM, slice BatchNorm2d, optimizer step):
    support queries, workspace sizes, argument errors - no GPU needed."""
    lib = L.load()
    assert lib.toda_spconv_gather_gemm_compact_supported(16, 16, 27) == 1 and lib.toda_spconv_gather_gemm_compact_supported(5, 16, 27) == 1
    assert lib.toda_spconv_gather_gemm_compact_supported(64, 16, 27) == 0 and lib.toda_spconv_gather_gemm_compact_supported(16, 16, 3) == 0
    assert lib.toda_spconv_gather_gemm_compact_supported(16, 18, 27) == 0                                   # produced channels: a multiple of 4
    assert lib.toda_spconv_gather_gemm_compact(None, 10, 64, None, 16, 64, 0, 0, None, 10, 27, 16, None, None, None) == -1 and b"K = 27" in lib.toda_last_error()
    assert lib.toda_spconv_gather_gemm_compact(None, 10, 16, None, 32, 16, 1, 0, None, 10, 27, 16, None, None, None) == -1 and b"does not map" in lib.toda_last_error()
    assert lib.toda_spconv_gather_gemm_compact(None, 10, 16, None, 16, 16, 0, 0, None, 0, 27, 16, None, None, None) == 0       # no output rows: nothing to do
    one = L.host_f32([0.0])
    p = L.hptr(one)
    assert lib.toda_bn2d_fwd_into(p, 2, 64, 100, p, p, None, None, 0.01, 1e-3, 1, p, 96, 40, p, None, 0, None) == -1 and b"outside" in lib.toda_last_error()
    assert lib.toda_bn2d_bwd_from(p, p, 96, 40, 2, 64, 100, p, p, p, 1, p, p, p, None, 0, None) == -1 and b"outside" in lib.toda_last_error()
    assert lib.toda_clip_adam_chunk() == 8192
    assert lib.toda_clip_adam_step(None, None, None, None, None, None, None, 4, None, None, 10.0, 1e-3, 0.9, 0.99, 1e-8, 0.01, 1, None) == -1 and b"null" in lib.toda_last_error()
    assert lib.toda_clip_adam_step(p, p, p, p, p, p, p, 4, p, p, 10.0, 1e-3, 0.9, 0.99, 1e-8, 0.01, 0, None) == -1 and b"step" in lib.toda_last_error()
    assert lib.toda_clip_adam_step(p, p, p, p, p, p, p, 0, p, p, 10.0, 1e-3, 0.9, 0.99, 1e-8, 0.01, 1, None) == 0             # no tensors: nothing to do
