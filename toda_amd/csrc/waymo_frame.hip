// Per-frame point pass of a processed Waymo frame for gfx950: the reference's WaymoDataset.get_lidar (waymo_dataset.py:159-167,
// repeated in mix_dataset/waymo_nus_*_dataset.py): drop the rows inside a no-label zone (NLZ flag != -1), keep x, y, z and the
// elongation, squash the intensity with tanh.  One thread per row; consecutive lanes cover consecutive rows, so every cache line
// fetched or written is used in full.  No LDS, no atomics: 4 c_in bytes in (the kernel reads five or six of the columns, the
// lines come whole), 20 + 4 bytes out per row, so the kernel is bound by HBM traffic, or by launch latency at one frame's
// 180 k rows; the flags feed the stable compaction of points.hip (toda_rows_select_append).
//
// The 24-byte input pitch (c_in = 6) and the 20-byte output pitch leave a row base 8- or 4-byte aligned only, and c_in is a
// run-time value, so rows are read and written as scalars.
//
// Arithmetic: intensity' = (float)tanh((double)intensity) - the fp64 routine, rounded once: the correctly rounded fp32 value
// that numpy's fp32 tanh approximates to 1 ulp.  It keeps the sign of zero, passes NaN and saturates to +-1.  Nothing else of
// the row is computed.  The NLZ test is the fp32 equality row[5] == -1.0f: a NaN or a neighbour of -1 drops the row, as numpy's
// NLZ_flag == -1 does.
#include <math.h>

#include "common.h"
#include "points_common.cuh"

namespace toda {

constexpr int WAYMO_IN_COLS_MIN = 6;    // x y z intensity elongation NLZ
constexpr int WAYMO_OUT_COLS = 5;       // x y z tanh(intensity) elongation

__global__ void __launch_bounds__(PT_BLOCK)
waymo_frame_kernel(const float* __restrict__ rows, int n, int c_in, int use_nlz, float* __restrict__ out, int32_t* __restrict__ flags) {
    const int j = pt_row(n, nullptr);
    if (j < 0) return;
    const float* p = rows + (size_t)j * c_in;
    const float x = p[0], y = p[1], z = p[2], intensity = p[3], elongation = p[4];
    const int keep = use_nlz ? (p[5] == -1.0f ? 1 : 0) : 1;
    float* o = out + (size_t)j * WAYMO_OUT_COLS;
    o[0] = x, o[1] = y, o[2] = z, o[3] = (float)tanh((double)intensity), o[4] = elongation;
    flags[j] = keep;
}

}  // namespace toda

using namespace toda;

extern "C" int toda_waymo_frame(const float* rows, int n, int c_in, int use_nlz, float* out, int32_t* flags, void* stream) {
    TODA_CHECK_ARG(n >= 0, "waymo_frame: need n >= 0");
    TODA_CHECK_ARG(c_in >= WAYMO_IN_COLS_MIN, "waymo_frame: %d columns, a processed frame has at least %d (x, y, z, intensity, elongation, NLZ flag)",
                   c_in, WAYMO_IN_COLS_MIN);
    PT_CHECK_TABLES(rows && out && flags, "waymo_frame: null rows, out or flags");
    hipLaunchKernelGGL(waymo_frame_kernel, dim3(cdiv(n, PT_BLOCK)), dim3(PT_BLOCK), 0, (hipStream_t)stream, rows, n, c_in, use_nlz, out, flags);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
