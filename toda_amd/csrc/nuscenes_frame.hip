// Multi-sweep merge of a nuScenes sample for gfx950: the per-frame point pass of the reference's NuScenesDataset
// (nuscenes_dataset.py get_sweep / get_lidar_with_sweeps): the key frame and up to SWEEPS_MAX - 1 earlier sweeps, each with the
// ego vehicle's points flagged for removal, moved into the key frame by a 4 x 4 matrix and stamped with its time lag.
// One thread per raw row, blockIdx.y = sweep: the sweep's matrix, offsets and lag are uniform per workgroup and travel by
// value as kernel arguments - no table upload, no sync, no per-thread search.  No LDS, no atomics: 20 bytes in, 24 bytes out
// per row, so the kernel is bound by HBM traffic; the flags feed the stable compaction of points.hip (toda_rows_select_append).
//
// The 20-byte row pitch leaves a row base 4-byte aligned only, so rows are read and written as scalars: consecutive lanes
// cover consecutive rows, every cache line fetched or written is used in full.
//
// Arithmetic (-ffp-contract=off, no fused multiply-adds):
//   x' = (float)(((double)x * m00 + (double)y * m01 + (double)z * m02) + m03)      numpy's float64 dot assigned into fp32
//   x' += shift[0]                                                                  in fp32, after the rounding (SHIFT_COOR)
// The ego test reads the raw fp32 coordinates; a NaN compares false, so the row is kept, as in numpy.
//
// The ego cut is a rectangle of two half-sides: toda_sweeps_merge passes its radius for both (nuScenes' square),
// toda_sweeps_merge_rect passes them apart (Lyft's 1.5 m x 1.0 m, lyft_dataset.py remove_ego_points).  One kernel for both.
#include <string.h>

#include "common.h"
#include "points_common.cuh"

namespace toda {

constexpr int SWEEPS_MAX = 16;
constexpr int SWEEP_IN_COLS = 5;      // x y z intensity ring
constexpr int SWEEP_OUT_COLS = 5;     // x y z intensity time

struct SweepTable {
    double m[SWEEPS_MAX][12];          // [3][4] row-major per sweep
    int32_t offset[SWEEPS_MAX + 1];
    float lag[SWEEPS_MAX];
    uint32_t has_matrix, drop_ego;     // bit s = sweep s
    float radius_x, radius_y;          // half-sides of the ego rectangle
    int32_t has_shift;
    float shift[3];
};

__global__ void __launch_bounds__(PT_BLOCK)
sweeps_merge_kernel(const float* __restrict__ rows, SweepTable t, float* __restrict__ out, int32_t* __restrict__ flags) {
    const int s = blockIdx.y;
    const int begin = t.offset[s], count = t.offset[s + 1] - begin;
    const int k = pt_row(count, nullptr);
    if (k < 0) return;
    const size_t j = (size_t)begin + k;
    const float* p = rows + j * SWEEP_IN_COLS;
    float x = p[0], y = p[1], z = p[2];
    const float intensity = p[3];
    const bool ego = ((t.drop_ego >> s) & 1u) && fabsf(x) < t.radius_x && fabsf(y) < t.radius_y;
    if ((t.has_matrix >> s) & 1u) {
        const double* m = t.m[s];
        const double dx = x, dy = y, dz = z;
        x = (float)((dx * m[0] + dy * m[1] + dz * m[2]) + m[3]);
        y = (float)((dx * m[4] + dy * m[5] + dz * m[6]) + m[7]);
        z = (float)((dx * m[8] + dy * m[9] + dz * m[10]) + m[11]);
    }
    if (t.has_shift) x += t.shift[0], y += t.shift[1], z += t.shift[2];
    float* o = out + j * SWEEP_OUT_COLS;
    o[0] = x, o[1] = y, o[2] = z, o[3] = intensity, o[4] = t.lag[s];
    flags[j] = ego ? 0 : 1;
}

}  // namespace toda

using namespace toda;

extern "C" int toda_sweeps_merge_max_sweeps(void) { return SWEEPS_MAX; }

// the host side of both entry points; `who` names the caller in the messages
static int sweeps_merge_launch(const char* who, const float* rows, int n, int n_sweeps, const int32_t* offsets_host,
                               const double* matrices_host, const int32_t* has_matrix_host, const int32_t* drop_ego_host,
                               const double* time_lags_host, float radius_x, float radius_y, const float* shift_host, float* out,
                               int32_t* flags, void* stream) {
    PT_CHECK_TABLES(offsets_host && matrices_host && has_matrix_host && drop_ego_host && time_lags_host, "%s: null sweep table", who);
    TODA_CHECK_ARG(rows && out && flags, "%s: null rows, out or flags", who);
    TODA_CHECK_ARG(offsets_host[0] == 0 && offsets_host[n_sweeps] == n, "%s: row offsets must run from 0 to n = %d", who, n);
    SweepTable t;
    memset(&t, 0, sizeof(t));
    int longest = 0;
    for (int s = 0; s < n_sweeps; ++s) {
        const int count = offsets_host[s + 1] - offsets_host[s];
        TODA_CHECK_ARG(count >= 0, "%s: row offsets decrease at sweep %d", who, s);
        longest = count > longest ? count : longest;
        t.offset[s] = offsets_host[s];
        t.lag[s] = (float)time_lags_host[s];
        if (has_matrix_host[s]) {
            t.has_matrix |= 1u << s;
            for (int i = 0; i < 12; ++i) t.m[s][i] = matrices_host[s * 12 + i];
        }
        if (drop_ego_host[s]) t.drop_ego |= 1u << s;
    }
    t.offset[n_sweeps] = n;
    t.radius_x = radius_x;
    t.radius_y = radius_y;
    if (shift_host) {
        t.has_shift = 1;
        for (int i = 0; i < 3; ++i) t.shift[i] = shift_host[i];
    }
    hipLaunchKernelGGL(sweeps_merge_kernel, dim3(cdiv(longest, PT_BLOCK), n_sweeps), dim3(PT_BLOCK), 0, (hipStream_t)stream, rows, t, out, flags);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_sweeps_merge(const float* rows, int n, int n_sweeps, const int32_t* offsets_host, const double* matrices_host,
                                 const int32_t* has_matrix_host, const int32_t* drop_ego_host, const double* time_lags_host,
                                 float radius, const float* shift_host, float* out, int32_t* flags, void* stream) {
    TODA_CHECK_ARG(n >= 0, "sweeps_merge: need n >= 0");
    TODA_CHECK_ARG(n_sweeps >= 1 && n_sweeps <= SWEEPS_MAX, "sweeps_merge: %d sweeps, supported are 1 to %d (key frame included)", n_sweeps, SWEEPS_MAX);
    TODA_CHECK_ARG(radius >= 0.f, "sweeps_merge: the ego radius must be a number >= 0");
    return sweeps_merge_launch("sweeps_merge", rows, n, n_sweeps, offsets_host, matrices_host, has_matrix_host, drop_ego_host, time_lags_host,
                               radius, radius, shift_host, out, flags, stream);
}

extern "C" int toda_sweeps_merge_rect(const float* rows, int n, int n_sweeps, const int32_t* offsets_host, const double* matrices_host,
                                      const int32_t* has_matrix_host, const int32_t* drop_ego_host, const double* time_lags_host,
                                      float radius_x, float radius_y, const float* shift_host, float* out, int32_t* flags, void* stream) {
    TODA_CHECK_ARG(n >= 0, "sweeps_merge_rect: need n >= 0");
    TODA_CHECK_ARG(n_sweeps >= 1 && n_sweeps <= SWEEPS_MAX, "sweeps_merge_rect: %d sweeps, supported are 1 to %d (key frame included)", n_sweeps,
                   SWEEPS_MAX);
    TODA_CHECK_ARG(radius_x >= 0.f && radius_y >= 0.f, "sweeps_merge_rect: the ego half-sides must be numbers >= 0");
    return sweeps_merge_launch("sweeps_merge_rect", rows, n, n_sweeps, offsets_host, matrices_host, has_matrix_host, drop_ego_host,
                               time_lags_host, radius_x, radius_y, shift_host, out, flags, stream);
}
