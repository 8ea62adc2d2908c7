// What the point-table kernels of points.hip, points_local.hip, kitti_frame.hip, nuscenes_frame.hip and waymo_frame.hip share: the block size,
// the thread -> row map, the argument rule of their entry points, the generic row pass and range reduction (a new pass is a
// functor with its arithmetic and nothing else), and the point-in-box tests.
#pragma once
#include "common.h"

namespace toda {

constexpr int PT_BLOCK = 256;

// this thread's row of the table, or -1 past the valid rows min(n, *n_dev); n_dev == nullptr: past n
__device__ __forceinline__ int pt_row(int n, const int32_t* n_dev) {
    const int rows = eff_n(n, n_dev);
    const int j = blockIdx.x * PT_BLOCK + threadIdx.x;
    return j < rows ? j : -1;
}

// ---- the argument rule of every entry point: sizes first, then n == 0 is TODA_OK without a look at any pointer, then pointers
// (an entry point's further size checks stand between the two)
#define PT_CHECK_SIZES(name) TODA_CHECK_ARG(n >= 0 && c >= 3, "%s: need n >= 0 and at least 3 columns (x, y, z)", name)
#define PT_CHECK_TABLES(ok, ...)    \
    if (n == 0) return TODA_OK;     \
    TODA_CHECK_ARG(ok, __VA_ARGS__)

// ---- the generic row pass: one thread per valid row, f(j, row) holds the arithmetic; F travels by value as a kernel argument
template <class F>
__global__ void __launch_bounds__(PT_BLOCK)
pt_rows_kernel(const float* __restrict__ pts, int n, const int32_t* __restrict__ n_dev, int c, F f) {
    const int j = pt_row(n, n_dev);
    if (j < 0) return;
    f(j, pts + (size_t)j * c);
}

// the whole host side of a row pass: argument rule (tables_ok: the entry point's pointers), launch, launch check
template <class F>
static int pt_rows_pass(const char* name, const float* pts, int n, const int32_t* n_dev, int c, bool tables_ok, F f, void* stream) {
    PT_CHECK_SIZES(name);
    PT_CHECK_TABLES(pts && tables_ok, "%s: null table", name);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pt_rows_kernel<F>), dim3(cdiv(n, PT_BLOCK)), dim3(PT_BLOCK), 0, (hipStream_t)stream, pts, n, n_dev, c, f);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

// ---- min / max of a per-row value over the valid rows that have one: f(row, v) says whether the row counts and sets v.
// Per-workgroup partials (grid-stride per thread, wave butterfly, wave 0 over the LDS partials), then the same kernel with one
// workgroup folds them (partial_in != nullptr) - no atomics, nothing to initialise.  No such row: (+inf, -inf).  fminf / fmaxf
// skip a NaN where numpy's min / max hand it on.
constexpr int PT_RANGE_BLOCKS = 256;

static inline size_t pt_range_workspace_bytes() { return (size_t)PT_RANGE_BLOCKS * 2 * sizeof(float); }

template <class F>
__global__ void __launch_bounds__(PT_BLOCK)
pt_range_kernel(const float* __restrict__ pts, int n, const int32_t* __restrict__ n_dev, int c, F f,
                const float* __restrict__ partial_in, int n_partial, float* __restrict__ out) {
    __shared__ float smin[PT_BLOCK / 64], smax[PT_BLOCK / 64];
    float lo = INFINITY, hi = -INFINITY;
    if (partial_in) {                                       // second pass: fold the partials
        for (int i = threadIdx.x; i < n_partial; i += PT_BLOCK) {
            lo = fminf(lo, partial_in[2 * i]);
            hi = fmaxf(hi, partial_in[2 * i + 1]);
        }
    } else {
        const int rows = eff_n(n, n_dev);
        for (int j = blockIdx.x * PT_BLOCK + threadIdx.x; j < rows; j += gridDim.x * PT_BLOCK) {
            float v;
            if (f(pts + (size_t)j * c, v)) {
                lo = fminf(lo, v);
                hi = fmaxf(hi, v);
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d, 64));
        hi = fmaxf(hi, __shfl_xor(hi, d, 64));
    }
    if ((threadIdx.x & 63) == 0) smin[threadIdx.x >> 6] = lo, smax[threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PT_BLOCK / 64; ++w) lo = fminf(lo, smin[w]), hi = fmaxf(hi, smax[w]);
        out[2 * blockIdx.x] = lo;
        out[2 * blockIdx.x + 1] = hi;
    }
}

// the host side of a range reduction behind the entry point's size check: workspace, pointers, the two launches.  A reduction
// always has a result: n == 0 still writes (+inf, -inf), so only the table may be null then.
template <class F>
static int pt_range_pass(const char* name, const float* pts, int n, const int32_t* n_dev, int c, F f, float* range_dev, void* ws,
                         size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (ws_bytes < pt_range_workspace_bytes()) {
        set_error("%s: workspace %zu < required %zu", name, ws_bytes, pt_range_workspace_bytes());
        return TODA_EWORKSPACE;
    }
    TODA_CHECK_ARG((pts || n == 0) && range_dev && ws, "%s: null table, result or workspace", name);
    const int blocks = n > 0 ? (cdiv(n, PT_BLOCK) < PT_RANGE_BLOCKS ? cdiv(n, PT_BLOCK) : PT_RANGE_BLOCKS) : 1;
    float* partial = (float*)ws;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pt_range_kernel<F>), dim3(blocks), dim3(PT_BLOCK), 0, s, pts, n, n_dev, c, f, (const float*)nullptr, 0, partial);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pt_range_kernel<F>), dim3(1), dim3(PT_BLOCK), 0, s, pts, n, n_dev, c, f, (const float*)partial, blocks, range_dev);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

struct BoxPre {
    float cx, cy, cz, dx, dy, dz, cosa, sina;
};

// mode 0: roiaware_pool3d.cpp:121-141 (|z-cz| > dz/2 rejects, |local| < d/2 + 1e-2, fp64 compare)
// mode 1: augmentor_utils.py:474-491   (|z-cz| <= dz/2, |local| <= fp32(d/2 + 0.1))
// mode 2: roiaware_pool3d_kernel.cu:23-36 (as mode 0 with margin 1e-5 and fp32 cos / sin) - points_in_boxes_gpu
template <int MODE>
__device__ __forceinline__ bool point_in_box(float x, float y, float z, const BoxPre& b) {
    const float sz = z - b.cz;
    if (MODE == 0 || MODE == 2) {
        if ((double)fabsf(sz) > (double)b.dz / 2.0) return false;
    } else {
        if (!(fabsf(sz) <= b.dz / 2.0f)) return false;
    }
    const float sx = x - b.cx, sy = y - b.cy;
    const float lx = sx * b.cosa + sy * (-b.sina);
    const float ly = sx * b.sina + sy * b.cosa;
    if (MODE == 0 || MODE == 2) {
        const double m = MODE == 0 ? (double)1e-2f : (double)1e-5f;
        return fabs((double)lx) < (double)b.dx / 2.0 + m && fabs((double)ly) < (double)b.dy / 2.0 + m;
    }
    const float mx = b.dx / 2.0f + 0.1f, my = b.dy / 2.0f + 0.1f;
    return fabsf(lx) <= mx && fabsf(ly) <= my;
}

}  // namespace toda
