// SECONDHead's device side for gfx950 (reference pcdet/models/roi_heads/second_head.py:53-110 and
// roi_heads/target_assigner/proposal_target_layer.py:92-96, 194-228).
//
// toda_roi_grid_pool_bev: the rotated-RoI grid pool.  The reference builds one affine grid per sample (F.affine_grid,
// align_corners=False) and samples an expand()ed copy of the BEV map with F.grid_sample (bilinear, zero padding).  Here one
// launch covers the whole batch: workgroup (channel chunk, roi) first turns its roi into the 2x3 matrix and the G x G sampling
// positions (four tap offsets + four bilinear weights per cell, in LDS), then its lanes walk the chunk's output in memory order,
// cell fastest.  Lanes next to each other read the taps of neighbouring cells of ONE channel plane - a window of a few rows -
// and write consecutive floats of the [R, C, G, G] output.  Plain stores, no atomics: the result is bit-reproducible.
//
// toda_roi_iou3d_max: 3-D IoU (rotated BEV overlap x height overlap / union volume) of every roi against the valid gts of
// its sample, reduced to (max, argmax) in registers: one lane per roi, the sample's gts staged in LDS in tiles.  The number
// of valid gts (last non-zero row + 1, at least 1) is found on the device, so the sampler needs no per-class host syncs.
#include "common.h"
#include "rotated_overlap.cuh"

namespace toda {

constexpr int POOL_THREADS = 256;
constexpr int POOL_CHUNK = 32;          // channels per workgroup
constexpr int POOL_MAX_CELLS = 256;     // G <= 16

// grid (cdiv(C, POOL_CHUNK), R); R = B * N rois, roi r belongs to sample r / N
__global__ void __launch_bounds__(POOL_THREADS)
roi_grid_pool_kernel(const float* __restrict__ feat, int C, int H, int W, const float* __restrict__ rois, int N, int roi_stride,
                     float min_x, float min_y, float step_x, float step_y, int G, float* __restrict__ out) {
    __shared__ int s_off[POOL_MAX_CELLS][4];
    __shared__ float s_w[POOL_MAX_CELLS][4];
    const int r = blockIdx.y, b = r / N, cells = G * G, tid = threadIdx.x;
    if (tid < cells) {
        const float* roi = rois + (size_t)r * roi_stride;
        // the reference's 2 x 3 matrix, operation for operation (second_head.py:79-92), including its (x2 - x1) in the -sin term
        const float x1 = (roi[0] - roi[3] / 2 - min_x) / step_x, x2 = (roi[0] + roi[3] / 2 - min_x) / step_x;
        const float y1 = (roi[1] - roi[4] / 2 - min_y) / step_y, y2 = (roi[1] + roi[4] / 2 - min_y) / step_y;
        const float cosa = cosf(roi[6]), sina = sinf(roi[6]);
        const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
        const float a00 = (x2 - x1) / wm1 * cosa, a01 = (x2 - x1) / wm1 * (-sina), a02 = (x1 + x2 - (float)W + 1.f) / wm1;
        const float a10 = (y2 - y1) / hm1 * sina, a11 = (y2 - y1) / hm1 * cosa, a12 = (y1 + y2 - (float)H + 1.f) / hm1;
        // affine_grid's base grid (align_corners=False): cell centres of [-1, 1]
        const int i = tid / G, j = tid % G;
        const float u = (float)(2 * j + 1) / (float)G - 1.f, v = (float)(2 * i + 1) / (float)G - 1.f;
        const float gx = a00 * u + a01 * v + a02, gy = a10 * u + a11 * v + a12;
        // grid_sample's unnormalisation (align_corners=False) and bilinear corner weights
        const float px = ((gx + 1.f) * (float)W - 1.f) / 2.f, py = ((gy + 1.f) * (float)H - 1.f) / 2.f;
        const float fx = floorf(px), fy = floorf(py), fx1 = fx + 1.f, fy1 = fy + 1.f;
        const int x0 = (int)fx, y0 = (int)fy;
        const float w[4] = {(fx1 - px) * (fy1 - py), (px - fx) * (fy1 - py), (fx1 - px) * (py - fy), (px - fx) * (py - fy)};   // nw, ne, sw, se
        const int cx[4] = {x0, x0 + 1, x0, x0 + 1}, cy[4] = {y0, y0, y0 + 1, y0 + 1};
        const bool finite = fabsf(px) < 1e9f && fabsf(py) < 1e9f;                            // (int) of a huge float is undefined
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = finite && cx[k] >= 0 && cx[k] < W && cy[k] >= 0 && cy[k] < H;
            s_off[tid][k] = in ? cy[k] * W + cx[k] : -1;
            s_w[tid][k] = w[k];
        }
    }
    __syncthreads();
    const int c0 = blockIdx.x * POOL_CHUNK, nc = min(POOL_CHUNK, C - c0);
    const size_t plane = (size_t)H * W;
    const float* src = feat + ((size_t)b * C + c0) * plane;
    float* dst = out + ((size_t)r * C + c0) * cells;
    for (int e = tid; e < nc * cells; e += POOL_THREADS) {
        const int c = e / cells, cell = e - c * cells;
        const float* p = src + (size_t)c * plane;
        float acc = 0.f;                              // corner order and skip rule of grid_sample's bilinear path
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int o = s_off[cell][k];
            if (o >= 0) acc += __ldg(p + o) * s_w[cell][k];
        }
        dst[e] = acc;
    }
}

constexpr int IOU_THREADS = 256;
constexpr int IOU_TILE = 256;           // gts per LDS tile

__device__ __forceinline__ float iou3d(const float* a, const float* b) {
    const float a_hi = a[2] + a[5] / 2, a_lo = a[2] - a[5] / 2, b_hi = b[2] + b[5] / 2, b_lo = b[2] - b[5] / 2;
    const float h = fmaxf(fminf(a_hi, b_hi) - fmaxf(a_lo, b_lo), 0.f);
    const float inter = overlap_area(a, b) * h;
    const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
    return inter / fmaxf(va + vb - inter, 1e-6f);
}

// grid (cdiv(N, IOU_THREADS), B)
__global__ void __launch_bounds__(IOU_THREADS)
roi_iou3d_max_kernel(const float* __restrict__ rois, int N, int roi_stride, const int64_t* __restrict__ roi_labels,
                     const float* __restrict__ gt, int M, int gt_stride, int by_class, float* __restrict__ max_iou,
                     int64_t* __restrict__ argmax) {
    __shared__ float s_gt[IOU_TILE][8];
    __shared__ int s_last[IOU_THREADS / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* g = gt + (size_t)b * M * gt_stride;
    // valid gts: the last row whose sum is non-zero, + 1 (proposal_target_layer.py:92-96); a wave-max per wave, then over waves
    int last = -1;
    for (int j = tid; j < M; j += IOU_THREADS) {
        float s = 0.f;
        for (int k = 0; k < gt_stride; ++k) s += g[(size_t)j * gt_stride + k];
        if (s != 0.f) last = j;
    }
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o));
    if ((tid & 63) == 0) s_last[tid >> 6] = last;
    __syncthreads();
    last = s_last[0];
    for (int w = 1; w < IOU_THREADS / 64; ++w) last = max(last, s_last[w]);
    const int n_valid = max(last + 1, 1);             // an all-zero sample keeps one (zero) row, as the reference does

    const int i = blockIdx.x * IOU_THREADS + tid;
    const bool active = i < N;
    float roi[7];
    long long lab = 0;
    if (active) {
        for (int k = 0; k < 7; ++k) roi[k] = rois[((size_t)b * N + i) * roi_stride + k];
        lab = roi_labels ? roi_labels[(size_t)b * N + i] : 0;
    }
    float best = -1.f;                                // the first eligible gt wins even at IoU 0 (torch.max: lowest index)
    int best_j = 0;
    for (int t0 = 0; t0 < n_valid; t0 += IOU_TILE) {
        const int nt = min(IOU_TILE, n_valid - t0);
        __syncthreads();
        for (int e = tid; e < nt * 8; e += IOU_THREADS) {
            const int j = e >> 3, k = e & 7, row = t0 + j;
            // rows past M exist only for M == 0 (the zero filler row); column 7 holds the label (gt_stride - 1)
            float v = 0.f;
            if (row < M) v = k < 7 ? g[(size_t)row * gt_stride + k] : g[(size_t)row * gt_stride + gt_stride - 1];
            s_gt[j][k] = v;
        }
        __syncthreads();
        if (active) {
            for (int j = 0; j < nt; ++j) {
                if (by_class && (long long)s_gt[j][7] != lab) continue;
                const float v = iou3d(roi, s_gt[j]);
                if (v > best) {
                    best = v;
                    best_j = t0 + j;
                }
            }
        }
    }
    if (active) {
        max_iou[(size_t)b * N + i] = best < 0.f ? 0.f : best;
        argmax[(size_t)b * N + i] = best < 0.f ? 0 : best_j;
    }
}

}  // namespace toda

using namespace toda;

extern "C" int toda_roi_grid_pool_bev(const float* feat, int B, int C, int H, int W, const float* rois, int N, int roi_stride,
                                      float min_x, float min_y, float step_x, float step_y, int grid_size, float* out,
                                      void* stream) {
    TODA_CHECK_ARG(B >= 0 && N >= 0 && C >= 0, "roi_grid_pool_bev: negative size");
    TODA_CHECK_ARG(grid_size >= 1 && grid_size * grid_size <= POOL_MAX_CELLS, "roi_grid_pool_bev: grid size %d not in [1, 16]",
                   grid_size);
    TODA_CHECK_ARG(roi_stride >= 7, "roi_grid_pool_bev: rois need 7 columns, stride %d", roi_stride);
    TODA_CHECK_ARG(H > 1 && W > 1 && (long long)H * W < (1ll << 31), "roi_grid_pool_bev: map %d x %d not supported", H, W);
    TODA_CHECK_ARG(step_x > 0.f && step_y > 0.f, "roi_grid_pool_bev: non-positive cell size");
    TODA_CHECK_ARG((long long)B * N < 65536, "roi_grid_pool_bev: at most 65535 rois");
    if (B == 0 || N == 0 || C == 0) return TODA_OK;
    hipLaunchKernelGGL(roi_grid_pool_kernel, dim3(cdiv(C, POOL_CHUNK), B * N), dim3(POOL_THREADS), 0, (hipStream_t)stream, feat,
                       C, H, W, rois, N, roi_stride, min_x, min_y, step_x, step_y, grid_size, out);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_roi_iou3d_max(const float* rois, int B, int N, int roi_stride, const int64_t* roi_labels, const float* gt,
                                  int M, int gt_stride, int by_class, float* max_iou, int64_t* argmax, void* stream) {
    TODA_CHECK_ARG(B >= 0 && N >= 0 && M >= 0, "roi_iou3d_max: negative size");
    TODA_CHECK_ARG(roi_stride >= 7, "roi_iou3d_max: rois need 7 columns, stride %d", roi_stride);
    TODA_CHECK_ARG(gt_stride >= 8, "roi_iou3d_max: gt rows need 7 box columns + a label, stride %d", gt_stride);
    TODA_CHECK_ARG(!by_class || roi_labels != nullptr, "roi_iou3d_max: by_class needs roi labels");
    TODA_CHECK_ARG(B < 65536, "roi_iou3d_max: at most 65535 samples");
    if (B == 0 || N == 0) return TODA_OK;
    hipLaunchKernelGGL(roi_iou3d_max_kernel, dim3(cdiv(N, IOU_THREADS), B), dim3(IOU_THREADS), 0, (hipStream_t)stream, rois, N,
                       roi_stride, roi_labels, gt, M, gt_stride, by_class, max_iou, argmax);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
