// Rotated BEV IoU and greedy NMS for gfx950 (needed by CenterHead decoding at
// eval time and by pseudo-label generation; reference pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu
// + the CPU sweep of iou3d_nms.cpp:100-135).
//
// One wave = 64 lanes = one 64-bit suppression word, so the pairwise pass maps 1:1 onto wave64:
// workgroup (cb, rb) of 64 threads compares 64 row boxes against the 64 column boxes staged in LDS
// and writes one u64 per row.  The greedy sweep, which the reference runs on the HOST after a
// blocking copy, stays on the device: a single wave walks the score-ordered boxes, keeps the
// "removed" bitset in LDS and ORs in the mask row of every survivor (coalesced 8-byte loads); the
// keep list and its length never leave the GPU, so decoding needs no synchronisation.
#include "common.h"
#include "rotated_overlap.cuh"

namespace toda {

__global__ void __launch_bounds__(256)
iou_matrix_kernel(const float* __restrict__ a, int na, const float* __restrict__ b, int nb, float* __restrict__ iou, int area_only) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)na * nb) return;
    const int i = (int)(t / nb), j = (int)(t % nb);
    float ba[7], bb[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        ba[k] = a[(size_t)i * 7 + k];
        bb[k] = b[(size_t)j * 7 + k];
    }
    iou[t] = area_only ? overlap_area(ba, bb) : iou_bev(ba, bb);
}

// mask[row * cb + col_block] bit j = IoU(row, col_block*64 + j) > thresh, for j after `row` only
__global__ void __launch_bounds__(64)
nms_mask_kernel(const float* __restrict__ boxes, int n, float thresh, unsigned long long* __restrict__ mask) {
    __shared__ float cols[64 * 7];
    const int cblk = blockIdx.x, rblk = blockIdx.y;
    const int ncol = min(64, n - cblk * 64);
    if (threadIdx.x < ncol)
        for (int k = 0; k < 7; ++k) cols[threadIdx.x * 7 + k] = boxes[(size_t)(cblk * 64 + threadIdx.x) * 7 + k];
    __syncthreads();
    const int row = rblk * 64 + threadIdx.x;
    if (row >= n) return;
    const int cb = (n + 63) / 64;
    unsigned long long word = 0;
    if (cblk >= rblk) {  // only later boxes can be suppressed by `row`
        float me[7];
        for (int k = 0; k < 7; ++k) me[k] = boxes[(size_t)row * 7 + k];
        const int first = cblk == rblk ? threadIdx.x + 1 : 0;
        for (int j = first; j < ncol; ++j)
            if (iou_bev(me, cols + j * 7) > thresh) word |= 1ull << j;
    }
    mask[(size_t)row * cb + cblk] = word;
}

// single wave: greedy sweep in score order; removed-set in LDS
__global__ void __launch_bounds__(64)
nms_sweep_kernel(const unsigned long long* __restrict__ mask, int n, long long* __restrict__ keep,
                 int* __restrict__ n_keep) {
    extern __shared__ unsigned long long removed[];
    const int cb = (n + 63) / 64, lane = threadIdx.x;
    for (int w = lane; w < cb; w += 64) removed[w] = 0ull;
    __builtin_amdgcn_wave_barrier();
    int kept = 0;
    for (int i = 0; i < n; ++i) {
        const unsigned long long word = removed[i >> 6];  // broadcast read
        if (word & (1ull << (i & 63))) continue;          // wave-uniform
        if (lane == 0) keep[kept] = i;
        ++kept;
        for (int w = (i >> 6) + lane; w < cb; w += 64) removed[w] |= mask[(size_t)i * cb + w];
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) *n_keep = kept;
}

}  // namespace toda

using namespace toda;

extern "C" int toda_boxes_iou_bev(const float* boxes_a, int na, const float* boxes_b, int nb, float* iou, void* stream) {
    TODA_CHECK_ARG(na >= 0 && nb >= 0, "boxes_iou_bev: negative size");
    if (na == 0 || nb == 0) return TODA_OK;
    hipLaunchKernelGGL(iou_matrix_kernel, dim3(cdiv((long long)na * nb, 256)), dim3(256), 0, (hipStream_t)stream, boxes_a, na,
                       boxes_b, nb, iou, 0);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_boxes_overlap_bev(const float* boxes_a, int na, const float* boxes_b, int nb, float* overlap, void* stream) {
    TODA_CHECK_ARG(na >= 0 && nb >= 0, "boxes_overlap_bev: negative size");
    if (na == 0 || nb == 0) return TODA_OK;
    hipLaunchKernelGGL(iou_matrix_kernel, dim3(cdiv((long long)na * nb, 256)), dim3(256), 0, (hipStream_t)stream, boxes_a, na,
                       boxes_b, nb, overlap, 1);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" size_t toda_nms_workspace_bytes(int n) {
    const size_t cb = (size_t)(n + 63) / 64;
    return align_up((size_t)(n > 0 ? n : 1) * (cb > 0 ? cb : 1) * sizeof(unsigned long long), 256);
}

extern "C" int toda_nms_rotated(const float* boxes_sorted, int n, float thresh, int64_t* keep, int32_t* n_keep_dev,
                                void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    TODA_CHECK_ARG(n >= 0, "nms_rotated: negative size");
    if (n == 0) {
        TODA_HIP(hipMemsetAsync(n_keep_dev, 0, sizeof(int32_t), s));
        return TODA_OK;
    }
    const int cb = (n + 63) / 64;
    TODA_CHECK_ARG((size_t)cb * 8 <= 64 * 1024, "nms_rotated: at most 524288 boxes");
    if (ws_bytes < toda_nms_workspace_bytes(n)) {
        set_error("nms_rotated: workspace %zu < required %zu", ws_bytes, toda_nms_workspace_bytes(n));
        return TODA_EWORKSPACE;
    }
    unsigned long long* mask = (unsigned long long*)ws;
    hipLaunchKernelGGL(nms_mask_kernel, dim3(cb, cb), dim3(64), 0, s, boxes_sorted, n, thresh, mask);
    hipLaunchKernelGGL(nms_sweep_kernel, dim3(1), dim3(64), cb * sizeof(unsigned long long), s, mask, n, (long long*)keep,
                       n_keep_dev);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
