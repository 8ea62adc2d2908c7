// Stable LSD radix sort of (int32 key, int32 val) pairs, 8 bits per pass: per-workgroup digit histograms (rs_hist), a device
// scan over them in digit-major order (scan.cuh), then a scatter that ranks equal digits in input order (rs_scatter); the host
// driver radix_sort_pairs runs the passes.  Two users: the dynamic voxel index (dynvox.hip) and the inverse neighbour table
// (voxel_pool.hip).  The kernels are static: every translation unit that includes this header has its own copy.  LDS integer atomics only.
#pragma once
#include "scan.cuh"

namespace toda {

constexpr int RS_BLOCK = 256;
constexpr int RS_ITEMS = 8;
constexpr int RS_TILE = RS_BLOCK * RS_ITEMS;      // elements per radix-sort workgroup
constexpr int RS_BINS = 256;

static __global__ void __launch_bounds__(RS_BLOCK)
rs_hist_kernel(const int32_t* __restrict__ key, int n, int shift, int nblk, int32_t* __restrict__ hist) {
    __shared__ int s_h[RS_BINS];
    s_h[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RS_ITEMS; ++j) {
        const int i = blockIdx.x * RS_TILE + j * RS_BLOCK + threadIdx.x;
        if (i < n) atomicAdd(&s_h[((unsigned)key[i] >> shift) & 255u], 1);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nblk + blockIdx.x] = s_h[threadIdx.x];     // digit-major: the scan gives digit, then block order
}

// element i of the tile goes to hist[digit][block] + (# earlier elements of the tile with that digit): rounds of 256 elements in
// index order; inside a round the wave peers of a digit (8 ballots) and the per-wave digit counts of the earlier waves.
static __global__ void __launch_bounds__(RS_BLOCK)
rs_scatter_kernel(const int32_t* __restrict__ key_in, const int32_t* __restrict__ val_in, int n, int shift, int nblk,
                  const int32_t* __restrict__ hist, int32_t* __restrict__ key_out, int32_t* __restrict__ val_out) {
    __shared__ int s_base[RS_BINS];
    __shared__ int s_wc[RS_BLOCK / 64][RS_BINS];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    s_base[t] = hist[(size_t)t * nblk + blockIdx.x];
#pragma unroll
    for (int k = 0; k < RS_BLOCK / 64; ++k) s_wc[k][t] = 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int j = 0; j < RS_ITEMS; ++j) {
        const int i = blockIdx.x * RS_TILE + j * RS_BLOCK + t;
        const bool valid = i < n;
        const int k = valid ? key_in[i] : 0;
        const int vv = valid ? val_in[i] : 0;
        const unsigned d = ((unsigned)k >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool on = (d >> b) & 1u;
            const unsigned long long bb = __ballot(valid && on);
            peers &= on ? bb : ~bb;
        }
        const int rank = __popcll(peers & below);
        if (valid && rank == 0) s_wc[w][d] = __popcll(peers);
        __syncthreads();
        if (valid) {
            int off = s_base[d] + rank;
            for (int q = 0; q < w; ++q) off += s_wc[q][d];
            key_out[off] = k;
            val_out[off] = vv;
        }
        __syncthreads();
        int add = 0;
#pragma unroll
        for (int q = 0; q < RS_BLOCK / 64; ++q) {
            add += s_wc[q][t];
            s_wc[q][t] = 0;
        }
        s_base[t] += add;
        __syncthreads();
    }
}

// workspace of one sort of up to n pairs, from byte `base` of the caller's buffer: the two ping-pong (key, val) pairs, the
// digit-major histogram and its scan partials, 256-byte aligned slots; `end` = the first byte after them
struct RsLayout {
    size_t ka, va, kb, vb, hist, hist_part, end;
};

static RsLayout rs_layout(long long n, size_t base) {
    RsLayout L;
    const int nblk = cdiv(n > 0 ? n : 1, RS_TILE);
    size_t o = base;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
    L.ka = take((size_t)n * 4);
    L.va = take((size_t)n * 4);
    L.kb = take((size_t)n * 4);
    L.vb = take((size_t)n * 4);
    L.hist = take((size_t)RS_BINS * nblk * 4);
    L.hist_part = take(scan_partials_bytes((long long)RS_BINS * nblk));
    L.end = o;
    return L;
}

// sorts the n pairs the caller wrote to (ka, va) of `ws` by key, keys in [0, bound): one hist -> scan -> scatter pass per 8 bits
// of bound - 1, ping-pong between the two pairs.  *keys / *vals (either may be NULL) = the pair that holds the result.
static int radix_sort_pairs(void* ws, const RsLayout& L, int n, long long bound, const int32_t** keys, const int32_t** vals,
                            hipStream_t s) {
    char* w = (char*)ws;
    int32_t *ka = (int32_t*)(w + L.ka), *va = (int32_t*)(w + L.va), *kb = (int32_t*)(w + L.kb), *vb = (int32_t*)(w + L.vb);
    int32_t* hist = (int32_t*)(w + L.hist);
    int bits = 1;
    while (bits < 31 && (1LL << bits) < bound) ++bits;
    const int nblk = cdiv(n, RS_TILE);
    for (int shift = 0; n > 0 && shift < bits; shift += 8) {
        hipLaunchKernelGGL(rs_hist_kernel, dim3(nblk), dim3(RS_BLOCK), 0, s, ka, n, shift, nblk, hist);
        TODA_LAUNCH_CHECK();
        int rc = exclusive_scan(PlainAccess{hist}, (long long)RS_BINS * nblk, (int32_t*)(w + L.hist_part), nullptr, s);
        if (rc) return rc;
        hipLaunchKernelGGL(rs_scatter_kernel, dim3(nblk), dim3(RS_BLOCK), 0, s, ka, va, n, shift, nblk, hist, kb, vb);
        TODA_LAUNCH_CHECK();
        int32_t* t = ka; ka = kb; kb = t;
        t = va; va = vb; vb = t;
    }
    if (keys) *keys = ka;
    if (vals) *vals = va;
    return TODA_OK;
}

}  // namespace toda
