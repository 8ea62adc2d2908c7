// What kitti_eval.hip, nuscenes_eval.hip, waymo_eval.hip and lyft_eval.hip share: the lexicographic pick and the sum over a wave, the counting rank
// by score into LDS, a segment's span with its guard, the run-then-tree fold, and on the host the CSR check, the workspace carver
// and the copy of a host table into its slot.  The intersections (ev_rect_inter, we_iou, ly_iou, the centre distance) are NOT here:
// each is pinned to its own metric's definition.  Everything is inline or static: every translation unit that
// includes this header compiles its own copy.
#pragma once
#include "common.h"

namespace toda {

constexpr int EVAL_WAVE = 64;

// The first of the wave's 64 picks in the order `before`, a strict total order whose last key is the index: the lower index wins
// ties and every lane returns the same pick.  A pick struct says itself how it travels: across(m) is its copy from lane ^ m, field by
// field (so no padding is moved and no double is split).
template <class Pick, class Before>
__device__ __forceinline__ Pick wave_best(Pick p, Before before) {
#pragma unroll
    for (int m = EVAL_WAVE / 2; m >= 1; m >>= 1) {
        const Pick o = p.across(m);
        if (before(o, p)) p = o;
    }
    return p;
}

template <class T>   // sum over the wave by the same tree in every lane, m = 32 .. 1
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = EVAL_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, EVAL_WAVE);
    return v;
}

// s_order[rank] = i for the n scores in LDS by score descending, equal scores the later position first (LATER_FIRST) or the earlier.
// Needs a TOTAL order, so no NaN: then every rank is written exactly once, without atomics.  The barriers are the caller's.
template <bool LATER_FIRST, class S>
__device__ __forceinline__ void rank_by_score(const S* s_score, int* s_order, int n, int tid, int nthreads) {
    for (int i = tid; i < n; i += nthreads) {
        const S si = s_score[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const S sj = s_score[j];
            rank += (sj > si || (sj == si && (LATER_FIRST ? j > i : j < i))) ? 1 : 0;
        }
        s_order[rank] = i;
    }
}

// Predictions [p0, p0 + np) and ground truths [g0, g0 + ng) of segment `seg` of the two CSR arrays; `inside` is false when it leaves
// the buffers or exceeds a cap (the caller's LDS arrays).  The launchers check the offsets on the host; this stands between a bad
// offset and a write out of bounds.  An empty side is inside: what an empty or a refused segment means is the caller's business.
struct SegSpan {
    int p0, np, g0, ng;
    bool inside;
};
__device__ __forceinline__ SegSpan seg_span(const int32_t* pred_off, const int32_t* gt_off, int seg, int n_pred, int n_gt, int cap_pred,
                                            int cap_gt) {
    const int p0 = pred_off[seg], np = pred_off[seg + 1] - p0, g0 = gt_off[seg], ng = gt_off[seg + 1] - g0;
    return {p0, np, g0, ng, np >= 0 && np <= cap_pred && ng >= 0 && ng <= cap_gt && p0 >= 0 && g0 >= 0 && p0 + np <= n_pred && g0 + ng <= n_gt};
}

// load(0) + .. + load(n - 1) by BLOCK lanes in one fixed order: lane k adds its contiguous run of cdiv(n, BLOCK) terms ascending, then
// a halving tree over s[BLOCK] in LDS.  Not bn_fold.cuh's fold_column, which strides the lanes over the terms: other last bits in fp64.
template <class T, int BLOCK, class Load>
__device__ __forceinline__ T fold_runs(int n, Load load, T* s) {
    const int run = (n + BLOCK - 1) / BLOCK, lo = threadIdx.x * run, hi = min(lo + run, n);
    T acc = 0;
    for (int i = lo; i < hi; ++i) acc += load(i);
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int m = BLOCK / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) s[threadIdx.x] += s[threadIdx.x + m];
        __syncthreads();
    }
    return s[0];
}

// ---- host: one CSR array, read before anything is launched.  It runs from 0 to n_total, never descends, and no segment holds more
// than `cap` of `what` ("predictions", "ground truths").
static int csr_check(const char* who, const int32_t* off, int n_seg, int n_total, int cap, const char* what) {
    TODA_CHECK_ARG(off[0] == 0 && off[n_seg] == n_total, "%s: the offsets of the %s must run from 0 to %d", who, what, n_total);
    for (int s = 0; s < n_seg; ++s) {
        TODA_CHECK_ARG(off[s + 1] >= off[s], "%s: the offsets of the %s descend at segment %d", who, what, s);
        TODA_CHECK_ARG(off[s + 1] - off[s] <= cap, "%s: segment %d has %d %s, at most %d fit one segment", who, s, off[s + 1] - off[s], what, cap);
    }
    return TODA_OK;
}

// a workspace as 256-byte slots in take() order; an export's size and its launchers' layout come from one struct built on this
struct WsCarver {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t here = at; at += align_up(bytes, 256); return here; }
};

// a host table of `count` entries into its slot of the workspace, on the stream of the launch that reads it; *dev points at the slot
template <class T>
static inline hipError_t stage(void* ws, size_t slot, const T* host, size_t count, hipStream_t stream, const T** dev) {
    *dev = (const T*)((char*)ws + slot);
    return hipMemcpyAsync((char*)ws + slot, host, count * sizeof(T), hipMemcpyHostToDevice, stream);
}

}  // namespace toda
