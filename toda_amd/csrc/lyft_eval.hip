// The Lyft detection metric's two device parts (mAP over the IoU cut-offs 0.5 .. 0.95; reference
// pcdet/datasets/lyft/lyft_mAP_eval/lyft_eval.py get_average_precisions, which intersects one shapely polygon pair per
// (prediction, ground truth) inside a Python loop over every prediction).  Written from the definition in DESIGN.md 3.18.  All
// arithmetic is fp64 without contraction or integer; no atomics at all, so two runs give the same bits.  Every loop has a bound
// known before it starts.
//
// A box is a row of 8 doubles in the global frame: centre x y z, c, s, width, length, height.  (c, s) is the first column of the
// box's rotation, NOT normalised: under a tilted pose c^2 + s^2 < 1 and the ground rectangle
//     centre +- length / 2 (c, s) +- width / 2 (s, -c)
// shrinks by that norm while the volume stays width * length * height, as in the reference.  So this file has an intersection of
// its own (ly_iou), not waymo_eval.hip's we_iou, which moves one box into the other's frame with a unit (c, s).
//
// lyft_eval_best_kernel: one workgroup per (sample, class) segment, one wave per prediction at a time, the lanes over the
// segment's ground truths in steps of 64 (a segment has no size cap).  A lane keeps the first largest IoU of its ascending
// columns; wave_best picks the largest of the 64 with the lower index winning ties: numpy's max / argmax.
//
// lyft_eval_flags_kernel: one workgroup per segment.  Prediction q stands before p iff score_q > score_p, or the scores are equal
// and q is earlier (the reference's stable descending sort).  m_p is the largest best_iou_q over the q before p with p's argmax;
// tp[t, p] = best_iou_p > thr_t && !(m_p > thr_t): a ground truth is claimed at cut-off t exactly when an earlier prediction
// with that argmax exceeded t, which is the reference's sequential gt_checked walk.  Each lane owns one p of a tile of
// LY_FLAGS_BLOCK predictions and reads all q as (score, best_iou, best_gt) triples staged through LDS in chunks of LY_CHUNK.
#include <limits.h>
#include <math.h>

#include "eval_common.cuh"

namespace toda {

constexpr int LY_COLS = 8;
constexpr int LY_BEST_BLOCK = 256;
constexpr int LY_BEST_WAVES = LY_BEST_BLOCK / EVAL_WAVE;
constexpr int LY_FLAGS_BLOCK = 256;
constexpr int LY_CHUNK = 256;                          // triples of one LDS stage of the flags kernel
constexpr int LY_MAX_CUT = TODA_LYFT_MAX_CUTOFFS;      // 16

// the ground rectangle in the reference's corner order: counter-clockwise for every (c, s) != 0, since
// cross(p1 - p0, p2 - p1) = width * length * (c^2 + s^2)
__device__ __forceinline__ void ly_corners(const double* b, double (*p)[2]) {
    const double hl = b[6] / 2, hw = b[5] / 2, c = b[3], s = b[4];
    p[0][0] = (b[0] + hl * c) + hw * s, p[0][1] = (b[1] + hl * s) - hw * c;
    p[1][0] = (b[0] + hl * c) - hw * s, p[1][1] = (b[1] + hl * s) + hw * c;
    p[2][0] = (b[0] - hl * c) - hw * s, p[2][1] = (b[1] - hl * s) + hw * c;
    p[3][0] = (b[0] - hl * c) + hw * s, p[3][1] = (b[1] - hl * s) - hw * c;
}

// one Sutherland-Hodgman step: the part of the convex polygon `in` (at most 8 corners) on or left of the line a -> b
__device__ __forceinline__ int ly_clip(const double (*in)[2], int n, const double* a, const double* b, double (*out)[2]) {
    const double ex = b[0] - a[0], ey = b[1] - a[1];
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int k = i + 1 < n ? i + 1 : 0;
        const double dp = ex * (in[i][1] - a[1]) - ey * (in[i][0] - a[0]);
        const double dq = ex * (in[k][1] - a[1]) - ey * (in[k][0] - a[0]);
        const bool pin = dp >= 0.0, qin = dq >= 0.0;
        if (pin && m < 8) {
            out[m][0] = in[i][0];
            out[m][1] = in[i][1];
            ++m;
        }
        if (pin != qin && m < 8) {
            const double t = dp / (dp - dq);
            out[m][0] = in[i][0] + t * (in[k][0] - in[i][0]);
            out[m][1] = in[i][1] + t * (in[k][1] - in[i][1]);
            ++m;
        }
    }
    return m;
}

// Rectangles whose circumcircles are apart by more than a part in a thousand clip to nothing: the margin is far above the rounding of
// the corners, so no pair with area is cut off and the full route would return the same +0.  The radius carries the norm of (c, s).
__device__ __forceinline__ bool ly_apart(const double* a, const double* b) {
    const double ex = a[0] - b[0], ey = a[1] - b[1];
    const double ra = sqrt((a[5] * a[5] + a[6] * a[6]) * (a[3] * a[3] + a[4] * a[4])) / 2;
    const double rb = sqrt((b[5] * b[5] + b[6] * b[6]) * (b[3] * b[3] + b[4] * b[4])) / 2;
    return ex * ex + ey * ey > ((ra + rb) * (ra + rb)) * 1.002;
}

// IoU of prediction row a and ground-truth row b: a's rectangle clipped by b's four edges, shoelace area about the polygon's first
// corner (global coordinates are large, the differences are not), times the overlap of the z intervals
__device__ double ly_iou(const double* a, const double* b) {
    double p[8][2], q[8][2], g[4][2];
    ly_corners(a, p);
    ly_corners(b, g);
    int n = ly_clip(p, 4, g[0], g[1], q);
    n = ly_clip(q, n, g[1], g[2], p);
    n = ly_clip(p, n, g[2], g[3], q);
    n = ly_clip(q, n, g[3], g[0], p);
    double area = 0.0;
    if (n >= 3) {
        double acc = 0.0;
        for (int i = 1; i + 1 < n; ++i)
            acc += (p[i][0] - p[0][0]) * (p[i + 1][1] - p[0][1]) - (p[i + 1][0] - p[0][0]) * (p[i][1] - p[0][1]);
        area = fabs(acc) / 2;
    }
    const double zlo = fmax(a[2] - a[7] / 2, b[2] - b[7] / 2), zhi = fmin(a[2] + a[7] / 2, b[2] + b[7] / 2);
    const double inter = fmax(zhi - zlo, 0.0) * area;
    const double uni = ((a[5] * a[6]) * a[7] + (b[5] * b[6]) * b[7]) - inter;
    return fmin(fmax(inter / uni, 0.0), 1.0);
}

struct LyPick {
    double iou;
    int idx;
    __device__ LyPick across(int m) const { return {__shfl_xor(iou, m, EVAL_WAVE), __shfl_xor(idx, m, EVAL_WAVE)}; }
};

__device__ __forceinline__ bool ly_larger(const LyPick& a, const LyPick& b) { return a.iou > b.iou || (a.iou == b.iou && a.idx < b.idx); }

__global__ __launch_bounds__(LY_BEST_BLOCK) void lyft_eval_best_kernel(const double* __restrict__ pred, const double* __restrict__ gt,
                                                                       const int32_t* __restrict__ pred_off,
                                                                       const int32_t* __restrict__ gt_off, int n_pred, int n_gt,
                                                                       double* __restrict__ best_iou, int32_t* __restrict__ best_gt) {
    const int seg = blockIdx.x, wave = threadIdx.x / EVAL_WAVE, lane = threadIdx.x % EVAL_WAVE;
    // the launcher has checked the offsets on the host; a segment outside the buffers is left alone
    const auto [p0, np, g0, ng, inside] = seg_span(pred_off, gt_off, seg, n_pred, n_gt, INT_MAX, INT_MAX);
    if (!inside) return;
    for (int i = wave; i < np; i += LY_BEST_WAVES) {
        double a[LY_COLS];
        for (int k = 0; k < LY_COLS; ++k) a[k] = pred[(size_t)(p0 + i) * LY_COLS + k];
        LyPick best = {-HUGE_VAL, INT_MAX};
        for (int j = lane; j < ng; j += EVAL_WAVE) {            // columns ascend, so a lane's equal IoU keeps its lower index
            const double* b = gt + (size_t)(g0 + j) * LY_COLS;
            const double v = ly_apart(a, b) ? 0.0 : ly_iou(a, b);
            if (v > best.iou) {
                best.iou = v;
                best.idx = j;
            }
        }
        best = wave_best(best, ly_larger);
        if (lane == 0) {
            best_iou[p0 + i] = best.iou;
            best_gt[p0 + i] = best.idx == INT_MAX ? -1 : best.idx;
        }
    }
}

struct LyCuts {
    double thr[LY_MAX_CUT];
    int n;
};

__global__ __launch_bounds__(LY_FLAGS_BLOCK) void lyft_eval_flags_kernel(const double* __restrict__ score, const double* __restrict__ best_iou,
                                                                         const int32_t* __restrict__ best_gt,
                                                                         const int32_t* __restrict__ pred_off, int n_pred, LyCuts cuts,
                                                                         uint8_t* __restrict__ tp) {
    __shared__ double s_score[LY_CHUNK];
    __shared__ double s_iou[LY_CHUNK];
    __shared__ int s_gt[LY_CHUNK];
    const int seg = blockIdx.x, tid = threadIdx.x;
    const int p0 = pred_off[seg], np = pred_off[seg + 1] - p0;
    if (p0 < 0 || np < 0 || (long long)p0 + np > n_pred) return;   // uniform per workgroup, before any barrier
    for (int base = 0; base < np; base += LY_FLAGS_BLOCK) {
        const int p = base + tid;
        const bool mine = p < np;
        const double sp = mine ? score[p0 + p] : 0.0, bi = mine ? best_iou[p0 + p] : -HUGE_VAL;
        const int bg = mine ? best_gt[p0 + p] : -1;
        double m = -HUGE_VAL;
        for (int qb = 0; qb < np; qb += LY_CHUNK) {
            const int count = min(LY_CHUNK, np - qb);
            __syncthreads();                                    // the last chunk has been read by every lane
            for (int k = tid; k < count; k += LY_FLAGS_BLOCK) {
                s_score[k] = score[p0 + qb + k];
                s_iou[k] = best_iou[p0 + qb + k];
                s_gt[k] = best_gt[p0 + qb + k];
            }
            __syncthreads();
            if (!mine || bg < 0) continue;
            for (int k = 0; k < count; ++k) {
                const double sq = s_score[k];
                const bool before = sq > sp || (sq == sp && qb + k < p);
                if (before && s_gt[k] == bg) m = fmax(m, s_iou[k]);
            }
        }
        if (!mine) continue;
        for (int t = 0; t < cuts.n; ++t) tp[(size_t)t * n_pred + p0 + p] = (bi > cuts.thr[t] && !(m > cuts.thr[t])) ? 1 : 0;
    }
}

// ws: pred_off | gt_off
struct LyWs {
    WsCarver c;
    size_t pred_off, gt_off;
    explicit LyWs(int n_seg) : pred_off(c.take((size_t)(n_seg + 1) * sizeof(int32_t))), gt_off(c.take((size_t)(n_seg + 1) * sizeof(int32_t))) {}
};

}  // namespace toda

using namespace toda;

extern "C" int toda_lyft_eval_flags_chunk(void) { return LY_CHUNK; }

extern "C" size_t toda_lyft_eval_workspace_bytes(int n_seg) {
    if (n_seg < 1) return 0;
    return LyWs(n_seg).c.at;
}

extern "C" int toda_lyft_eval_best(const double* pred, int n_pred, const double* gt, int n_gt, const int32_t* pred_off_host,
                                   const int32_t* gt_off_host, int n_seg, double* best_iou, int32_t* best_gt, void* ws, size_t ws_bytes,
                                   void* stream) {
    TODA_CHECK_ARG(n_pred >= 0 && n_gt >= 0 && n_seg >= 0, "lyft_eval_best: negative size (n_pred %d, n_gt %d, n_seg %d)", n_pred, n_gt, n_seg);
    if (n_seg == 0) {
        TODA_CHECK_ARG(n_pred == 0 && n_gt == 0, "lyft_eval_best: %d predictions, %d ground truths but no segment", n_pred, n_gt);
        return TODA_OK;
    }
    TODA_CHECK_ARG(pred_off_host && gt_off_host, "lyft_eval_best: null offsets");
    if (csr_check("lyft_eval_best", pred_off_host, n_seg, n_pred, INT_MAX, "predictions") != TODA_OK) return TODA_EINVAL;
    if (csr_check("lyft_eval_best", gt_off_host, n_seg, n_gt, INT_MAX, "ground truths") != TODA_OK) return TODA_EINVAL;
    if (n_pred == 0) return TODA_OK;
    TODA_CHECK_ARG(pred && best_iou && best_gt && (gt || n_gt == 0), "lyft_eval_best: null boxes or output");
    const LyWs w(n_seg);
    TODA_CHECK_ARG(ws && ws_bytes >= w.c.at, "lyft_eval_best: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int32_t *pred_off, *gt_off;
    TODA_HIP(stage(ws, w.pred_off, pred_off_host, n_seg + 1, s, &pred_off));
    TODA_HIP(stage(ws, w.gt_off, gt_off_host, n_seg + 1, s, &gt_off));
    hipLaunchKernelGGL(lyft_eval_best_kernel, dim3(n_seg), dim3(LY_BEST_BLOCK), 0, s, pred, gt, pred_off, gt_off, n_pred, n_gt, best_iou, best_gt);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_lyft_eval_flags(const double* score, const double* best_iou, const int32_t* best_gt, int n_pred,
                                    const int32_t* pred_off_host, int n_seg, const double* thresholds_host, int n_thresholds, uint8_t* tp,
                                    void* ws, size_t ws_bytes, void* stream) {
    TODA_CHECK_ARG(n_pred >= 0 && n_seg >= 0, "lyft_eval_flags: negative size (n_pred %d, n_seg %d)", n_pred, n_seg);
    TODA_CHECK_ARG(n_thresholds >= 1 && n_thresholds <= LY_MAX_CUT, "lyft_eval_flags: %d cut-offs, supported are 1 to %d", n_thresholds, LY_MAX_CUT);
    TODA_CHECK_ARG(thresholds_host, "lyft_eval_flags: null cut-offs");
    LyCuts cuts = {};
    cuts.n = n_thresholds;
    for (int t = 0; t < n_thresholds; ++t) {
        TODA_CHECK_ARG(thresholds_host[t] == thresholds_host[t] && (t == 0 || thresholds_host[t] > thresholds_host[t - 1]),
                       "lyft_eval_flags: the cut-offs must ascend (entry %d)", t);
        cuts.thr[t] = thresholds_host[t];
    }
    if (n_seg == 0) {
        TODA_CHECK_ARG(n_pred == 0, "lyft_eval_flags: %d predictions but no segment", n_pred);
        return TODA_OK;
    }
    TODA_CHECK_ARG(pred_off_host, "lyft_eval_flags: null offsets");
    if (csr_check("lyft_eval_flags", pred_off_host, n_seg, n_pred, INT_MAX, "predictions") != TODA_OK) return TODA_EINVAL;
    if (n_pred == 0) return TODA_OK;
    TODA_CHECK_ARG(score && best_iou && best_gt && tp, "lyft_eval_flags: null scores, best IoU, best ground truth or output");
    const LyWs w(n_seg);
    TODA_CHECK_ARG(ws && ws_bytes >= w.c.at, "lyft_eval_flags: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int32_t* pred_off;
    TODA_HIP(stage(ws, w.pred_off, pred_off_host, n_seg + 1, s, &pred_off));
    hipLaunchKernelGGL(lyft_eval_flags_kernel, dim3(n_seg), dim3(LY_FLAGS_BLOCK), 0, s, score, best_iou, best_gt, pred_off, n_pred, cuts, tp);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
