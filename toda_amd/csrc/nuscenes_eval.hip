// The nuScenes detection metric's two device parts (public definition `detection_cvpr_2019`; the reference hands the whole metric
// to the nuScenes devkit, a Python loop over every prediction and every ground truth).  All arithmetic is fp64 without
// contraction; no atomics, so two runs give the same bits.
//
// nusc_eval_prepare_kernel: one lane per box, predictions and ground truths alike.  A LiDAR-frame row goes to the global frame
// through its sample's G = inv(car_from_global) . inv(ref_from_car): centre G (x y z 1), yaw atan2 of the xy part of
// R (cos h, sin h, 0), velocity xy of R v, and the keep flag `ego distance < range of the class` (strict).
//
// nusc_eval_match_kernel: one workgroup per (sample, class) segment, one wavefront per distance threshold.  The block ranks the
// segment's predictions by (score descending, index descending) in LDS: with at most NUSC_MAX_PRED of them a counting rank (one
// pass over all scores per prediction) is cheaper than a sort.  Each wave then walks the predictions in that order.  Lane l owns
// ground truths l, l + 64, ... and keeps their taken bits in one 32-bit register, hence NUSC_MAX_GT = 64 * 32 = 2048 ground
// truths per segment.  The nearest free ground truth is the lexicographic minimum of (distance, index) over the wave: six
// shuffle steps.  It is a match iff the distance is strictly below the threshold; otherwise the prediction takes nothing.  The wave
// of the true-positive threshold also writes each match's five errors.  Rank, minimum and segment guard are eval_common.cuh's.
#include "eval_common.cuh"

namespace toda {

constexpr int NE_BLOCK = 256;
constexpr int NE_THRESH = NE_BLOCK / EVAL_WAVE;          // 4 thresholds: one wave each
constexpr int NE_MAX_PRED = TODA_NUSC_MAX_PRED;        // 500
constexpr int NE_MAX_GT = TODA_NUSC_MAX_GT;            // 2048
constexpr int NE_SLOTS = NE_MAX_GT / EVAL_WAVE;          // 32: the bits of a lane's taken mask
constexpr int NE_CLASSES = 10;
constexpr int NE_BARRIER = 9;
constexpr int NE_ROW = 10;                             // prepare input: x y z dx dy dz heading vx vy vz
constexpr int NE_OUT = 6;                              // prepare output: cx cy cz yaw vx vy
constexpr int NE_BOX = 8;                              // match input: cx cy yaw vx vy dx dy dz
constexpr double NE_PI = 3.14159265358979323846;
static_assert(NE_SLOTS == 32, "a lane's taken bits must fit its 32-bit mask");

// class order of TODA_NUSC_CLASSES: car truck bus trailer construction_vehicle | pedestrian motorcycle bicycle | traffic_cone barrier
__device__ __forceinline__ double ne_class_range(int cls) { return cls < 5 ? 50.0 : cls < 8 ? 40.0 : 30.0; }

__global__ __launch_bounds__(NE_BLOCK) void nusc_eval_prepare_kernel(const double* __restrict__ rows, const int32_t* __restrict__ sample,
                                                                      const int32_t* __restrict__ cls, const double* __restrict__ G,
                                                                      const double* __restrict__ ego, int n, int n_samples,
                                                                      double* __restrict__ out, int32_t* __restrict__ keep) {
    const int i = blockIdx.x * NE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int s = sample[i], c = cls[i];
    double* o = out + (size_t)i * NE_OUT;
    if (s < 0 || s >= n_samples) {                      // a row without a sample takes no part and reads no matrix
        for (int k = 0; k < NE_OUT; ++k) o[k] = nan("");
        keep[i] = 0;
        return;
    }
    const double* r = rows + (size_t)i * NE_ROW;
    const double* g = G + (size_t)s * 12;
    const double* e = ego + (size_t)s * 3;
    const double x = r[0], y = r[1], z = r[2];
    const double cx = ((g[0] * x + g[1] * y) + g[2] * z) + g[3];
    const double cy = ((g[4] * x + g[5] * y) + g[6] * z) + g[7];
    const double cz = ((g[8] * x + g[9] * y) + g[10] * z) + g[11];
    const double ch = cos(r[6]), sh = sin(r[6]);
    const double vx = r[7], vy = r[8], vz = r[9];
    o[0] = cx;
    o[1] = cy;
    o[2] = cz;
    o[3] = atan2(g[4] * ch + g[5] * sh, g[0] * ch + g[1] * sh);
    o[4] = (g[0] * vx + g[1] * vy) + g[2] * vz;
    o[5] = (g[4] * vx + g[5] * vy) + g[6] * vz;
    const double ex = cx - e[0], ey = cy - e[1];
    keep[i] = (c >= 0 && c < NE_CLASSES && sqrt(ex * ex + ey * ey) < ne_class_range(c)) ? 1 : 0;
}

struct NePick {
    double d;
    int idx;
    __device__ NePick across(int m) const { return {__shfl_xor(d, m, EVAL_WAVE), __shfl_xor(idx, m, EVAL_WAVE)}; }
};

__device__ __forceinline__ bool ne_nearer(const NePick& a, const NePick& b) { return a.d < b.d || (a.d == b.d && a.idx < b.idx); }

// floored remainder x mod p for p > 0
__device__ __forceinline__ double ne_mod(double x, double p) {
    double m = fmod(x, p);
    if (m < 0) m += p;
    return m;
}

struct NeMatch {
    const double* pred;          // [n_pred, NE_BOX], segment after segment
    const double* score;         // [n_pred]
    const int32_t* pred_attr;    // [n_pred], -1 none
    const double* gt;            // [n_gt, NE_BOX]
    const int32_t* gt_attr;      // [n_gt], -1 none
    const int32_t* pred_off;     // [n_seg + 1]
    const int32_t* gt_off;       // [n_seg + 1]
    const int32_t* seg_cls;      // [n_seg]
    int n_pred, n_gt, tp_wave;
    double thresh[NE_THRESH];
};

__global__ __launch_bounds__(NE_BLOCK) void nusc_eval_match_kernel(NeMatch p, int32_t* __restrict__ match, double* __restrict__ err) {
    __shared__ double s_score[NE_MAX_PRED];
    __shared__ double s_xy[NE_MAX_PRED][2];
    __shared__ int s_order[NE_MAX_PRED];
    const int seg = blockIdx.x;
    // the launcher has checked the offsets on the host; a segment outside the buffers or the LDS arrays is left alone
    const auto [p0, np, g0, ng, inside] = seg_span(p.pred_off, p.gt_off, seg, p.n_pred, p.n_gt, NE_MAX_PRED, NE_MAX_GT);
    if (!inside || np <= 0) return;
    for (int i = threadIdx.x; i < np; i += NE_BLOCK) {
        s_score[i] = p.score[p0 + i];
        s_xy[i][0] = p.pred[(size_t)(p0 + i) * NE_BOX];
        s_xy[i][1] = p.pred[(size_t)(p0 + i) * NE_BOX + 1];
        s_order[i] = -1;
    }
    __syncthreads();
    rank_by_score<true>(s_score, s_order, np, threadIdx.x, NE_BLOCK);     // equal scores: the later position first; the host refuses
    __syncthreads();                                                      // non-finite scores, so the order is total

    const int lane = threadIdx.x & (EVAL_WAVE - 1), wave = threadIdx.x / EVAL_WAVE;
    const double thresh = p.thresh[wave];
    const bool write_err = wave == p.tp_wave;
    const double period = p.seg_cls[seg] == NE_BARRIER ? NE_PI : 2 * NE_PI;
    const double* gt = p.gt + (size_t)g0 * NE_BOX;
    const int slots = (ng + EVAL_WAVE - 1) / EVAL_WAVE;
    // the first slot (every ground truth of a segment with at most 64 of them) stays in registers
    const double gx0 = lane < ng ? gt[(size_t)lane * NE_BOX] : 0.0, gy0 = lane < ng ? gt[(size_t)lane * NE_BOX + 1] : 0.0;
    int32_t* out = match + (size_t)wave * p.n_pred + p0;
    unsigned taken = 0;
    for (int r = 0; r < np; ++r) {
        const int i = s_order[r];
        if (i < 0) continue;                            // only with a NaN score, which the host refuses
        const double px = s_xy[i][0], py = s_xy[i][1];
        NePick best = {HUGE_VAL, 0x7fffffff};
        for (int k = 0; k < slots; ++k) {
            const int g = k * EVAL_WAVE + lane;
            if (g >= ng || (taken >> k & 1u)) continue;
            const double dx = (k == 0 ? gx0 : gt[(size_t)g * NE_BOX]) - px, dy = (k == 0 ? gy0 : gt[(size_t)g * NE_BOX + 1]) - py;
            const double d = sqrt(dx * dx + dy * dy);
            if (d < best.d) {                           // slots ascend, so a lane's equal distance keeps its lower index
                best.d = d;
                best.idx = g;
            }
        }
        best = wave_best(best, ne_nearer);
        const bool hit = best.d < thresh;
        if (hit && (best.idx & (EVAL_WAVE - 1)) == lane) taken |= 1u << (best.idx / EVAL_WAVE);
        if (lane == 0) out[i] = hit ? g0 + best.idx : -1;
        if (lane != 0 || !write_err) continue;          // the shuffles above are behind this prediction: lanes rejoin at the loop head
        double e[5];
        for (int k = 0; k < 5; ++k) e[k] = nan("");
        if (hit) {
            const double* a = gt + (size_t)best.idx * NE_BOX;
            const double* b = p.pred + (size_t)(p0 + i) * NE_BOX;
            const double dvx = a[3] - b[3], dvy = a[4] - b[4];
            const double inter = (fmin(a[5], b[5]) * fmin(a[6], b[6])) * fmin(a[7], b[7]);
            const double va = (a[5] * a[6]) * a[7], vb = (b[5] * b[6]) * b[7];
            double turn = ne_mod((a[2] - b[2]) + period / 2, period) - period / 2;
            if (turn > NE_PI) turn -= 2 * NE_PI;
            const int ga = p.gt_attr[g0 + best.idx];
            e[0] = best.d;
            e[1] = sqrt(dvx * dvx + dvy * dvy);
            e[2] = 1.0 - inter / ((va + vb) - inter);
            e[3] = fabs(turn);
            e[4] = ga < 0 ? nan("") : (ga == p.pred_attr[p0 + i] ? 0.0 : 1.0);
        }
        for (int k = 0; k < 5; ++k) err[(size_t)k * p.n_pred + p0 + i] = e[k];
    }
}

// ws: pred_off | gt_off | seg_cls
struct NeWs {
    WsCarver c;
    size_t pred_off, gt_off, seg_cls;
    explicit NeWs(int n_seg)
        : pred_off(c.take((size_t)(n_seg + 1) * sizeof(int32_t))), gt_off(c.take((size_t)(n_seg + 1) * sizeof(int32_t))),
          seg_cls(c.take((size_t)n_seg * sizeof(int32_t))) {}
};

}  // namespace toda

using namespace toda;

extern "C" int toda_nusc_eval_prepare(const double* rows, const int32_t* sample, const int32_t* cls, int n, const double* G,
                                      const double* ego, int n_samples, double* out, int32_t* keep, void* stream) {
    TODA_CHECK_ARG(n >= 0 && n_samples >= 0, "nusc_eval_prepare: negative size (n %d, n_samples %d)", n, n_samples);
    if (n == 0) return TODA_OK;
    TODA_CHECK_ARG(rows && sample && cls && out && keep, "nusc_eval_prepare: null rows, sample index, class or output");
    TODA_CHECK_ARG(n_samples == 0 || (G && ego), "nusc_eval_prepare: null transforms");
    hipLaunchKernelGGL(nusc_eval_prepare_kernel, dim3(cdiv(n, NE_BLOCK)), dim3(NE_BLOCK), 0, (hipStream_t)stream, rows, sample, cls, G,
                       ego, n, n_samples, out, keep);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" size_t toda_nusc_eval_match_workspace_bytes(int n_seg) {
    if (n_seg < 1) return 0;
    return NeWs(n_seg).c.at;
}

extern "C" int toda_nusc_eval_match(const double* pred, const double* pred_score, const int32_t* pred_attr, int n_pred,
                                    const double* gt, const int32_t* gt_attr, int n_gt, const int32_t* pred_off_host,
                                    const int32_t* gt_off_host, const int32_t* seg_cls_host, int n_seg,
                                    const double* thresholds_host, int tp_threshold, int32_t* match, double* err, void* ws,
                                    size_t ws_bytes, void* stream) {
    TODA_CHECK_ARG(n_pred >= 0 && n_gt >= 0 && n_seg >= 0, "nusc_eval_match: negative size (n_pred %d, n_gt %d, n_seg %d)", n_pred, n_gt, n_seg);
    if (n_pred == 0 || n_seg == 0) {
        TODA_CHECK_ARG(n_pred == 0, "nusc_eval_match: %d predictions but no segment", n_pred);
        return TODA_OK;
    }
    TODA_CHECK_ARG(pred && pred_score && pred_attr && match && err, "nusc_eval_match: null predictions or output");
    TODA_CHECK_ARG(n_gt == 0 || (gt && gt_attr), "nusc_eval_match: null ground truths");
    TODA_CHECK_ARG(pred_off_host && gt_off_host && seg_cls_host && thresholds_host, "nusc_eval_match: null offsets, classes or thresholds");
    TODA_CHECK_ARG(tp_threshold >= 0 && tp_threshold < NE_THRESH, "nusc_eval_match: tp_threshold must index the %d thresholds, got %d",
                   NE_THRESH, tp_threshold);
    // the taken mask holds NE_MAX_GT ground truths, NE_MAX_PRED predictions are ranked
    if (csr_check("nusc_eval_match", pred_off_host, n_seg, n_pred, NE_MAX_PRED, "predictions") != TODA_OK) return TODA_EINVAL;
    if (csr_check("nusc_eval_match", gt_off_host, n_seg, n_gt, NE_MAX_GT, "ground truths") != TODA_OK) return TODA_EINVAL;
    for (int s = 0; s < n_seg; ++s)
        TODA_CHECK_ARG(seg_cls_host[s] >= 0 && seg_cls_host[s] < NE_CLASSES, "nusc_eval_match: class %d of segment %d", seg_cls_host[s], s);
    const NeWs w(n_seg);
    TODA_CHECK_ARG(ws && ws_bytes >= w.c.at, "nusc_eval_match: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    NeMatch p = {};
    TODA_HIP(stage(ws, w.pred_off, pred_off_host, n_seg + 1, s, &p.pred_off));
    TODA_HIP(stage(ws, w.gt_off, gt_off_host, n_seg + 1, s, &p.gt_off));
    TODA_HIP(stage(ws, w.seg_cls, seg_cls_host, n_seg, s, &p.seg_cls));
    p.pred = pred;
    p.score = pred_score;
    p.pred_attr = pred_attr;
    p.gt = gt;
    p.gt_attr = gt_attr;
    p.n_pred = n_pred;
    p.n_gt = n_gt;
    p.tp_wave = tp_threshold;
    for (int k = 0; k < NE_THRESH; ++k) p.thresh[k] = thresholds_host[k];
    hipLaunchKernelGGL(nusc_eval_match_kernel, dim3(n_seg), dim3(NE_BLOCK), 0, s, p, match, err);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
