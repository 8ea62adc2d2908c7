// The KITTI AP evaluator's two device parts (reference: pcdet/datasets/kitti/kitti_object_eval_python/rotate_iou.py, a
// numba-CUDA kernel, and eval.py:87-154 / 157-337, numba-JIT host loops).
//
// eval_overlaps_kernel: one workgroup per frame, one (box, query) pair per lane, only same-frame pairs.  The rotated part is
// the metric's own intersection, not rotated_overlap.cuh: corners inside the other rectangle are taken with NO margin, edge
// crossings by strict sign tests, the points are ordered by angle about their centroid and the area is a triangle fan, all in
// fp32 without contraction, angles clockwise-positive.  Two rectangles that share corners or edges can yield more than the 8
// points of a generic intersection; the point buffer holds every point the two loops can produce (8 + 16).
// One case is decided before the arithmetic: a corner whose two coordinates EQUAL those of a corner of the other rectangle
// lies on that rectangle and is taken (the inside test includes the boundary).  The reference leaves this case to the signs
// of two rounded dot products that are zero in exact arithmetic, and so returns an intersection of 0 or of half the area
// for most pairs of bit-identical rotated rectangles; here a box against itself has IoU 1.  No other pair is affected.
//
// eval_match_kernel: one wavefront per (frame, score threshold).  Ground truths are visited in order (an earlier match takes
// its detection away from a later one); the detections of one ground truth are reduced across the wave by a rule without
// carried state (see ev_better; the ladder is eval_common.cuh's wave_best).  The wave's counts and its AOS sum go to a [F, T, 4] slab of
// doubles; eval_fold_kernel adds the frames up in one fixed order (fold_runs), so two runs give the same bits.  No atomics anywhere.
#include "eval_common.cuh"

namespace toda {

constexpr int EV_BLOCK = 256;
constexpr int EV_WAVES = EV_BLOCK / EVAL_WAVE;
constexpr int EV_MAX_PTS = 24;     // 4 + 4 corners, 4 x 4 edge crossings

struct EvPt {
    float x, y;
};

__device__ __forceinline__ EvPt ev_from(EvPt o, EvPt p) { return {p.x - o.x, p.y - o.y}; }
__device__ __forceinline__ float ev_dot(EvPt u, EvPt v) { return u.x * v.x + u.y * v.y; }
__device__ __forceinline__ float ev_det(EvPt u, EvPt v) { return u.x * v.y - v.x * u.y; }
__device__ __forceinline__ bool ev_same(EvPt u, EvPt v) { return u.x == v.x && u.y == v.y; }

// Orientation predicate: seen from o, does u lie strictly on the turning side of v?  A zero determinant is "no".
__device__ __forceinline__ bool ev_turn(EvPt o, EvPt u, EvPt v) {
    const EvPt s = ev_from(o, u), t = ev_from(o, v);
    return s.y * t.x > t.y * s.x;
}

struct EvRect {
    EvPt c[4];      // (-,-) (-,+) (+,+) (+,-) half extents, turned clockwise by the angle, moved to the centre
};

__device__ __forceinline__ EvRect ev_rect(const float* r) {          // r = cx, cy, dx, dy, angle
    const float co = (float)cos((double)r[4]), si = (float)sin((double)r[4]);
    const float hx = r[2] / 2, hy = r[3] / 2;
    EvRect out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float lx = (k & 2) ? hx : -hx, ly = (k == 1 || k == 2) ? hy : -hy;
        out.c[k] = {co * lx + si * ly + r[0], -si * lx + co * ly + r[1]};
    }
    return out;
}

// Is p in the closed rectangle?  Its offset from corner 0, projected on the two sides that leave corner 0, must fall within
// [0, |side|^2] on both.  A point that IS one of the four corners is in, whatever the rounding of the projections says.
__device__ __forceinline__ bool ev_holds(const EvRect& r, EvPt p) {
    if (ev_same(p, r.c[0]) || ev_same(p, r.c[1]) || ev_same(p, r.c[2]) || ev_same(p, r.c[3])) return true;
    const EvPt off = ev_from(r.c[0], p);
    for (int side = 1; side <= 3; side += 2) {
        const EvPt e = ev_from(r.c[0], r.c[side]);
        const float len2 = ev_dot(e, e), proj = ev_dot(e, off);
        if (!(len2 >= proj && proj >= 0)) return false;
    }
    return true;
}

// Proper crossing of segment a-b with segment c-d: c and d on different sides of a-b AND a and b on different sides of c-d,
// each by the strict orientation predicate (touching or collinear segments do not cross).  The point is the intersection
// of the two carrier lines by determinants.
__device__ __forceinline__ bool ev_meet(EvPt a, EvPt b, EvPt c, EvPt d, EvPt* at) {
    if (ev_turn(a, d, c) == ev_turn(b, d, c)) return false;
    if (ev_turn(a, c, b) == ev_turn(a, d, b)) return false;
    const EvPt s = ev_from(a, b), t = ev_from(c, d);
    const float wa = ev_det(a, b), wc = ev_det(c, d);
    const float den = s.y * t.x - s.x * t.y;
    at->x = (wa * t.x - s.x * wc) / den;
    at->y = (wa * t.y - s.y * wc) / den;
    return true;
}

// area of the intersection of rectangle a with rectangle b, each (cx, cy, dx, dy, angle); `a` is the first operand
__device__ float ev_rect_inter(const float* a, const float* b) {
    const EvRect p = ev_rect(a), q = ev_rect(b);
    EvPt pts[EV_MAX_PTS];
    float key[EV_MAX_PTS];
    int order[EV_MAX_PTS];
    int n = 0;
    for (int k = 0; k < 4; ++k) {
        if (ev_holds(q, p.c[k])) pts[n++] = p.c[k];
        if (ev_holds(p, q.c[k])) pts[n++] = q.c[k];
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            EvPt at;
            if (ev_meet(p.c[i], p.c[(i + 1) & 3], q.c[j], q.c[(j + 1) & 3], &at)) pts[n++] = at;   // n <= 8 + 16 = EV_MAX_PTS
        }
    if (n < 3) return 0.0f;
    // Angular order about the mean point.  The key is monotone in the angle: the unit direction's x over the upper half
    // plane, -2 minus it over the lower.  A point on the mean has a NaN key; every comparison with it is false, so the
    // stable index sort below leaves it where it stands.
    EvPt mean = {0.0f, 0.0f};
    for (int i = 0; i < n; ++i) {
        mean.x += pts[i].x;
        mean.y += pts[i].y;
    }
    mean.x /= n;
    mean.y /= n;
    for (int i = 0; i < n; ++i) {
        EvPt dir = ev_from(mean, pts[i]);
        const float len = sqrtf(dir.x * dir.x + dir.y * dir.y);
        dir.x = dir.x / len;
        dir.y = dir.y / len;
        key[i] = dir.y < 0 ? -2 - dir.x : dir.x;
        order[i] = i;
    }
    for (int i = 1; i < n; ++i) {
        const int moving = order[i];
        int slot = i;
        while (slot > 0 && key[order[slot - 1]] > key[moving]) {
            order[slot] = order[slot - 1];
            --slot;
        }
        order[slot] = moving;
    }
    // fan of triangles from the first point of the order
    const EvPt apex = pts[order[0]];
    float area = 0.0f;
    for (int i = 1; i + 1 < n; ++i) {
        const EvPt u = pts[order[i]], v = pts[order[i + 1]];
        area += fabsf(((apex.x - v.x) * (u.y - v.y) - (apex.y - v.y) * (u.x - v.x)) / 2.0f);
    }
    return area;
}

__device__ __forceinline__ float ev_norm(float inter, float first, float second, int criterion) {
    if (criterion == -1) return inter / (first + second - inter);
    if (criterion == 0) return inter / first;
    if (criterion == 1) return inter / second;
    return inter;
}

// box3d rows: x, y, z, l, h, w, ry (KITTI camera frame; y is the bottom face, the box spans [y - h, y]); bbox rows: x1 y1 x2 y2
__global__ __launch_bounds__(EV_BLOCK) void eval_overlaps_kernel(const float* __restrict__ box3d, const float* __restrict__ bbox,
                                                                  const float* __restrict__ q3d, const float* __restrict__ qbbox,
                                                                  const int32_t* __restrict__ box_off,
                                                                  const int32_t* __restrict__ q_off,
                                                                  const long long* __restrict__ out_off, int n_frames,
                                                                  int metric, int criterion, float* __restrict__ out) {
    for (int f = blockIdx.x; f < n_frames; f += gridDim.x) {
        const int b0 = box_off[f], nb = box_off[f + 1] - b0;
        const int g0 = q_off[f], nq = q_off[f + 1] - g0;
        float* dst = out + out_off[f];
        for (int e = threadIdx.x; e < nb * nq; e += EV_BLOCK) {
            const int i = e / nq, k = e - i * nq;
            float v = 0.0f;
            if (metric == 0) {
                const float* b = bbox + (size_t)(b0 + i) * 4;
                const float* q = qbbox + (size_t)(g0 + k) * 4;
                const float iw = fminf(b[2], q[2]) - fmaxf(b[0], q[0]);
                const float ih = fminf(b[3], q[3]) - fmaxf(b[1], q[1]);
                if (iw > 0 && ih > 0) {
                    const float ba = (b[2] - b[0]) * (b[3] - b[1]), qa = (q[2] - q[0]) * (q[3] - q[1]);
                    const float ua = criterion == -1 ? ba + qa - iw * ih : criterion == 0 ? ba : criterion == 1 ? qa : 1.0f;
                    v = iw * ih / ua;
                }
            } else {
                const float* b = box3d + (size_t)(b0 + i) * 7;
                const float* q = q3d + (size_t)(g0 + k) * 7;
                const float rb[5] = {b[0], b[2], b[3], b[5], b[6]};
                const float rq[5] = {q[0], q[2], q[3], q[5], q[6]};
                const float inter = ev_rect_inter(rq, rb);           // the query rectangle is the first operand
                if (metric == 1) {
                    v = ev_norm(inter, rq[2] * rq[3], rb[2] * rb[3], criterion);
                } else if (inter > 0) {
                    // the vertical part in fp64 on the fp32 area, as the host loop that follows the kernel in the reference
                    const double top = fmin((double)b[1], (double)q[1]);
                    const double bot = fmax((double)b[1] - (double)b[4], (double)q[1] - (double)q[4]);
                    const double ih = top - bot;
                    if (ih > 0) {
                        const double vb = (double)b[3] * (double)b[4] * (double)b[5];
                        const double vq = (double)q[3] * (double)q[4] * (double)q[5];
                        const double inc = ih * (double)inter;
                        const double ua = criterion == -1 ? vb + vq - inc : criterion == 0 ? vb : criterion == 1 ? vq : inc;
                        v = (float)(inc / ua);
                    }
                }
            }
            dst[e] = v;
        }
    }
}

// ---- matching -----------------------------------------------------------------------------------------------------------

struct EvPick {
    int cls;      // 2: a detection that counts, 1: an ignored one (height below the difficulty's minimum), 0: none
    double val;   // what is maximised inside cls 2
    int idx;
    __device__ EvPick across(int m) const { return {__shfl_xor(cls, m, EVAL_WAVE), __shfl_xor(val, m, EVAL_WAVE), __shfl_xor(idx, m, EVAL_WAVE)}; }
};

__device__ __forceinline__ bool ev_better(const EvPick& a, const EvPick& b) {   // a before b
    if (a.cls != b.cls) return a.cls > b.cls;
    if (a.val != b.val) return a.val > b.val;
    return a.idx < b.idx;
}

struct EvMatch {
    const float* overlaps;        // ragged [n_det_f, n_gt_f] blocks
    const long long* ov_off;      // [F + 1]
    const int32_t* det_off;       // [F + 1]
    const int32_t* gt_off;        // [F + 1]
    const int32_t* ign_det;       // -1 other class, 0 counts, 1 ignored
    const int32_t* ign_gt;
    const double* score;          // per detection
    const double* det_alpha;
    const double* gt_alpha;
    const double* det_bbox;       // [n_det, 4], metric 0 only
    const double* dc_bbox;        // [n_dc, 4] DontCare regions
    const int32_t* dc_off;        // [F + 1]
    const double* thresh;         // [T]
    int n_frames, n_thresh, n_det_total, use_dc, aos;
    double min_overlap;
};

// The inner loop of the reference over the detections of one ground truth, as a rule without carried state.  A candidate
// is a detection of the class (ign != -1), not assigned, not under the threshold, with overlap > min_overlap.
//   FP (thresholded pass): the candidate with ign == 0 of largest overlap, lowest index on ties (the reference replaces its
//     choice only on a strictly larger overlap, and an ign == 0 candidate always replaces an ign == 1 one); without any, the
//     lowest-index candidate with ign == 1 (only the first is taken, later ones find a choice already made).
//   !FP (first pass): the candidate of largest score, lowest index on ties, whatever its ign.
// Lane l owns detections l, l + 64, ...: it alone reads and writes their `assigned` bytes.
template <bool FP>
__global__ __launch_bounds__(EV_BLOCK) void eval_match_kernel(EvMatch p, unsigned char* __restrict__ assigned_ws,
                                                               double* __restrict__ partial, double* __restrict__ scores_out,
                                                               int32_t* __restrict__ count_out) {
    const int lane = threadIdx.x & (EVAL_WAVE - 1);
    const long long item = (long long)blockIdx.x * EV_WAVES + (threadIdx.x / EVAL_WAVE);
    if (item >= (long long)p.n_frames * p.n_thresh) return;       // whole waves leave: no barrier below
    const int f = (int)(item / p.n_thresh), t = (int)(item - (long long)f * p.n_thresh);
    const int d0 = p.det_off[f], nd = p.det_off[f + 1] - d0;
    const int g0 = p.gt_off[f], ng = p.gt_off[f + 1] - g0;
    const float* ov = p.overlaps + p.ov_off[f];
    const int32_t* ign_det = p.ign_det + d0;
    const double* score = p.score + d0;
    unsigned char* assigned = assigned_ws + (size_t)t * p.n_det_total + d0;
    const double thresh = FP ? p.thresh[t] : 0.0;
    for (int j = lane; j < nd; j += EVAL_WAVE) assigned[j] = 0;
    int tp = 0, fn = 0;
    double sim = 0.0;
    for (int i = 0; i < ng; ++i) {
        const int ig = p.ign_gt[g0 + i];
        if (ig == -1) continue;
        EvPick best = {0, 0.0, 0x7fffffff};
        for (int j = lane; j < nd; j += EVAL_WAVE) {
            const int id = ign_det[j];
            if (id == -1 || assigned[j]) continue;
            if (FP && score[j] < thresh) continue;
            const float o = ov[(size_t)j * ng + i];
            if (!((double)o > p.min_overlap)) continue;
            EvPick c;
            if (FP) {
                c.cls = id == 0 ? 2 : 1;
                c.val = id == 0 ? (double)o : 0.0;
            } else {
                c.cls = 2;
                c.val = score[j];
            }
            c.idx = j;
            if (ev_better(c, best)) best = c;
        }
        best = wave_best(best, ev_better);
        if (best.cls == 0) {
            if (ig == 0) ++fn;
            continue;
        }
        const int di = best.idx;
        if ((di & (EVAL_WAVE - 1)) == lane) assigned[di] = 1;
        if (ig == 1 || ign_det[di] == 1) continue;
        if (!FP) {
            if (lane == 0) scores_out[g0 + tp] = score[di];
        } else if (p.aos) {
            sim += (1.0 + cos(p.gt_alpha[g0 + i] - p.det_alpha[d0 + di])) / 2.0;
        }
        ++tp;
    }
    if (!FP) {
        if (lane == 0) count_out[f] = tp;
        return;
    }
    // false positives: counting detections left over, minus those a DontCare region covers (image metric only)
    const int c0 = p.use_dc ? p.dc_off[f] : 0, nc = p.use_dc ? p.dc_off[f + 1] - c0 : 0;
    int fp = 0;
    for (int j = lane; j < nd; j += EVAL_WAVE) {
        if (assigned[j] || ign_det[j] != 0 || score[j] < thresh) continue;
        bool stuff = false;
        const double* b = p.det_bbox + (size_t)(d0 + j) * 4;
        for (int c = 0; c < nc && !stuff; ++c) {
            const double* q = p.dc_bbox + (size_t)(c0 + c) * 4;
            const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
            const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
            if (iw > 0 && ih > 0) stuff = iw * ih / ((b[2] - b[0]) * (b[3] - b[1])) > p.min_overlap;
        }
        if (!stuff) ++fp;
    }
    fp = wave_sum(fp);
    if (lane == 0) {
        double* dst = partial + ((size_t)f * p.n_thresh + t) * 4;
        dst[0] = tp;
        dst[1] = fp;
        dst[2] = fn;
        dst[3] = sim;
    }
}

// pr[t, c] = sum over frames of partial[f, t, c]: lane k adds its contiguous run of frames in order, then a fixed tree
__global__ __launch_bounds__(EV_BLOCK) void eval_fold_kernel(const double* __restrict__ partial, int n_frames, int n_thresh,
                                                              double* __restrict__ pr) {
    __shared__ double s[EV_BLOCK];
    const int t = blockIdx.x, c = blockIdx.y;
    const double sum = fold_runs<double, EV_BLOCK>(n_frames, [&](int f) { return partial[((size_t)f * n_thresh + t) * 4 + c]; }, s);
    if (threadIdx.x == 0) pr[t * 4 + c] = sum;
}

// ws: partial [F, T, 4] doubles | assigned [T, n_det_total] bytes | one spare slot (part of the size this export has always returned)
struct EvWs {
    WsCarver c;
    size_t partial, assigned, spare;
    EvWs(int n_frames, int n_thresh, int n_det_total)
        : partial(c.take((size_t)n_frames * n_thresh * 4 * sizeof(double))), assigned(c.take((size_t)n_thresh * n_det_total)),
          spare(c.take(256)) {}
};

}  // namespace toda

using namespace toda;

extern "C" int toda_eval_overlaps(const float* box3d, const float* bbox, const int32_t* box_off, const float* query3d,
                                  const float* query_bbox, const int32_t* query_off, const long long* out_off, int n_frames,
                                  long long n_pairs, int metric, int criterion, float* out, void* stream) {
    TODA_CHECK_ARG(metric >= 0 && metric <= 2, "eval_overlaps: metric must be 0 (image box), 1 (BEV) or 2 (3-D), got %d", metric);
    TODA_CHECK_ARG(criterion >= -1 && criterion <= 2, "eval_overlaps: criterion must be -1, 0, 1 or 2, got %d", criterion);
    TODA_CHECK_ARG(n_frames >= 0 && n_pairs >= 0, "eval_overlaps: negative size");
    if (n_frames == 0 || n_pairs == 0) return TODA_OK;
    TODA_CHECK_ARG(box_off && query_off && out_off && out, "eval_overlaps: null offsets or output");
    TODA_CHECK_ARG(metric == 0 ? (bbox && query_bbox) : (box3d && query3d), "eval_overlaps: null boxes for metric %d", metric);
    const int grid = n_frames < (1 << 20) ? n_frames : (1 << 20);
    hipLaunchKernelGGL(eval_overlaps_kernel, dim3(grid), dim3(EV_BLOCK), 0, (hipStream_t)stream, box3d, bbox, query3d,
                       query_bbox, box_off, query_off, out_off, n_frames, metric, criterion, out);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" size_t toda_eval_match_workspace_bytes(int n_frames, int n_thresh, int n_det_total) {
    if (n_frames < 1 || n_thresh < 1 || n_det_total < 0) return 0;
    return EvWs(n_frames, n_thresh, n_det_total).c.at;
}

static int ev_fill(EvMatch& p, const char* who, const float* overlaps, const long long* ov_off, const int32_t* det_off,
                   const int32_t* gt_off, const int32_t* ign_det, const int32_t* ign_gt, const double* score, int n_frames,
                   int n_det_total, double min_overlap) {
    TODA_CHECK_ARG(n_frames >= 0 && n_det_total >= 0, "%s: negative size", who);
    TODA_CHECK_ARG(min_overlap >= 0.0 && min_overlap < 1.0, "%s: min_overlap must lie in [0, 1), got %g", who, min_overlap);
    if (n_frames == 0) return TODA_OK;
    TODA_CHECK_ARG(ov_off && det_off && gt_off, "%s: null offsets", who);
    p.overlaps = overlaps;
    p.ov_off = ov_off;
    p.det_off = det_off;
    p.gt_off = gt_off;
    p.ign_det = ign_det;
    p.ign_gt = ign_gt;
    p.score = score;
    p.n_frames = n_frames;
    p.n_det_total = n_det_total;
    p.min_overlap = min_overlap;
    return TODA_OK;
}

extern "C" int toda_eval_match_scores(const float* overlaps, const long long* ov_off, const int32_t* det_off,
                                      const int32_t* gt_off, const int32_t* ign_det, const int32_t* ign_gt,
                                      const double* det_score, int n_frames, int n_det_total, double min_overlap,
                                      double* scores_out, int32_t* count_out, void* ws, size_t ws_bytes, void* stream) {
    EvMatch p = {};
    const int rc = ev_fill(p, "eval_match_scores", overlaps, ov_off, det_off, gt_off, ign_det, ign_gt, det_score, n_frames,
                           n_det_total, min_overlap);
    if (rc != TODA_OK || n_frames == 0) return rc;
    TODA_CHECK_ARG(count_out, "eval_match_scores: null count output");
    TODA_CHECK_ARG(ws && ws_bytes >= toda_eval_match_workspace_bytes(n_frames, 1, n_det_total),
                   "eval_match_scores: workspace too small");
    p.n_thresh = 1;
    unsigned char* assigned = (unsigned char*)ws + EvWs(n_frames, 1, n_det_total).assigned;
    hipLaunchKernelGGL(eval_match_kernel<false>, dim3(cdiv(n_frames, EV_WAVES)), dim3(EV_BLOCK), 0, (hipStream_t)stream, p,
                       assigned, (double*)nullptr, scores_out, count_out);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_eval_match(const float* overlaps, const long long* ov_off, const int32_t* det_off, const int32_t* gt_off,
                               const int32_t* ign_det, const int32_t* ign_gt, const double* det_score, const double* det_alpha,
                               const double* gt_alpha, const double* det_bbox, const double* dc_bbox, const int32_t* dc_off,
                               int n_frames, int n_det_total, const double* thresholds, int n_thresh, double min_overlap,
                               int metric, int compute_aos, double* pr, void* ws, size_t ws_bytes, void* stream) {
    EvMatch p = {};
    const int rc = ev_fill(p, "eval_match", overlaps, ov_off, det_off, gt_off, ign_det, ign_gt, det_score, n_frames, n_det_total,
                           min_overlap);
    if (rc != TODA_OK) return rc;
    TODA_CHECK_ARG(metric >= 0 && metric <= 2, "eval_match: metric must be 0, 1 or 2, got %d", metric);
    TODA_CHECK_ARG(n_thresh >= 0 && n_thresh <= 65535, "eval_match: need 0 <= thresholds <= 65535, got %d", n_thresh);
    if (n_thresh == 0) return TODA_OK;
    TODA_CHECK_ARG(pr && thresholds, "eval_match: null thresholds or output");
    hipStream_t s = (hipStream_t)stream;
    if (n_frames == 0) {
        TODA_HIP(hipMemsetAsync(pr, 0, (size_t)n_thresh * 4 * sizeof(double), s));
        return TODA_OK;
    }
    TODA_CHECK_ARG(!compute_aos || (det_alpha && gt_alpha), "eval_match: AOS needs both alpha arrays");
    TODA_CHECK_ARG(metric != 0 || ((det_bbox || n_det_total == 0) && dc_off),
                   "eval_match: the image metric needs the detections' boxes and dc_off");
    TODA_CHECK_ARG(ws && ws_bytes >= toda_eval_match_workspace_bytes(n_frames, n_thresh, n_det_total),
                   "eval_match: workspace too small");
    TODA_CHECK_ARG((long long)n_frames * n_thresh < (1ll << 31), "eval_match: too many (frame, threshold) pairs");
    p.det_alpha = det_alpha;
    p.gt_alpha = gt_alpha;
    p.det_bbox = det_bbox;
    p.dc_bbox = dc_bbox;
    p.dc_off = dc_off;
    p.thresh = thresholds;
    p.n_thresh = n_thresh;
    p.use_dc = metric == 0 ? 1 : 0;
    p.aos = compute_aos ? 1 : 0;
    const EvWs w(n_frames, n_thresh, n_det_total);
    double* partial = (double*)((char*)ws + w.partial);
    unsigned char* assigned = (unsigned char*)ws + w.assigned;
    hipLaunchKernelGGL(eval_match_kernel<true>, dim3(cdiv((long long)n_frames * n_thresh, EV_WAVES)), dim3(EV_BLOCK), 0, s, p,
                       assigned, partial, (double*)nullptr, (int32_t*)nullptr);
    TODA_LAUNCH_CHECK();
    hipLaunchKernelGGL(eval_fold_kernel, dim3(n_thresh, 4), dim3(EV_BLOCK), 0, s, (const double*)partial, n_frames, n_thresh, pr);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
