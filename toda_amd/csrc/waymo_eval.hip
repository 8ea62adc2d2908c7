// The Waymo detection metric's two device parts (LEVEL_1 / LEVEL_2 AP and APH per object type; the reference hands the metric to
// TensorFlow and the waymo_open_dataset package).  Written from the definition in DESIGN.md 3.15.  All arithmetic is fp64 without
// contraction or integer; no float atomics, so two runs give the same bits.  Every loop has a bound known before it starts.
//
// waymo_eval_iou_kernel: one workgroup per (frame, type) segment, one lane per (prediction, ground truth) pair of it.  The
// prediction's rectangle is moved into the ground truth's frame and clipped by the four half-planes |u| <= dx / 2, |v| <= dy / 2
// (no corner margins); shoelace area times the overlap of the z-intervals; IoU = inter / (volA + volB - inter), 0 when that
// denominator is not positive, clamped to [0, 1].  Pairs whose circumcircles are apart get their 0 at once; the others wait in an
// LDS queue until full waves of them can be clipped.  The order in the queue varies from run to run, a pair's value does not.
//
// waymo_eval_match_kernel: one single-wavefront workgroup per segment, so every column scan ends in a shuffle ladder and no step
// waits for another wave.  The wave ranks the predictions by (score descending, position: rank_by_score<false>) in LDS and inserts them one at a time
// into a shortest-augmenting-path assignment on the integer costs 1000 - w, w = IoU >= t ? (int)(IoU * 1000) : 0.  Pairs with
// w = 0 are no edges.  Every prediction has a private "stay free" column of cost 1000; these are not stored: such a column is
// reachable from its own row only, its dual stays 0, and a row that sits on it can never be entered again, so the nearest of them
// is one running minimum beside the column scan.  After k insertions the assignment is optimal for the k best-scored predictions:
// the 101 score cutoffs are snapshots of one pass, taken whenever the next score falls below the next cutoff.  The set of matched
// ground truths only grows (an augmenting path ends in a free column and frees none), so TP / FN / FP are running counters; the
// heading sum is taken afresh over the columns at a snapshot whose assignment changed.  Lane l owns columns l, l + 64, ...
//
// waymo_eval_fold_kernel: the per-segment snapshot slabs, added per type in one fixed order (fold_runs).
#include "eval_common.cuh"

namespace toda {

constexpr int WE_IOU_BLOCK = 256;
constexpr int WE_IOU_QUEUE = 2048;                     // pairs waiting to be clipped; a tile adds at most WE_IOU_BLOCK
constexpr int WE_FOLD_BLOCK = 256;
constexpr int WE_MAX_PRED = TODA_WAYMO_MAX_PRED;       // 512
constexpr int WE_MAX_GT = TODA_WAYMO_MAX_GT;           // 512
constexpr int WE_CUT = TODA_WAYMO_CUTOFFS;             // 101
constexpr int WE_TYPES = 4;                            // Vehicle, Pedestrian, Sign, Cyclist: estimator types 1..4
constexpr int WE_INT_ROWS = 5;                         // slab rows: tp L1, tp L2, fn L1, fn L2, fp
constexpr int WE_HA_ROWS = 2;                          // slab rows: sum_ha L1, L2
constexpr int WE_INF = 0x3fffffff;
constexpr double WE_PI = 3.14159265358979323846;

// one clip of a convex polygon (at most 8 corners) by c <= lim (sign +1) or c >= -lim (sign -1) on coordinate `axis`
__device__ __forceinline__ int we_clip(const double (*in)[2], int n, int axis, double sign, double lim, double (*out)[2]) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int k = i + 1 < n ? i + 1 : 0;
        const double pc = sign * in[i][axis], qc = sign * in[k][axis];
        const bool pin = pc <= lim, qin = qc <= lim;
        if (pin && m < 8) {
            out[m][0] = in[i][0];
            out[m][1] = in[i][1];
            ++m;
        }
        if (pin != qin && m < 8) {
            const double t = (lim - pc) / (qc - pc);
            const int o = 1 - axis;
            out[m][axis] = sign * lim;
            out[m][o] = in[i][o] + t * (in[k][o] - in[i][o]);
            ++m;
        }
    }
    return m;
}

// rows: x y z dx dy dz heading.  Rectangles whose circumcircles are apart by more than a part in a thousand clip to nothing: the
// margin is far above the rounding of the corners, so no pair with area is cut off and the full route would return the same 0.
__device__ __forceinline__ bool we_apart(const double* a, const double* b) {
    const double ex = a[0] - b[0], ey = a[1] - b[1];
    const double reach = sqrt(a[3] * a[3] + a[4] * a[4]) / 2 + sqrt(b[3] * b[3] + b[4] * b[4]) / 2;
    return ex * ex + ey * ey > (reach * reach) * 1.002;
}

// ca, sa / cb, sb: cosine and sine of the two headings
__device__ double we_iou(const double* a, const double* b, double ca, double sa, double cb, double sb) {
    const double hx = a[3] / 2, hy = a[4] / 2;
    const double sx[4] = {1.0, -1.0, -1.0, 1.0}, sy[4] = {1.0, 1.0, -1.0, -1.0};
    double p[8][2], q[8][2];
    for (int k = 0; k < 4; ++k) {
        const double lx = sx[k] * hx, ly = sy[k] * hy;
        const double rx = (a[0] + (lx * ca - ly * sa)) - b[0], ry = (a[1] + (lx * sa + ly * ca)) - b[1];
        p[k][0] = rx * cb + ry * sb;
        p[k][1] = ry * cb - rx * sb;
    }
    const double bx = b[3] / 2, by = b[4] / 2;
    int n = we_clip(p, 4, 0, 1.0, bx, q);
    n = we_clip(q, n, 0, -1.0, bx, p);
    n = we_clip(p, n, 1, 1.0, by, q);
    n = we_clip(q, n, 1, -1.0, by, p);
    double area = 0.0;
    if (n >= 3) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) {
            const int k = i + 1 < n ? i + 1 : 0;
            acc += p[i][0] * p[k][1] - p[k][0] * p[i][1];
        }
        area = fabs(acc) / 2;
    }
    const double zlo = fmax(a[2] - a[5] / 2, b[2] - b[5] / 2), zhi = fmin(a[2] + a[5] / 2, b[2] + b[5] / 2);
    const double h = fmax(zhi - zlo, 0.0);
    const double inter = area * h;
    const double den = ((a[3] * a[4]) * a[5] + (b[3] * b[4]) * b[5]) - inter;
    if (!(den > 0.0)) return 0.0;
    return fmin(fmax(inter / den, 0.0), 1.0);
}

// Tiles of 256 pairs: a lane writes 0 for a pair that is apart and queues the others in LDS; when the queue could not take another
// tile, and after the last one, all lanes clip the queued pairs, so the clipping runs on full waves although few pairs need it.
__global__ __launch_bounds__(WE_IOU_BLOCK) void waymo_eval_iou_kernel(const double* __restrict__ pred, const double* __restrict__ gt,
                                                                       const int32_t* __restrict__ pred_off,
                                                                       const int32_t* __restrict__ gt_off,
                                                                       const long long* __restrict__ iou_off, int n_pred, int n_gt,
                                                                       double* __restrict__ iou) {
    __shared__ double s_pcs[WE_MAX_PRED][2];   // cosine and sine of each heading, taken once per box
    __shared__ double s_gcs[WE_MAX_GT][2];
    __shared__ int s_queue[WE_IOU_QUEUE];
    __shared__ int s_count;
    const int seg = blockIdx.x;
    // the launcher has checked the offsets on the host; a segment outside the buffers is left alone, an empty one has no pairs
    const auto [p0, np, g0, ng, inside] = seg_span(pred_off, gt_off, seg, n_pred, n_gt, WE_MAX_PRED, WE_MAX_GT);
    if (!inside || np <= 0 || ng <= 0) return;
    const double* pa = pred + (size_t)p0 * 7;
    const double* gb = gt + (size_t)g0 * 7;
    double* dst = iou + iou_off[seg];
    for (int i = threadIdx.x; i < np; i += WE_IOU_BLOCK) {
        s_pcs[i][0] = cos(pa[(size_t)i * 7 + 6]);
        s_pcs[i][1] = sin(pa[(size_t)i * 7 + 6]);
    }
    for (int j = threadIdx.x; j < ng; j += WE_IOU_BLOCK) {
        s_gcs[j][0] = cos(gb[(size_t)j * 7 + 6]);
        s_gcs[j][1] = sin(gb[(size_t)j * 7 + 6]);
    }
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const int total = np * ng, tiles = (total + WE_IOU_BLOCK - 1) / WE_IOU_BLOCK;
    for (int tile = 0; tile < tiles; ++tile) {
        const int e = tile * WE_IOU_BLOCK + threadIdx.x;
        if (e < total) {
            const int i = e / ng, j = e - i * ng;
            if (we_apart(pa + (size_t)i * 7, gb + (size_t)j * 7)) dst[e] = 0.0;
            else s_queue[atomicAdd(&s_count, 1)] = e;
        }
        __syncthreads();
        const int count = s_count;
        __syncthreads();                                // every lane holds the same count before the next tile adds to it
        if (count <= WE_IOU_QUEUE - WE_IOU_BLOCK && tile + 1 < tiles) continue;
        for (int k = threadIdx.x; k < count; k += WE_IOU_BLOCK) {
            const int f = s_queue[k], i = f / ng, j = f - i * ng;
            dst[f] = we_iou(pa + (size_t)i * 7, gb + (size_t)j * 7, s_pcs[i][0], s_pcs[i][1], s_gcs[j][0], s_gcs[j][1]);
        }
        __syncthreads();
        if (threadIdx.x == 0) s_count = 0;
        __syncthreads();
    }
}

struct WeMatch {
    const double* iou;           // the segments' [n_pred_s, n_gt_s] blocks
    const float* score;          // [n_pred]
    const double* pred_heading;  // [n_pred]
    const double* gt_heading;    // [n_gt]
    const int32_t* gt_level;     // [n_gt]: difficulty, in level L iff <= L
    const int32_t* pred_off;     // [n_seg + 1]
    const int32_t* gt_off;       // [n_seg + 1]
    const long long* iou_off;    // [n_seg + 1]
    const int32_t* seg_type;     // [n_seg], 1..4
    const float* cutoffs;        // [WE_CUT], ascending
    int n_pred, n_gt;
};

struct WePick {
    int d, idx;
    __device__ WePick across(int m) const { return {__shfl_xor(d, m, EVAL_WAVE), __shfl_xor(idx, m, EVAL_WAVE)}; }
};

__device__ __forceinline__ bool we_nearer(const WePick& a, const WePick& b) { return a.d < b.d || (a.d == b.d && a.idx < b.idx); }

__device__ __forceinline__ int we_weight(double iou, double thresh) { return iou >= thresh ? (int)(fmin(iou, 1.0) * 1000.0) : 0; }

__global__ __launch_bounds__(EVAL_WAVE) void waymo_eval_match_kernel(WeMatch p, int32_t* __restrict__ slab_int, double* __restrict__ slab_ha,
                                                                   int32_t* __restrict__ match_dbg) {
    __shared__ float s_score[WE_MAX_PRED];
    __shared__ int s_order[WE_MAX_PRED];     // rank -> position in the segment
    __shared__ int s_u[WE_MAX_PRED];         // row duals, by rank
    __shared__ int s_rowcol[WE_MAX_PRED];    // by rank: column, or -1 on the row's own free column
    __shared__ int s_v[WE_MAX_GT];           // column duals
    __shared__ int s_minv[WE_MAX_GT];
    __shared__ int s_way[WE_MAX_GT];         // the tree column whose row reaches this one best, -1: the new row
    __shared__ int s_colrow[WE_MAX_GT];      // rank of the matched row, or -1
    __shared__ int s_used[WE_MAX_GT];
    __shared__ int s_level[WE_MAX_GT];
    __shared__ float s_cut[WE_CUT];
    __shared__ int s_cnt[WE_INT_ROWS][WE_CUT];
    __shared__ double s_ha[WE_HA_ROWS][WE_CUT];
    const int seg = blockIdx.x, lane = threadIdx.x;
    int32_t* out_int = slab_int + (size_t)seg * (WE_INT_ROWS * WE_CUT);
    double* out_ha = slab_ha + (size_t)seg * (WE_HA_ROWS * WE_CUT);
    // the launcher has checked the offsets on the host; a segment outside the buffers or the LDS arrays counts nothing
    const auto [p0, np, g0, ng, inside] = seg_span(p.pred_off, p.gt_off, seg, p.n_pred, p.n_gt, WE_MAX_PRED, WE_MAX_GT);
    if (!inside) {
        for (int e = lane; e < WE_INT_ROWS * WE_CUT; e += EVAL_WAVE) out_int[e] = 0;
        for (int e = lane; e < WE_HA_ROWS * WE_CUT; e += EVAL_WAVE) out_ha[e] = 0.0;
        return;
    }
    const double* iou = p.iou + p.iou_off[seg];
    const double thresh = p.seg_type[seg] == 1 ? 0.7 : 0.5;
    int n_l1 = 0, n_l2 = 0;
    for (int i = lane; i < np; i += EVAL_WAVE) {
        const float s = p.score[p0 + i];
        s_score[i] = s == s ? s : -HUGE_VALF;           // a NaN score is below every cutoff, and the order stays total
        s_rowcol[i] = -1;
        s_u[i] = 0;
    }
    for (int j = lane; j < ng; j += EVAL_WAVE) {
        const int lv = p.gt_level[g0 + j];
        s_level[j] = lv;
        s_v[j] = 0;
        s_colrow[j] = -1;
        n_l1 += lv <= 1 ? 1 : 0;
        n_l2 += lv <= 2 ? 1 : 0;
    }
    for (int k = lane; k < WE_CUT; k += EVAL_WAVE) s_cut[k] = p.cutoffs[k];
    n_l1 = wave_sum(n_l1);
    n_l2 = wave_sum(n_l2);
    __syncthreads();
    rank_by_score<false>(s_score, s_order, np, lane, EVAL_WAVE);            // equal scores: the earlier position first
    __syncthreads();

    int tp1 = 0, tp2 = 0, n_match = 0, n_in = 0, k = WE_CUT - 1;
    double ha1 = 0.0, ha2 = 0.0;
    bool ha_stale = false;
    // the state after n_in insertions is the answer at every cutoff the next score lies below; r == np flushes the rest
    for (int r = 0; r <= np; ++r) {
        const float sc = r < np ? s_score[s_order[r]] : -HUGE_VALF;
        for (; k >= 0 && (r == np || sc < s_cut[k]); --k) {
            if (ha_stale) {
                double a1 = 0.0, a2 = 0.0;
                for (int j = lane; j < ng; j += EVAL_WAVE) {
                    const int row = s_colrow[j];
                    if (row < 0) continue;
                    const double d = fmod(fabs(p.pred_heading[p0 + s_order[row]] - p.gt_heading[g0 + j]), 2 * WE_PI);
                    const double acc = 1.0 - fmin(d, 2 * WE_PI - d) / WE_PI;
                    a1 += s_level[j] <= 1 ? acc : 0.0;
                    a2 += s_level[j] <= 2 ? acc : 0.0;
                }
                ha1 = wave_sum(a1);
                ha2 = wave_sum(a2);
                ha_stale = false;
            }
            if (lane == 0) {
                s_cnt[0][k] = tp1;
                s_cnt[1][k] = tp2;
                s_cnt[2][k] = n_l1 - tp1;
                s_cnt[3][k] = n_l2 - tp2;
                s_cnt[4][k] = n_in - n_match;
                s_ha[0][k] = ha1;
                s_ha[1][k] = ha2;
            }
            if (match_dbg) {
                int32_t* dbg = match_dbg + (size_t)k * p.n_pred + p0;
                for (int rr = lane; rr < np; rr += EVAL_WAVE) dbg[s_order[rr]] = (rr < n_in && s_rowcol[rr] >= 0) ? g0 + s_rowcol[rr] : -1;
            }
        }
        if (k < 0 || r == np) break;

        // insert row r: Dijkstra over the columns on reduced costs, the duals kept current step by step
        for (int j = lane; j < ng; j += EVAL_WAVE) {
            s_minv[j] = WE_INF;
            s_used[j] = 0;
        }
        __syncthreads();
        int i0 = r, j0 = -1;                 // the tree row being expanded and the column it was reached through
        int dmin = WE_INF, dway = -1;        // the nearest private free column of a tree row, and that row's column
        int jend = -1;                       // the free ground truth reached, or -1: a private free column
        for (int step = 0; step <= ng; ++step) {
            const int ui0 = s_u[i0];
            const double* wrow = iou + (size_t)s_order[i0] * ng;
            if (1000 - ui0 < dmin) {
                dmin = 1000 - ui0;
                dway = j0;
            }
            WePick best = {WE_INF, 0x7fffffff};
            for (int j = lane; j < ng; j += EVAL_WAVE) {
                if (s_used[j]) continue;
                const int w = we_weight(wrow[j], thresh);
                int mv = s_minv[j];
                if (w > 0) {
                    const int cur = 1000 - w - ui0 - s_v[j];
                    if (cur < mv) {
                        mv = cur;
                        s_minv[j] = cur;
                        s_way[j] = j0;
                    }
                }
                if (mv < best.d) {                      // columns ascend, so a lane's equal distance keeps its lower index
                    best.d = mv;
                    best.idx = j;
                }
            }
            best = wave_best(best, we_nearer);
            const bool stay = dmin <= best.d;           // on equal distances the private column: the shorter path
            const int delta = stay ? dmin : best.d;
            for (int j = lane; j < ng; j += EVAL_WAVE) {
                if (s_used[j]) {
                    s_u[s_colrow[j]] += delta;
                    s_v[j] -= delta;
                } else if (s_minv[j] < WE_INF) {
                    s_minv[j] -= delta;
                }
            }
            if (lane == 0) s_u[r] += delta;
            dmin -= delta;
            if (stay) break;
            j0 = best.idx;
            if (lane == 0) s_used[j0] = 1;
            __syncthreads();
            i0 = s_colrow[j0];
            if (i0 < 0) {
                jend = j0;
                break;
            }
        }
        __syncthreads();
        if (lane == 0) {
            int j = jend;
            if (jend < 0) {                             // the row reached through dway leaves that column for its own free one
                s_rowcol[dway < 0 ? r : s_colrow[dway]] = -1;
                j = dway;
            }
            for (int hop = 0; hop <= ng && j >= 0; ++hop) {
                const int jp = s_way[j];
                const int row = jp < 0 ? r : s_colrow[jp];
                s_colrow[j] = row;
                s_rowcol[row] = j;
                j = jp;
            }
        }
        __syncthreads();
        ++n_in;
        if (jend >= 0) {
            ++n_match;
            tp1 += s_level[jend] <= 1 ? 1 : 0;
            tp2 += s_level[jend] <= 2 ? 1 : 0;
        }
        ha_stale = ha_stale || jend >= 0 || dway >= 0;
    }
    __syncthreads();
    for (int e = lane; e < WE_INT_ROWS * WE_CUT; e += EVAL_WAVE) out_int[e] = (&s_cnt[0][0])[e];
    for (int e = lane; e < WE_HA_ROWS * WE_CUT; e += EVAL_WAVE) out_ha[e] = (&s_ha[0][0])[e];
}

// Entry e = row * 101 + cutoff of the slabs (rows tp L1, tp L2, fn L1, fn L2, fp | sum_ha L1, L2), summed over the segments of type
// blockIdx.y + 1: lane k adds its contiguous run of segments in order, then a fixed tree.
__global__ __launch_bounds__(WE_FOLD_BLOCK) void waymo_eval_fold_kernel(const int32_t* __restrict__ slab_int, const double* __restrict__ slab_ha,
                                                                        const int32_t* __restrict__ seg_type, int n_seg,
                                                                        long long* __restrict__ tp, long long* __restrict__ fn,
                                                                        long long* __restrict__ fp, double* __restrict__ sum_ha) {
    __shared__ long long s_i[WE_FOLD_BLOCK];
    __shared__ double s_d[WE_FOLD_BLOCK];
    const int e = blockIdx.x, t = blockIdx.y;
    const int eh = e - WE_INT_ROWS * WE_CUT;
    // a segment of another type adds 0, which changes no sum: the integers trivially, and an fp64 run that starts at +0 never holds -0
    const auto load_int = [&](int s) { return seg_type[s] == t + 1 ? (long long)slab_int[(size_t)s * (WE_INT_ROWS * WE_CUT) + e] : 0ll; };
    const auto load_ha = [&](int s) { return seg_type[s] == t + 1 ? slab_ha[(size_t)s * (WE_HA_ROWS * WE_CUT) + eh] : 0.0; };
    const long long sum_i = eh < 0 ? fold_runs<long long, WE_FOLD_BLOCK>(n_seg, load_int, s_i) : 0;     // a workgroup folds one side only
    const double sum_d = eh < 0 ? 0.0 : fold_runs<double, WE_FOLD_BLOCK>(n_seg, load_ha, s_d);
    if (threadIdx.x != 0) return;
    const int row = e / WE_CUT, k = e - row * WE_CUT;
    if (row < 2) tp[((size_t)t * 2 + row) * WE_CUT + k] = sum_i;
    else if (row < 4) fn[((size_t)t * 2 + row - 2) * WE_CUT + k] = sum_i;
    else if (row < 5) fp[(size_t)t * WE_CUT + k] = sum_i;
    else sum_ha[((size_t)t * 2 + row - 5) * WE_CUT + k] = sum_d;
}

// ws: pred_off | gt_off | seg_type | iou_off | cutoffs | slab_int [n_seg, 5, 101] | slab_ha [n_seg, 2, 101]
struct WeWs {
    WsCarver c;
    size_t pred_off, gt_off, seg_type, iou_off, cutoffs, slab_int, slab_ha;
    explicit WeWs(int n_seg)
        : pred_off(c.take((size_t)(n_seg + 1) * sizeof(int32_t))), gt_off(c.take((size_t)(n_seg + 1) * sizeof(int32_t))),
          seg_type(c.take((size_t)n_seg * sizeof(int32_t))), iou_off(c.take((size_t)(n_seg + 1) * sizeof(long long))),
          cutoffs(c.take((size_t)WE_CUT * sizeof(float))), slab_int(c.take((size_t)n_seg * WE_INT_ROWS * WE_CUT * sizeof(int32_t))),
          slab_ha(c.take((size_t)n_seg * WE_HA_ROWS * WE_CUT * sizeof(double))) {}
};

// the sizes, the CSR offsets of both sides (csr_check) and the IoU blocks, read on the host before anything is launched
static int we_check_spans(const char* who, int n_pred, int n_gt, const int32_t* pred_off, const int32_t* gt_off, const long long* iou_off,
                          int n_seg, long long n_pairs) {
    TODA_CHECK_ARG(n_pred >= 0 && n_gt >= 0 && n_seg >= 0 && n_pairs >= 0, "%s: negative size (n_pred %d, n_gt %d, n_seg %d, n_pairs %lld)", who,
                   n_pred, n_gt, n_seg, n_pairs);
    if (n_seg == 0) {
        TODA_CHECK_ARG(n_pred == 0 && n_gt == 0 && n_pairs == 0, "%s: %d predictions, %d ground truths, %lld pairs but no segment", who, n_pred,
                       n_gt, n_pairs);
        return TODA_OK;
    }
    TODA_CHECK_ARG(pred_off && gt_off && iou_off, "%s: null offsets", who);
    if (csr_check(who, pred_off, n_seg, n_pred, WE_MAX_PRED, "predictions") != TODA_OK) return TODA_EINVAL;
    if (csr_check(who, gt_off, n_seg, n_gt, WE_MAX_GT, "ground truths") != TODA_OK) return TODA_EINVAL;
    TODA_CHECK_ARG(iou_off[0] == 0 && iou_off[n_seg] == n_pairs, "%s: the offsets of the IoU blocks must run from 0 to n_pairs", who);
    for (int s = 0; s < n_seg; ++s) {
        const int np = pred_off[s + 1] - pred_off[s], ng = gt_off[s + 1] - gt_off[s];
        TODA_CHECK_ARG(iou_off[s + 1] - iou_off[s] == (long long)np * ng, "%s: the IoU block of segment %d is not [%d, %d]", who, s, np, ng);
    }
    return TODA_OK;
}

}  // namespace toda

using namespace toda;

extern "C" size_t toda_waymo_eval_match_workspace_bytes(int n_seg) {
    if (n_seg < 1) return 0;
    return WeWs(n_seg).c.at;
}

extern "C" int toda_waymo_eval_iou(const double* pred, int n_pred, const double* gt, int n_gt, const int32_t* pred_off_host,
                                   const int32_t* gt_off_host, const long long* iou_off_host, int n_seg, long long n_pairs, double* iou,
                                   void* ws, size_t ws_bytes, void* stream) {
    if (we_check_spans("waymo_eval_iou", n_pred, n_gt, pred_off_host, gt_off_host, iou_off_host, n_seg, n_pairs) != TODA_OK) return TODA_EINVAL;
    if (n_seg == 0 || n_pairs == 0) return TODA_OK;
    TODA_CHECK_ARG(pred && gt && iou, "waymo_eval_iou: null boxes or output");
    const WeWs w(n_seg);
    TODA_CHECK_ARG(ws && ws_bytes >= w.c.at, "waymo_eval_iou: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int32_t *pred_off, *gt_off;
    const long long* iou_off;
    TODA_HIP(stage(ws, w.pred_off, pred_off_host, n_seg + 1, s, &pred_off));
    TODA_HIP(stage(ws, w.gt_off, gt_off_host, n_seg + 1, s, &gt_off));
    TODA_HIP(stage(ws, w.iou_off, iou_off_host, n_seg + 1, s, &iou_off));
    hipLaunchKernelGGL(waymo_eval_iou_kernel, dim3(n_seg), dim3(WE_IOU_BLOCK), 0, s, pred, gt, pred_off, gt_off, iou_off, n_pred, n_gt, iou);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_waymo_eval_match(const double* iou, const float* pred_score, const double* pred_heading, int n_pred,
                                     const double* gt_heading, const int32_t* gt_level, int n_gt, const int32_t* pred_off_host,
                                     const int32_t* gt_off_host, const long long* iou_off_host, const int32_t* seg_type_host, int n_seg,
                                     long long n_pairs, const float* cutoffs_host, long long* tp, long long* fn, long long* fp,
                                     double* sum_ha, int32_t* match_dbg, void* ws, size_t ws_bytes, void* stream) {
    if (we_check_spans("waymo_eval_match", n_pred, n_gt, pred_off_host, gt_off_host, iou_off_host, n_seg, n_pairs) != TODA_OK) return TODA_EINVAL;
    TODA_CHECK_ARG(tp && fn && fp && sum_ha, "waymo_eval_match: null output");
    TODA_CHECK_ARG(cutoffs_host, "waymo_eval_match: null cutoffs");
    for (int k = 0; k < WE_CUT; ++k)
        TODA_CHECK_ARG(cutoffs_host[k] == cutoffs_host[k] && (k == 0 || cutoffs_host[k] >= cutoffs_host[k - 1]),
                       "waymo_eval_match: the %d cutoffs must ascend (entry %d)", WE_CUT, k);
    hipStream_t s = (hipStream_t)stream;
    const size_t cells = (size_t)WE_TYPES * 2 * WE_CUT;
    if (n_seg == 0) {
        TODA_HIP(hipMemsetAsync(tp, 0, cells * sizeof(long long), s));
        TODA_HIP(hipMemsetAsync(fn, 0, cells * sizeof(long long), s));
        TODA_HIP(hipMemsetAsync(fp, 0, cells / 2 * sizeof(long long), s));
        TODA_HIP(hipMemsetAsync(sum_ha, 0, cells * sizeof(double), s));
        return TODA_OK;
    }
    TODA_CHECK_ARG(seg_type_host, "waymo_eval_match: null segment types");
    for (int g = 0; g < n_seg; ++g)
        TODA_CHECK_ARG(seg_type_host[g] >= 1 && seg_type_host[g] <= WE_TYPES, "waymo_eval_match: type %d of segment %d (1 Vehicle .. 4 Cyclist)",
                       seg_type_host[g], g);
    TODA_CHECK_ARG(n_pred == 0 || (pred_score && pred_heading), "waymo_eval_match: null scores or headings of the predictions");
    TODA_CHECK_ARG(n_gt == 0 || (gt_heading && gt_level), "waymo_eval_match: null headings or levels of the ground truths");
    TODA_CHECK_ARG(n_pairs == 0 || iou, "waymo_eval_match: null IoU blocks");
    const WeWs w(n_seg);
    TODA_CHECK_ARG(ws && ws_bytes >= w.c.at, "waymo_eval_match: workspace too small");
    WeMatch p = {};
    TODA_HIP(stage(ws, w.pred_off, pred_off_host, n_seg + 1, s, &p.pred_off));
    TODA_HIP(stage(ws, w.gt_off, gt_off_host, n_seg + 1, s, &p.gt_off));
    TODA_HIP(stage(ws, w.iou_off, iou_off_host, n_seg + 1, s, &p.iou_off));
    TODA_HIP(stage(ws, w.seg_type, seg_type_host, n_seg, s, &p.seg_type));
    TODA_HIP(stage(ws, w.cutoffs, cutoffs_host, WE_CUT, s, &p.cutoffs));
    p.iou = iou;
    p.score = pred_score;
    p.pred_heading = pred_heading;
    p.gt_heading = gt_heading;
    p.gt_level = gt_level;
    p.n_pred = n_pred;
    p.n_gt = n_gt;
    int32_t* slab_int = (int32_t*)((char*)ws + w.slab_int);
    double* slab_ha = (double*)((char*)ws + w.slab_ha);
    hipLaunchKernelGGL(waymo_eval_match_kernel, dim3(n_seg), dim3(EVAL_WAVE), 0, s, p, slab_int, slab_ha, match_dbg);
    TODA_LAUNCH_CHECK();
    hipLaunchKernelGGL(waymo_eval_fold_kernel, dim3((WE_INT_ROWS + WE_HA_ROWS) * WE_CUT, WE_TYPES), dim3(WE_FOLD_BLOCK), 0, s,
                       (const int32_t*)slab_int, (const double*)slab_ha, p.seg_type, n_seg, tp, fn, fp, sum_ha);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
