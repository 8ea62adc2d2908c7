// Anchor target assignment on the GPU for the whole batch and every anchor class in two launches
// (reference: a Python loop over batch x classes, pcdet/models/dense_heads/target_assigner/
// axis_aligned_target_assigner.py:36-210, with POS_FRACTION < 0, NORM_BY_NUM_EXAMPLES False, MATCH_HEIGHT False).
// Grid = (anchor tile, class, sample), one anchor per lane.  The sample's gt rectangles of the class are compacted into LDS
// in gt order and read as broadcasts.  Pass 1 takes each gt's maximum IoU over the anchors: wave reduction, LDS atomicMax,
// one global atomicMax per gt per workgroup, all on the fp32 bit pattern (IoU >= 0 orders like an int: order independent ->
// deterministic).  Pass 2 recomputes the IoUs with the same function against the finished maxima, decides the label,
// encodes the positives and writes labels, targets and weights in the requested anchor order.
#include "common.h"

namespace toda {

constexpr int AA_BLOCK = 256;
constexpr int AA_WAVE = 64;
constexpr int AA_CHUNK = AA_BLOCK;        // gt rows scanned (and at most kept) per LDS chunk
constexpr int AA_MAX_CLASSES = 32;
constexpr int AA_MAX_CODE = 16;

struct AAClass {
    const float* anchors;   // [locs, per_loc, stride]
    int locs, per_loc;      // nz*ny*nx, sizes*rotations
    int out_off;            // single-head order: first column of the class inside a location; multi-head: unused
    long long out_base;     // multi-head order: first output row of the class
    float matched, unmatched;
};

struct AAParams {
    AAClass cls[AA_MAX_CLASSES];
    const float* gt;         // [B, M, gt_stride], class id in the last column
    const int32_t* slot_of;  // [n_ids] class id -> anchor class, -1: none
    int n_ids, n_gt, gt_stride, anchor_stride, code, n_extra, sincos, multihead;
    int per_loc_total;       // single-head order: anchors per location over all classes
    long long n_anchor;      // output rows per sample
};

struct AARect {
    float x1, y1, x2, y2, area;
};

// box_utils.boxes3d_lidar_to_aligned_bev_boxes for one box, fp32, the operation order torch evaluates.
__device__ __forceinline__ AARect aa_rect(const float* box) {
    const float pi = 3.14159265358979323846f;
    const float r = box[6];
    const float rot = fabsf(__fsub_rn(r, __fmul_rn(floorf(__fadd_rn(__fdiv_rn(r, pi), 0.5f)), pi)));
    const bool keep = rot < (float)(3.14159265358979323846 / 4);
    const float hx = __fdiv_rn(keep ? box[3] : box[4], 2.0f), hy = __fdiv_rn(keep ? box[4] : box[3], 2.0f);
    AARect q;
    q.x1 = __fsub_rn(box[0], hx);
    q.y1 = __fsub_rn(box[1], hy);
    q.x2 = __fadd_rn(box[0], hx);
    q.y2 = __fadd_rn(box[1], hy);
    q.area = __fmul_rn(__fsub_rn(q.x2, q.x1), __fsub_rn(q.y2, q.y1));
    return q;
}

// box_utils.boxes_iou_normal for one pair.  The one IoU function of both passes: a recomputed value is bit-identical.
// Rounding intrinsics only, so nothing contracts into an fma; an empty intersection is 0 / union = +0 either way.
__device__ __forceinline__ float aa_iou(const AARect& a, float bx1, float by1, float bx2, float by2, float barea) {
    const float w = fmaxf(__fsub_rn(fminf(a.x2, bx2), fmaxf(a.x1, bx1)), 0.0f);
    const float h = fmaxf(__fsub_rn(fminf(a.y2, by2), fmaxf(a.y1, by1)), 0.0f);
    const float inter = __fmul_rn(w, h);
    if (!(inter > 0.0f)) return 0.0f;
    const float uni = fmaxf(__fsub_rn(__fadd_rn(a.area, barea), inter), 1e-6f);
    return __fdiv_rn(inter, uni);
}

struct AAShared {
    float x1[AA_CHUNK], y1[AA_CHUNK], x2[AA_CHUNK], y2[AA_CHUNK], area[AA_CHUNK];
    int orig[AA_CHUNK];
    int best[AA_CHUNK];      // pass 1: the workgroup's maximum, pass 2: the finished maximum (fp32 bits)
    int wave_cnt[AA_BLOCK / AA_WAVE];
};

// Compacts the gt rows [start, start + AA_CHUNK) of sample `b` that belong to anchor class `c` into LDS, gt order kept.
// Returns how many were kept.  Ends with a barrier.
__device__ __forceinline__ int aa_load_chunk(const AAParams& p, int b, int c, int start, AAShared& s) {
    const int gi = start + (int)threadIdx.x;
    const float* row = p.gt + ((size_t)b * p.n_gt + (gi < p.n_gt ? gi : 0)) * p.gt_stride;
    bool mine = false;
    if (gi < p.n_gt) {
        const int id = (int)row[p.gt_stride - 1];
        mine = id >= 0 && id < p.n_ids && p.slot_of[id] == c;
    }
    const unsigned long long vote = __ballot(mine);
    const int lane = threadIdx.x % AA_WAVE, wave = threadIdx.x / AA_WAVE;
    if (lane == 0) s.wave_cnt[wave] = __popcll(vote);
    __syncthreads();
    int pos = __popcll(vote & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < AA_BLOCK / AA_WAVE; ++w) {
        if (w < wave) pos += s.wave_cnt[w];
        total += s.wave_cnt[w];
    }
    if (mine) {
        const AARect q = aa_rect(row);
        s.x1[pos] = q.x1;
        s.y1[pos] = q.y1;
        s.x2[pos] = q.x2;
        s.y2[pos] = q.y2;
        s.area[pos] = q.area;
        s.orig[pos] = gi;
    }
    __syncthreads();
    return total;
}

// Thread -> anchor of class `c`: `t` runs in OUTPUT order inside the class so that the writes of pass 2 are contiguous.
// Returns the anchor's row in the class table and its output row.
__device__ __forceinline__ void aa_locate(const AAParams& p, const AAClass& k, long long t, long long& mem, long long& out) {
    if (p.multihead) {       // (size, rot, z, y, x) per class, classes back to back
        const long long sr = t / k.locs, loc = t - sr * k.locs;
        mem = loc * k.per_loc + sr;
        out = k.out_base + t;
    } else {                 // (z, y, x, class, size, rot)
        const long long loc = t / k.per_loc, sr = t - loc * k.per_loc;
        mem = t;
        out = loc * p.per_loc_total + k.out_off + sr;
    }
}

__global__ void __launch_bounds__(AA_BLOCK)
anchor_gt_max_kernel(AAParams p, int* __restrict__ gt_max /*[B, M] fp32 bits, zeroed*/) {
    __shared__ AAShared s;
    const int c = blockIdx.y, b = blockIdx.z;
    const AAClass& k = p.cls[c];
    const long long n_cls = (long long)k.locs * k.per_loc;
    const long long t = (long long)blockIdx.x * AA_BLOCK + threadIdx.x;
    if ((long long)blockIdx.x * AA_BLOCK >= n_cls) return;
    const bool live = t < n_cls;
    AARect a = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
        long long mem, out;
        aa_locate(p, k, t, mem, out);
        a = aa_rect(k.anchors + (size_t)mem * p.anchor_stride);
    }
    for (int start = 0; start < p.n_gt; start += AA_CHUNK) {
        const int n = aa_load_chunk(p, b, c, start, s);
        if (threadIdx.x < n) s.best[threadIdx.x] = 0;
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            float v = live ? aa_iou(a, s.x1[j], s.y1[j], s.x2[j], s.y2[j], s.area[j]) : 0.0f;
            if (__ballot(v > 0.0f) == 0ull) continue;       // wave-uniform: most tiles do not touch most gts
            for (int off = AA_WAVE / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, AA_WAVE));
            if (threadIdx.x % AA_WAVE == 0) atomicMax(&s.best[j], __float_as_int(v));
        }
        __syncthreads();
        if ((int)threadIdx.x < n && s.best[threadIdx.x] > 0)
            atomicMax(&gt_max[(size_t)b * p.n_gt + s.orig[threadIdx.x]], s.best[threadIdx.x]);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(AA_BLOCK)
anchor_label_kernel(AAParams p, const int* __restrict__ gt_max, int32_t* __restrict__ labels, float* __restrict__ targets,
                    float* __restrict__ weights) {
    __shared__ AAShared s;
    __shared__ float s_tgt[AA_BLOCK * AA_MAX_CODE];
    __shared__ long long s_out[AA_BLOCK];
    const int c = blockIdx.y, b = blockIdx.z;
    const AAClass& k = p.cls[c];
    const long long n_cls = (long long)k.locs * k.per_loc;
    const long long t = (long long)blockIdx.x * AA_BLOCK + threadIdx.x;
    if ((long long)blockIdx.x * AA_BLOCK >= n_cls) return;
    const bool live = t < n_cls;
    AARect a = {0.f, 0.f, 0.f, 0.f, 0.f};
    long long mem = 0, out = -1;
    if (live) {
        aa_locate(p, k, t, mem, out);
        a = aa_rect(k.anchors + (size_t)mem * p.anchor_stride);
    }
    // argmax over the class's gts in gt order (strict > keeps the lowest index on a tie, like torch.argmax) and the
    // `iou == gt's maximum` broadcast of the reference (a maximum of 0 = the gt touches nothing = matches nothing)
    float best = -1.0f;
    int best_gt = -1;
    bool forced = false;
    for (int start = 0; start < p.n_gt; start += AA_CHUNK) {
        const int n = aa_load_chunk(p, b, c, start, s);
        if ((int)threadIdx.x < n) s.best[threadIdx.x] = gt_max[(size_t)b * p.n_gt + s.orig[threadIdx.x]];
        __syncthreads();
        if (live) {
            for (int j = 0; j < n; ++j) {
                const float v = aa_iou(a, s.x1[j], s.y1[j], s.x2[j], s.y2[j], s.area[j]);
                if (v > best) {
                    best = v;
                    best_gt = s.orig[j];
                }
                forced = forced || (s.best[j] > 0 && __float_as_int(v) == s.best[j]);
            }
        }
        __syncthreads();
    }
    int label = 0;               // a class without gts in this sample: all background
    bool encode = false;
    if (live && best_gt >= 0) {
        const float* g = p.gt + ((size_t)b * p.n_gt + best_gt) * p.gt_stride;
        const int gcls = (int)g[p.gt_stride - 1];
        label = -1;
        if (best >= k.matched) label = gcls;
        encode = forced || label > 0;                       // the reference gathers its foreground before the background pass
        if (best < k.unmatched) label = 0;
        if (forced) label = gcls;
    }
    s_out[threadIdx.x] = out;
    float* row = s_tgt + threadIdx.x * p.code;
    for (int e = 0; e < p.code; ++e) row[e] = 0.0f;
    if (encode) {
        // ResidualCoder.encode_torch; evaluated in fp64 from the fp32 inputs and rounded once
        const float* g = p.gt + ((size_t)b * p.n_gt + best_gt) * p.gt_stride;
        const float* q = k.anchors + (size_t)mem * p.anchor_stride;
        const double dxa = fmaxf(q[3], 1e-5f), dya = fmaxf(q[4], 1e-5f), dza = fmaxf(q[5], 1e-5f);
        const double dxg = fmaxf(g[3], 1e-5f), dyg = fmaxf(g[4], 1e-5f), dzg = fmaxf(g[5], 1e-5f);
        const double diag = sqrt(dxa * dxa + dya * dya);
        row[0] = (float)(((double)g[0] - (double)q[0]) / diag);
        row[1] = (float)(((double)g[1] - (double)q[1]) / diag);
        row[2] = (float)(((double)g[2] - (double)q[2]) / dza);
        row[3] = (float)log(dxg / dxa);
        row[4] = (float)log(dyg / dya);
        row[5] = (float)log(dzg / dza);
        int e = 6;
        if (p.sincos) {
            row[e++] = (float)(cos((double)g[6]) - cos((double)q[6]));
            row[e++] = (float)(sin((double)g[6]) - sin((double)q[6]));
        } else {
            row[e++] = (float)((double)g[6] - (double)q[6]);
        }
        for (int x = 0; x < p.n_extra; ++x) row[e++] = __fsub_rn(g[7 + x], q[7 + x]);
    }
    if (live) {
        labels[(size_t)b * p.n_anchor + out] = label;
        weights[(size_t)b * p.n_anchor + out] = label > 0 ? 1.0f : 0.0f;
    }
    __syncthreads();
    // the target rows of the tile, element by element: consecutive lanes write consecutive floats wherever the output
    // order keeps the tile's rows together (all of it in multi-head order, runs of per_loc rows in single-head order)
    float* dst = targets + (size_t)b * p.n_anchor * p.code;
    for (int e = threadIdx.x; e < AA_BLOCK * p.code; e += AA_BLOCK) {
        const int r = e / p.code;
        const long long o = s_out[r];
        if (o >= 0) dst[(size_t)o * p.code + (e - r * p.code)] = s_tgt[e];
    }
}

}  // namespace toda

using namespace toda;

extern "C" size_t toda_anchor_assign_workspace_bytes(int batch, int n_gt) {
    if (batch < 1 || n_gt < 0) return 0;
    return align_up((size_t)batch * (size_t)(n_gt > 0 ? n_gt : 1) * sizeof(int32_t), 256);
}

extern "C" int toda_anchor_assign(const void* const* anchors_host, const int32_t* locs_host, const int32_t* per_loc_host,
                                  const float* matched_host, const float* unmatched_host, int n_classes, int anchor_stride,
                                  const float* gt_boxes, int batch, int n_gt, int gt_stride, const int32_t* slot_of,
                                  int n_ids, int code_size, int encode_angle_by_sincos, int multihead_order,
                                  int32_t* labels, float* targets, float* weights, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    TODA_CHECK_ARG(n_classes >= 1 && n_classes <= AA_MAX_CLASSES, "anchor_assign: need 1..%d anchor classes, got %d",
                   AA_MAX_CLASSES, n_classes);
    TODA_CHECK_ARG(batch >= 1 && batch <= 65535 && n_gt >= 0, "anchor_assign: need 1 <= batch <= 65535 and n_gt >= 0");
    TODA_CHECK_ARG(anchor_stride >= 7 && gt_stride >= 8, "anchor_assign: anchors need >= 7 columns, gt boxes >= 8");
    TODA_CHECK_ARG(anchors_host && locs_host && per_loc_host && matched_host && unmatched_host,
                   "anchor_assign: null class table");
    const int n_extra = (anchor_stride - 7) < (gt_stride - 8) ? (anchor_stride - 7) : (gt_stride - 8);
    const int want = 6 + (encode_angle_by_sincos ? 2 : 1) + n_extra;
    TODA_CHECK_ARG(code_size == want && code_size <= AA_MAX_CODE,
                   "anchor_assign: code size %d does not match the anchor / gt columns (%d), or is above %d", code_size,
                   want, AA_MAX_CODE);
    TODA_CHECK_ARG(n_ids >= 0 && (n_ids == 0 || slot_of), "anchor_assign: null class-id table");
    TODA_CHECK_ARG(ws_bytes >= toda_anchor_assign_workspace_bytes(batch, n_gt) && ws, "anchor_assign: workspace too small");
    AAParams p;
    long long total = 0, max_cls = 0;
    int per_loc_total = 0;
    for (int c = 0; c < n_classes; ++c) {
        TODA_CHECK_ARG(anchors_host[c] && locs_host[c] >= 1 && per_loc_host[c] >= 1, "anchor_assign: empty anchor class %d", c);
        TODA_CHECK_ARG(multihead_order || locs_host[c] == locs_host[0],
                       "anchor_assign: single-head order needs one feature map size for all classes");
        AAClass& k = p.cls[c];
        k.anchors = (const float*)anchors_host[c];
        k.locs = locs_host[c];
        k.per_loc = per_loc_host[c];
        k.out_off = per_loc_total;
        k.out_base = total;
        k.matched = matched_host[c];
        k.unmatched = unmatched_host[c];
        const long long n = (long long)k.locs * k.per_loc;
        per_loc_total += k.per_loc;
        total += n;
        if (n > max_cls) max_cls = n;
    }
    TODA_CHECK_ARG(total * code_size * batch < (1ll << 40) && max_cls < (1ll << 31) - AA_BLOCK, "anchor_assign: too many anchors");
    TODA_CHECK_ARG(labels && targets && weights && (gt_boxes || n_gt == 0), "anchor_assign: null tensor");
    p.gt = gt_boxes;
    p.slot_of = slot_of;
    p.n_ids = n_ids;
    p.n_gt = n_gt;
    p.gt_stride = gt_stride;
    p.anchor_stride = anchor_stride;
    p.code = code_size;
    p.n_extra = n_extra;
    p.sincos = encode_angle_by_sincos ? 1 : 0;
    p.multihead = multihead_order ? 1 : 0;
    p.per_loc_total = per_loc_total;
    p.n_anchor = total;
    const dim3 grid(cdiv(max_cls, AA_BLOCK), n_classes, batch);
    if (n_gt > 0) {
        TODA_HIP(hipMemsetAsync(ws, 0, (size_t)batch * n_gt * sizeof(int32_t), s));
        hipLaunchKernelGGL(anchor_gt_max_kernel, grid, dim3(AA_BLOCK), 0, s, p, (int*)ws);
        TODA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(anchor_label_kernel, grid, dim3(AA_BLOCK), 0, s, p, (const int*)ws, labels, targets, weights);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
