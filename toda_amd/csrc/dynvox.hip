// Dynamic voxelisation for gfx950: the index, segmented reductions and gather of DynPillarVFE / DynMeanVFE.
//
// The reference (pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:95-141, dynamic_mean_vfe.py:47-76) keeps every in-range
// point, groups the points by cell with torch.unique over an x-major merge key and reduces with torch_scatter (whose CUDA
// scatter_mean / scatter_max use float atomics: the sum order, and so the result, changes from run to run).  Here:
//   1. dv_mark: per point the fp32 cell floor((p - lo) / size), the in-range test, the merge key; the key's bit is set in a
//      bitmap over the key space (integer atomicOr) and the point's keep flag is stored for a compaction scan.
//   2. two device scans: over the bitmap words (rank prefix = the row order of torch.unique) and over the keep flags (the
//      position of a kept point among the kept points = reference `points[mask]`).  M and K end in counts_dev: the host
//      reads them once (ops.read_counts) and sizes the outputs.
//   3. dv_rank: every kept point writes its row: original index, unq_inv = prefix + popcount below its bit, merge key.
//   4. a stable LSD radix sort (8-bit digits, ceil(bits(M - 1) / 8) passes) of (unq_inv, kept row) -> seg_pts: each voxel's
//      kept rows, ascending.  Stable by construction: the rows enter in ascending order and every pass ranks equal digits in
//      input order.  A 60 k-point cell costs what any 60 k points cost.
//   5. dv_heads: segment heads -> seg_off, voxel_coords; dv_counts -> unq_cnt.
// Every reduction after that reads its segment in seg_pts order with one thread per (voxel, column): no atomics, the same
// order on every run, bit-reproducible.  Integer atomics only (bitmap bits, LDS histograms); no float atomic in this file.
// Byte-bound index work: ~70 B per point plus the bitmap (2 bits of words + prefixes per key-space cell, memset per call).
#include "grid_index.cuh"
#include "radix_sort.cuh"

namespace toda {

constexpr int DV_BLOCK = 256;

struct DvGeom {
    float r0[3];
    float vs[3];
    int grid[3];      // cells x y z
    int pillar;       // 1: key (b, x, y), x / y tested; 0: key (b, x, y, z), all three tested
    int batch;
};

static inline long long dv_cells(const DvGeom& g) {
    return (long long)g.grid[0] * g.grid[1] * (g.pillar ? 1 : g.grid[2]);
}

// the merge key of dynamic_pillar_vfe.py:107-109 / dynamic_mean_vfe.py:61-64, or -1 for a dropped point
__device__ __forceinline__ long long dv_key(const float* __restrict__ p, const DvGeom& g) {
    const float bf = p[0];
    if (!(bf >= 0.0f) || !(bf < (float)g.batch)) return -1;        // a batch column outside [0, batch): not a row of this batch
    const int b = (int)bf;
    int cc[3];
    const int axes = g.pillar ? 2 : 3;
    for (int j = 0; j < axes; ++j) {
        const float f = floorf((p[1 + j] - g.r0[j]) / g.vs[j]);
        if (!(f >= 0.0f) || !(f < (float)g.grid[j])) return -1;     // NaN fails both
        cc[j] = (int)f;
    }
    if (g.pillar) return ((long long)b * g.grid[0] + cc[0]) * g.grid[1] + cc[1];
    return (((long long)b * g.grid[0] + cc[0]) * g.grid[1] + cc[1]) * g.grid[2] + cc[2];
}

__global__ void __launch_bounds__(DV_BLOCK)
dv_mark_kernel(const float* __restrict__ pts, int n, int width, DvGeom g, uint2* __restrict__ cells, int32_t* __restrict__ keep_pos) {
    const int i = blockIdx.x * DV_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long key = dv_key(pts + (size_t)i * width, g);
    keep_pos[i] = key >= 0;
    if (key >= 0) gi_set_bit(cells, key);      // a hot cell: once its bit is visible the atomics stop
}

__global__ void __launch_bounds__(DV_BLOCK)
dv_rank_kernel(const float* __restrict__ pts, int n, int width, DvGeom g, const uint2* __restrict__ cells,
               const int32_t* __restrict__ keep_pos, uint8_t* __restrict__ keep, int32_t* __restrict__ rows, int32_t* __restrict__ inv,
               int32_t* __restrict__ sort_key, int32_t* __restrict__ sort_val, long long* __restrict__ row_key) {
    const int i = blockIdx.x * DV_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long key = dv_key(pts + (size_t)i * width, g);
    keep[i] = key >= 0;
    if (key < 0) return;
    const int v = gi_rank(cells, key);      // (its bit is set: dv_mark saw the same key)
    const int r = keep_pos[i];
    rows[r] = i;
    inv[r] = v;
    sort_key[r] = v;
    sort_val[r] = r;
    row_key[r] = key;
}

__global__ void __launch_bounds__(DV_BLOCK)
dv_heads_kernel(const int32_t* __restrict__ skey, const int32_t* __restrict__ sval, const long long* __restrict__ row_key, int k, int m,
                DvGeom g, int32_t* __restrict__ seg_off, int32_t* __restrict__ coords) {
    const int p = blockIdx.x * DV_BLOCK + threadIdx.x;
    if (p >= k) return;
    const int v = skey[p];
    if (p == k - 1) seg_off[m] = k;
    if (p > 0 && skey[p - 1] == v) return;
    seg_off[v] = p;
    const long long key = row_key[sval[p]];
    int b, x, y, z;
    if (g.pillar) {
        const long long plane = (long long)g.grid[0] * g.grid[1];
        b = (int)(key / plane);
        const long long rem = key % plane;
        x = (int)(rem / g.grid[1]);
        y = (int)(rem % g.grid[1]);
        z = 0;
    } else {
        const long long vol = (long long)g.grid[0] * g.grid[1] * g.grid[2];
        b = (int)(key / vol);
        const long long rem = key % vol;
        x = (int)(rem / ((long long)g.grid[1] * g.grid[2]));
        y = (int)((rem / g.grid[2]) % g.grid[1]);
        z = (int)(rem % g.grid[2]);
    }
    int4 o = make_int4(b, z, y, x);
    *reinterpret_cast<int4*>(coords + (size_t)v * 4) = o;
}

__global__ void __launch_bounds__(DV_BLOCK)
dv_counts_kernel(const int32_t* __restrict__ seg_off, int m, int32_t* __restrict__ cnt) {
    const int v = blockIdx.x * DV_BLOCK + threadIdx.x;
    if (v < m) cnt[v] = seg_off[v + 1] - seg_off[v];
}

// ---- segmented reductions, one thread per (voxel, column), the segment read in seg_pts order -------------------------------------
// out[v, c] = sum_{j in seg v} src[row(j), col0 + c] (row(j) = rowmap[seg_pts[j]] or seg_pts[j]); divide: / count (scatter_mean)
__global__ void __launch_bounds__(DV_BLOCK)
dv_seg_sum_kernel(const float* __restrict__ src, int ld, int col0, int ncol, const int32_t* __restrict__ rowmap,
                  const int32_t* __restrict__ seg_off, const int32_t* __restrict__ seg_pts, int m, int divide, float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * DV_BLOCK + threadIdx.x;
    if (t >= (long long)m * ncol) return;
    const int v = (int)(t / ncol), c = (int)(t % ncol);
    const int j0 = seg_off[v], j1 = seg_off[v + 1];
    float s = 0.0f;
    for (int j = j0; j < j1; ++j) {
        int r = seg_pts[j];
        if (rowmap) r = rowmap[r];
        s += src[(size_t)r * ld + col0 + c];
    }
    if (divide) s = s / (float)(j1 - j0);
    out[t] = s;
}

// out[v, c] = max over the segment, arg[v, c] = its row; ties: the first in seg_pts order = the lowest row
__global__ void __launch_bounds__(DV_BLOCK)
dv_seg_max_kernel(const float* __restrict__ x, int c, const int32_t* __restrict__ seg_off, const int32_t* __restrict__ seg_pts, int m,
                  float* __restrict__ out, int32_t* __restrict__ arg) {
    const long long t = (long long)blockIdx.x * DV_BLOCK + threadIdx.x;
    if (t >= (long long)m * c) return;
    const int v = (int)(t / c), col = (int)(t % c);
    const int j0 = seg_off[v], j1 = seg_off[v + 1];
    int best_r = seg_pts[j0];
    float best = x[(size_t)best_r * c + col];
    for (int j = j0 + 1; j < j1; ++j) {
        const int r = seg_pts[j];
        const float val = x[(size_t)r * c + col];
        if (val > best) {
            best = val;
            best_r = r;
        }
    }
    out[t] = best;
    arg[t] = best_r;
}

__global__ void __launch_bounds__(DV_BLOCK)
dv_seg_max_bwd_kernel(const float* __restrict__ gout, const int32_t* __restrict__ arg, int m, int c, float* __restrict__ gx) {
    const long long t = (long long)blockIdx.x * DV_BLOCK + threadIdx.x;
    if (t >= (long long)m * c) return;
    gx[(size_t)arg[t] * c + (t % c)] = gout[t];       // each (row, column) is the argmax of at most one (voxel, column)
}

// out[r, :] = [x[r, :], xmax[inv[r], :]]
__global__ void __launch_bounds__(DV_BLOCK)
dv_gather_concat_kernel(const float* __restrict__ x, const float* __restrict__ xmax, const int32_t* __restrict__ inv, int k, int c,
                        float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * DV_BLOCK + threadIdx.x;
    if (t >= (long long)k * 2 * c) return;
    const int r = (int)(t / (2 * c)), col = (int)(t % (2 * c));
    out[t] = col < c ? x[(size_t)r * c + col] : xmax[(size_t)inv[r] * c + col - c];
}

struct DecoParams {
    float vx, vy, x_off, y_off, z_off;
    int width;        // floats per point row (1 + C)
    int first;        // first copied column: 1 (absolute xyz) or 4
    int with_dist;
    int f;            // output row width
};

// dynamic_pillar_vfe.py:110-129: [points[:, first:], xyz - mean[inv], xyz - centre, (|xyz|)], one thread per kept row
__global__ void __launch_bounds__(DV_BLOCK)
dv_pillar_decorate_kernel(const float* __restrict__ pts, const int32_t* __restrict__ rows, const int32_t* __restrict__ inv,
                          const int32_t* __restrict__ coords, const float* __restrict__ mean, int k, DecoParams d, float* __restrict__ out) {
    const int r = blockIdx.x * DV_BLOCK + threadIdx.x;
    if (r >= k) return;
    const float* p = pts + (size_t)rows[r] * d.width;
    const int v = inv[r];
    float* o = out + (size_t)r * d.f;
    int q = 0;
    for (int j = d.first; j < d.width; ++j) o[q++] = p[j];
    const float x = p[1], y = p[2], z = p[3];
    o[q++] = x - mean[(size_t)v * 3 + 0];
    o[q++] = y - mean[(size_t)v * 3 + 1];
    o[q++] = z - mean[(size_t)v * 3 + 2];
    const int cy = coords[(size_t)v * 4 + 2], cx = coords[(size_t)v * 4 + 3];
    const float xc = (float)cx * d.vx;
    const float yc = (float)cy * d.vy;
    o[q++] = x - (xc + d.x_off);
    o[q++] = y - (yc + d.y_off);
    o[q++] = z - d.z_off;
    if (d.with_dist) o[q++] = sqrtf(x * x + y * y + z * z);
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------
struct DvLayout {
    size_t cells, cells_part, keep_pos, keep_part, row_key, bytes;
    RsLayout sort;
    long long nwords;
};

static DvLayout dv_layout(int n, const DvGeom& g) {
    DvLayout L;
    L.nwords = (dv_cells(g) * g.batch + 31) / 32;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
    L.cells = take((size_t)L.nwords * sizeof(uint2));
    L.cells_part = take(scan_partials_bytes(L.nwords));
    L.keep_pos = take((size_t)(n + 1) * 4);
    L.keep_part = take(scan_partials_bytes(n + 1));
    L.row_key = take((size_t)n * 8);
    L.sort = rs_layout(n, o);
    L.bytes = L.sort.end;
    return L;
}

static int dv_geom(DvGeom* g, const float* range_host, const float* vsize_host, const int32_t* grid_host, int pillar, int batch) {
    TODA_CHECK_ARG(range_host && vsize_host && grid_host, "dynvox: range, voxel size and grid are required");
    TODA_CHECK_ARG(batch >= 1, "dynvox: batch must be >= 1 (got %d)", batch);
    for (int j = 0; j < 3; ++j) {
        TODA_CHECK_ARG(grid_host[j] >= 1, "dynvox: grid must be positive");
        g->r0[j] = range_host[j];
        g->vs[j] = vsize_host[j];
        g->grid[j] = grid_host[j];
    }
    g->pillar = pillar ? 1 : 0;
    g->batch = batch;
    TODA_CHECK_ARG(dv_cells(*g) * batch < (1LL << 40), "dynvox: key space of %lld cells is too large", dv_cells(*g) * batch);
    return TODA_OK;
}

}  // namespace toda

using namespace toda;

extern "C" size_t toda_dynvox_workspace_bytes(int n, int batch, const int32_t* grid_host, int pillar) {
    if (n < 0 || batch < 1 || !grid_host) return 0;
    DvGeom g{};
    for (int j = 0; j < 3; ++j) g.grid[j] = grid_host[j] > 0 ? grid_host[j] : 1;
    g.pillar = pillar ? 1 : 0;
    g.batch = batch;
    return dv_layout(n, g).bytes + 256;
}

extern "C" int toda_dynvox_count(const float* points, int n, int width, int batch, const float* range_host, const float* vsize_host,
                                 const int32_t* grid_host, int pillar, int32_t* counts_dev, void* ws, size_t ws_bytes, void* stream) {
    DvGeom g;
    int rc = dv_geom(&g, range_host, vsize_host, grid_host, pillar, batch);
    if (rc) return rc;
    TODA_CHECK_ARG(n >= 0 && width >= 4, "dynvox: need n >= 0 and rows of >= 4 floats (got n=%d width=%d)", n, width);
    TODA_CHECK_ARG(counts_dev && ws && (n == 0 || points), "dynvox: null pointer");
    const DvLayout L = dv_layout(n, g);
    if (ws_bytes < L.bytes) {
        set_error("dynvox: workspace of %zu bytes, need %zu", ws_bytes, L.bytes);
        return TODA_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    uint2* cells = (uint2*)(w + L.cells);
    int32_t* keep_pos = (int32_t*)(w + L.keep_pos);
    TODA_HIP(hipMemsetAsync(cells, 0, (size_t)L.nwords * sizeof(uint2), s));
    TODA_HIP(hipMemsetAsync(keep_pos, 0, (size_t)(n + 1) * 4, s));
    if (n > 0) hipLaunchKernelGGL(dv_mark_kernel, dim3(cdiv(n, DV_BLOCK)), dim3(DV_BLOCK), 0, s, points, n, width, g, cells, keep_pos);
    TODA_LAUNCH_CHECK();
    rc = exclusive_scan(CellAccess{cells}, L.nwords, (int32_t*)(w + L.cells_part), counts_dev, s);
    if (rc) return rc;
    return exclusive_scan(PlainAccess{keep_pos}, (long long)n + 1, (int32_t*)(w + L.keep_part), counts_dev + 1, s);
}

extern "C" int toda_dynvox_index(const float* points, int n, int width, int batch, const float* range_host, const float* vsize_host,
                                 const int32_t* grid_host, int pillar, int m, int k, uint8_t* keep, int32_t* rows, int32_t* inv,
                                 int32_t* seg_pts, int32_t* seg_off, int32_t* cnt, int32_t* coords, void* ws, size_t ws_bytes,
                                 void* stream) {
    DvGeom g;
    int rc = dv_geom(&g, range_host, vsize_host, grid_host, pillar, batch);
    if (rc) return rc;
    TODA_CHECK_ARG(n >= 0 && width >= 4 && k >= 0 && k <= n && m >= 0 && m <= k && (m > 0) == (k > 0),
                   "dynvox: inconsistent sizes n=%d width=%d k=%d m=%d", n, width, k, m);
    TODA_CHECK_ARG(ws && seg_off && (n == 0 || (points && keep)) && (k == 0 || (rows && inv && seg_pts && cnt && coords)),
                   "dynvox: null pointer");
    const DvLayout L = dv_layout(n, g);
    if (ws_bytes < L.bytes) {
        set_error("dynvox: workspace of %zu bytes, need %zu", ws_bytes, L.bytes);
        return TODA_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    long long* row_key = (long long*)(w + L.row_key);
    if (n > 0)
        hipLaunchKernelGGL(dv_rank_kernel, dim3(cdiv(n, DV_BLOCK)), dim3(DV_BLOCK), 0, s, points, n, width, g, (const uint2*)(w + L.cells),
                           (const int32_t*)(w + L.keep_pos), keep, rows, inv, (int32_t*)(w + L.sort.ka), (int32_t*)(w + L.sort.va), row_key);
    TODA_LAUNCH_CHECK();
    if (k == 0) {
        TODA_HIP(hipMemsetAsync(seg_off, 0, 4, s));
        return TODA_OK;
    }
    const int32_t *skey, *sval;
    rc = radix_sort_pairs(w, L.sort, k, m, &skey, &sval, s);       // keys = unq_inv in [0, m)
    if (rc) return rc;
    TODA_HIP(hipMemcpyAsync(seg_pts, sval, (size_t)k * 4, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(dv_heads_kernel, dim3(cdiv(k, DV_BLOCK)), dim3(DV_BLOCK), 0, s, skey, sval, row_key, k, m, g, seg_off, coords);
    hipLaunchKernelGGL(dv_counts_kernel, dim3(cdiv(m, DV_BLOCK)), dim3(DV_BLOCK), 0, s, seg_off, m, cnt);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_dynvox_seg_sum(const float* src, int ld, int col0, int ncol, const int32_t* rowmap, const int32_t* seg_off,
                                   const int32_t* seg_pts, int m, int divide, float* out, void* stream) {
    TODA_CHECK_ARG(m >= 0 && ncol >= 1 && col0 >= 0 && col0 + ncol <= ld, "dynvox seg_sum: columns %d..%d outside rows of %d", col0,
                   col0 + ncol, ld);
    if (m == 0) return TODA_OK;
    TODA_CHECK_ARG(src && seg_off && seg_pts && out, "dynvox seg_sum: null pointer");
    hipLaunchKernelGGL(dv_seg_sum_kernel, dim3(cdiv((long long)m * ncol, DV_BLOCK)), dim3(DV_BLOCK), 0, (hipStream_t)stream, src, ld, col0,
                       ncol, rowmap, seg_off, seg_pts, m, divide, out);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_dynvox_pillar_decorate(const float* points, int width, const int32_t* rows, const int32_t* inv,
                                           const int32_t* coords, const float* mean, int k, const float* vsize_host,
                                           const float* offset_host, int use_abs_xyz, int with_dist, float* out, int f, void* stream) {
    TODA_CHECK_ARG(width >= 4 && k >= 0 && vsize_host && offset_host, "dynvox decorate: bad arguments");
    DecoParams d;
    d.vx = vsize_host[0];
    d.vy = vsize_host[1];
    d.x_off = offset_host[0];
    d.y_off = offset_host[1];
    d.z_off = offset_host[2];
    d.width = width;
    d.first = use_abs_xyz ? 1 : 4;
    d.with_dist = with_dist ? 1 : 0;
    d.f = f;
    TODA_CHECK_ARG(f == width - d.first + 6 + d.with_dist, "dynvox decorate: row width %d, the decoration makes %d", f,
                   width - d.first + 6 + d.with_dist);
    if (k == 0) return TODA_OK;
    TODA_CHECK_ARG(points && rows && inv && coords && mean && out, "dynvox decorate: null pointer");
    hipLaunchKernelGGL(dv_pillar_decorate_kernel, dim3(cdiv(k, DV_BLOCK)), dim3(DV_BLOCK), 0, (hipStream_t)stream, points, rows, inv, coords,
                       mean, k, d, out);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_dynvox_seg_max_fwd(const float* x, int c, const int32_t* seg_off, const int32_t* seg_pts, int m, float* out,
                                       int32_t* arg, void* stream) {
    TODA_CHECK_ARG(m >= 0 && c >= 1, "dynvox seg_max: bad sizes m=%d c=%d", m, c);
    if (m == 0) return TODA_OK;
    TODA_CHECK_ARG(x && seg_off && seg_pts && out && arg, "dynvox seg_max: null pointer");
    hipLaunchKernelGGL(dv_seg_max_kernel, dim3(cdiv((long long)m * c, DV_BLOCK)), dim3(DV_BLOCK), 0, (hipStream_t)stream, x, c, seg_off,
                       seg_pts, m, out, arg);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_dynvox_seg_max_bwd(const float* gout, const int32_t* arg, int m, int c, int k, float* gx, void* stream) {
    TODA_CHECK_ARG(m >= 0 && c >= 1 && k >= m, "dynvox seg_max bwd: bad sizes m=%d c=%d k=%d", m, c, k);
    if (k == 0) return TODA_OK;
    TODA_CHECK_ARG(gx && (m == 0 || (gout && arg)), "dynvox seg_max bwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    TODA_HIP(hipMemsetAsync(gx, 0, (size_t)k * c * 4, s));
    if (m == 0) return TODA_OK;
    hipLaunchKernelGGL(dv_seg_max_bwd_kernel, dim3(cdiv((long long)m * c, DV_BLOCK)), dim3(DV_BLOCK), 0, s, gout, arg, m, c, gx);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_dynvox_gather_concat(const float* x, const float* xmax, const int32_t* inv, int k, int c, float* out, void* stream) {
    TODA_CHECK_ARG(k >= 0 && c >= 1, "dynvox gather_concat: bad sizes k=%d c=%d", k, c);
    if (k == 0) return TODA_OK;
    TODA_CHECK_ARG(x && xmax && inv && out, "dynvox gather_concat: null pointer");
    hipLaunchKernelGGL(dv_gather_concat_kernel, dim3(cdiv((long long)k * 2 * c, DV_BLOCK)), dim3(DV_BLOCK), 0, (hipStream_t)stream, x, xmax,
                       inv, k, c, out);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
