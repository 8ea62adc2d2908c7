// Adversarial edit of one pseudo-labelled frame for gfx950 (reference pcdet/datasets/nuscenes/nuscenes_mixup_adv_dataset.py
// get_ps_adv_lidar_with_sweeps, :191-274): for every pseudo box one of modify / add / remove on a random subset of the rows the
// box holds, with x' = x - eps * g, g the stored loss gradient of the row's voxel.  The reference computes the box membership
// once, on the frame's coordinates, and then loops over the boxes in numpy (fancy indexing, np.concatenate, a final np.delete);
// here a row's fate depends on the row, the box table and one rank threshold per box, so every pass is one thread per row.
//
//   adv_member      row x box test on the ORIGINAL x, y, z (point_in_box<1>), membership words bits[n, ceil(k / 32)], and the
//                   histogram of the top 8 bits of every member's key             n * 4c bytes in, n * 4 * words out
//   adv_select x 4  per box: scan the 256 bins, fix 8 more bits of the key of rank r_j (the first also forms c_j, k_j, r_j)
//   adv_hist   x 3  the members whose key carries the fixed prefix add the next 8 bits to the box's bins (1 / 256 of them, then
//                   1 / 65536 ...): reads bits only
//   adv_walk<0>     a row through its boxes in table order: keep flag and number of emitted copies -> sc[0:n], sc[n:2n]
//   exclusive scan  over sc[0:2n] (scan.cuh): sc[i] = output row of row i, sc[n + i] = output row of its first copy (the kept
//                   rows come first, so the second half already carries their count), total = output rows
//   adv_walk<1>     the same walk, writing: n * 4c bytes in, (n + copies) * 4c bytes out
//
// The subset: T_j = the r_j = c_j - k_j members smallest in key_j(i) = fmix32(seed_j ^ uint32(i * 0x9E3779B9)).  Multiplication
// by an odd constant, the xor and fmix32 are bijections of uint32, so the keys of a box are pairwise different for i < 2^32 and
// "key <= threshold" selects exactly r_j rows; the (key, i) order of the specification never has to break a tie.  The threshold
// is found by a radix select over the members wherever they lie in memory: no per-box list, nothing held in LDS but 256 bins of
// a scan, so a box with 70 000 rows costs what 70 000 rows in 40 boxes cost.  Integer atomics only: every result is exact and
// the same from run to run.
//
// Arithmetic (-ffp-contract=off): cell = floorf((v - lo) / voxel) in fp32, d = eps * g and cur - d in fp32.  A NaN coordinate
// fails every box test and the cell test, so the row passes through.
#include <string.h>

#include "common.h"
#include "points_common.cuh"
#include "scan.cuh"

namespace toda {

constexpr int ADV_CHUNK = 64;          // boxes staged through LDS at a time = two membership words
constexpr int ADV_MAX_BOXES = 1024;
constexpr int ADV_COLS = 10;           // cx cy cz dx dy dz rz op frac seed
constexpr int ADV_BINS = 256;
static_assert(ADV_BINS == SCAN_BLOCK, "adv_select_kernel: thread t of a SCAN_BLOCK workgroup is bin t, and block_exclusive_scan spans the workgroup");
static_assert(ADV_CHUNK <= PT_BLOCK && ADV_CHUNK % 32 == 0, "adv_member_kernel: one thread stages one box of a chunk; a chunk is whole membership words");
static_assert(ADV_MAX_BOXES >= 512, "NUM_MAX_OBJS of the CenterPoint configs is 500");

enum AdvOp { ADV_MODIFY = 0, ADV_ADD = 1, ADV_REMOVE = 2, ADV_NONE = 3 };

struct AdvBox {            // per box, in the workspace: written by adv_select, read by adv_hist and adv_walk
    uint32_t prefix;       // the fixed high bits of the threshold key; after the fourth select the threshold itself
    int32_t rank;          // rank (1-based) of the threshold among the members that carry the prefix
    int32_t act;           // 0: T_j is empty
    uint32_t seed;
    int32_t op;
    int32_t pad[3];
};

struct AdvGrid {
    float lo[3], voxel[3];
    int32_t grid[3];
    float eps;
};

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ uint32_t adv_key(uint32_t seed, int i) { return fmix32(seed ^ ((uint32_t)i * 0x9E3779B9u)); }

__global__ void __launch_bounds__(PT_BLOCK)
adv_member_kernel(const float* __restrict__ pts, int n, int c, const double* __restrict__ table, int k, int words,
                  uint32_t* __restrict__ bits, int32_t* __restrict__ hist) {
    __shared__ BoxPre sb[ADV_CHUNK];
    __shared__ uint32_t sseed[ADV_CHUNK];
    const int i = pt_row(n, nullptr);
    float x = 0.f, y = 0.f, z = 0.f;
    if (i >= 0) x = pts[(size_t)i * c], y = pts[(size_t)i * c + 1], z = pts[(size_t)i * c + 2];
    for (int base = 0; base < k; base += ADV_CHUNK) {
        const int m = k - base < ADV_CHUNK ? k - base : ADV_CHUNK;
        __syncthreads();
        if ((int)threadIdx.x < m) {
            const double* r = table + (size_t)(base + threadIdx.x) * ADV_COLS;
            BoxPre b;
            b.cx = (float)r[0], b.cy = (float)r[1], b.cz = (float)r[2];
            b.dx = (float)r[3], b.dy = (float)r[4], b.dz = (float)r[5];
            const double a = (double)(-(float)r[6]);
            b.cosa = (float)cos(a);
            b.sina = (float)sin(a);
            sb[threadIdx.x] = b;
            sseed[threadIdx.x] = (uint32_t)r[9];
        }
        __syncthreads();
        if (i < 0) continue;
        for (int h = 0; h < ADV_CHUNK / 32; ++h) {
            if (h * 32 >= m) break;
            uint32_t word = 0;
            const int lim = m - h * 32 < 32 ? m - h * 32 : 32;
            for (int q = 0; q < lim; ++q) {
                const int jb = h * 32 + q;
                if (point_in_box<1>(x, y, z, sb[jb])) {
                    word |= 1u << q;
                    atomicAdd(&hist[(size_t)(base + jb) * ADV_BINS + (adv_key(sseed[jb], i) >> 24)], 1);
                }
            }
            bits[(size_t)i * words + base / 32 + h] = word;
        }
    }
}

// One workgroup per box, thread t = bin t.  pass 0 also forms c_j (written to counts), whether the box acts, and r_j.
__global__ void __launch_bounds__(SCAN_BLOCK)
adv_select_kernel(const double* __restrict__ table, int pass, int32_t* __restrict__ hist, AdvBox* __restrict__ boxes,
                  int32_t* __restrict__ counts) {
    const int j = blockIdx.x, t = threadIdx.x;
    const int h = hist[(size_t)j * ADV_BINS + t];
    hist[(size_t)j * ADV_BINS + t] = 0;
    AdvBox b;
    if (pass) b = boxes[j];                                  // every read before the scan's barriers, the one write after them
    int total;
    const int ex = block_exclusive_scan(h, &total);
    if (pass == 0) {
        const double* r = table + (size_t)j * ADV_COLS;
        b.op = (int)r[7];
        b.seed = (uint32_t)r[9];
        const int cj = total;
        b.act = ((b.op == ADV_MODIFY || b.op == ADV_ADD) && cj >= 1) || (b.op == ADV_REMOVE && cj > 5);
        long long kj = (long long)floor(r[8] * (double)cj);
        if (kj > cj - 1) kj = cj - 1;
        if (kj < 0) kj = 0;
        b.rank = cj - (int)kj;
        b.prefix = 0;
        b.pad[0] = b.pad[1] = b.pad[2] = 0;
        if (t == 0) counts[j] = cj;
        if (!b.act && t == 0) boxes[j] = b;
    }
    if (!b.act) return;
    if (h > 0 && ex < b.rank && b.rank <= ex + h) {          // exactly one bin: 1 <= rank <= total
        b.prefix |= (uint32_t)t << (24 - 8 * pass);
        b.rank -= ex;
        boxes[j] = b;
    }
}

__global__ void __launch_bounds__(PT_BLOCK)
adv_hist_kernel(int n, int words, const uint32_t* __restrict__ bits, const AdvBox* __restrict__ boxes, int pass,
                int32_t* __restrict__ hist) {
    const int i = pt_row(n, nullptr);
    if (i < 0) return;
    const int shift = 24 - 8 * pass;
    for (int w = 0; w < words; ++w) {
        uint32_t word = bits[(size_t)i * words + w];
        while (word) {
            const int q = __ffs(word) - 1;
            word &= word - 1;
            const int j = w * 32 + q;
            const AdvBox b = boxes[j];
            if (!b.act) continue;
            const uint32_t key = adv_key(b.seed, i);
            if ((key >> (shift + 8)) == (b.prefix >> (shift + 8))) atomicAdd(&hist[(size_t)j * ADV_BINS + ((key >> shift) & 255u)], 1);
        }
    }
}

// the stored gradient of the row's voxel times eps; zero outside the grid or for an absent key
__device__ __forceinline__ void adv_displacement(float x, float y, float z, const AdvGrid& g, const int64_t* __restrict__ keys,
                                                 const float* __restrict__ grads, int m, float d[3]) {
    d[0] = d[1] = d[2] = 0.f;
    if (m <= 0) return;
    const float cx = floorf((x - g.lo[0]) / g.voxel[0]), cy = floorf((y - g.lo[1]) / g.voxel[1]), cz = floorf((z - g.lo[2]) / g.voxel[2]);
    if (!(cx >= 0.f && cx < (float)g.grid[0] && cy >= 0.f && cy < (float)g.grid[1] && cz >= 0.f && cz < (float)g.grid[2])) return;
    const long long key = ((long long)cz * g.grid[1] + (long long)cy) * g.grid[0] + (long long)cx;
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < m && keys[lo] == key) {
        d[0] = g.eps * grads[(size_t)lo * 3], d[1] = g.eps * grads[(size_t)lo * 3 + 1], d[2] = g.eps * grads[(size_t)lo * 3 + 2];
    }
}

// WRITE 0: sc[i] = row i is kept, sc[n + i] = number of its copies.  WRITE 1 (sc scanned): the rows themselves.
template <int WRITE>
__global__ void __launch_bounds__(PT_BLOCK)
adv_walk_kernel(const float* __restrict__ pts, int n, int c, int words, const uint32_t* __restrict__ bits,
                const AdvBox* __restrict__ boxes, AdvGrid g, const int64_t* __restrict__ keys, const float* __restrict__ grads, int m,
                int32_t* __restrict__ sc, float* __restrict__ dst, int cap_rows, const int32_t* __restrict__ cursor) {
    const int i = pt_row(n, nullptr);
    if (i < 0) return;
    const float* p = pts + (size_t)i * c;
    float x = p[0], y = p[1], z = p[2];
    float d[3];
    bool have_d = false, marked = false;
    int emitted = 0;
    const long long first = WRITE ? (long long)*cursor : 0;
    for (int w = 0; w < words; ++w) {
        uint32_t word = bits[(size_t)i * words + w];
        while (word) {
            const int q = __ffs(word) - 1;
            word &= word - 1;
            const AdvBox b = boxes[w * 32 + q];
            if (!b.act || adv_key(b.seed, i) > b.prefix) continue;
            if (b.op == ADV_REMOVE) {
                marked = true;
                continue;
            }
            if (!have_d) {
                adv_displacement(p[0], p[1], p[2], g, keys, grads, m, d);
                have_d = true;
            }
            const float nx = x - d[0], ny = y - d[1], nz = z - d[2];
            if (b.op == ADV_MODIFY) {
                x = nx, y = ny, z = nz;
            } else {
                if (WRITE) {
                    const long long row = first + sc[n + i] + emitted;
                    if (row < cap_rows) {
                        float* o = dst + row * c;
                        o[0] = nx, o[1] = ny, o[2] = nz;
                        for (int ch = 3; ch < c; ++ch) o[ch] = p[ch];
                    }
                }
                ++emitted;
            }
        }
    }
    if (!WRITE) {
        sc[i] = marked ? 0 : 1;
        sc[n + i] = emitted;
    } else if (!marked) {
        const long long row = first + sc[i];
        if (row < cap_rows) {
            float* o = dst + row * c;
            o[0] = x, o[1] = y, o[2] = z;
            for (int ch = 3; ch < c; ++ch) o[ch] = p[ch];
        }
    }
}

__global__ void adv_cursor_add_kernel(int32_t* cursor, const int32_t* total) { *cursor += *total; }

struct AdvLayout {
    size_t bits, hist, boxes, sc, partials, total, end;
};

static AdvLayout adv_layout(int n, int k) {
    AdvLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
    const size_t rows = n > 0 ? n : 1, bx = k > 0 ? k : 1;
    L.bits = take(rows * cdiv(bx, 32) * sizeof(uint32_t));
    L.hist = take(bx * ADV_BINS * sizeof(int32_t));
    L.boxes = take(bx * sizeof(AdvBox));
    L.sc = take(2 * rows * sizeof(int32_t));
    L.partials = take(scan_partials_bytes(2 * (long long)rows));
    L.total = take(sizeof(int32_t));
    L.end = o;
    return L;
}

}  // namespace toda

using namespace toda;

extern "C" int toda_adv_edit_max_boxes(void) { return ADV_MAX_BOXES; }
extern "C" int toda_adv_edit_chunk(void) { return ADV_CHUNK; }
extern "C" size_t toda_adv_edit_workspace_bytes(int n, int k) { return adv_layout(n, k).end; }

extern "C" int toda_adv_edit(const float* points, int n, int c, const double* table_host, const double* table_dev, int k,
                             const int64_t* keys, const float* grads, int m, const float* range_lo_host, const float* voxel_host,
                             const int32_t* grid_host, float eps, float* dst, int cap_rows, int32_t* cursor_dev, int32_t* counts,
                             void* ws, size_t ws_bytes, void* stream) {
    TODA_CHECK_ARG(n >= 0 && c >= 4, "adv_edit: need n >= 0 and at least 4 columns (x, y, z and one more)");
    TODA_CHECK_ARG(k >= 0 && k <= ADV_MAX_BOXES && m >= 0 && cap_rows >= 0, "adv_edit: need 0 <= k <= %d boxes, m >= 0 keys and cap_rows >= 0", ADV_MAX_BOXES);
    if (n == 0 || k == 0) return TODA_OK;
    TODA_CHECK_ARG((long long)n * (k + 1) <= 0x7fffffffLL, "adv_edit: n * (k + 1) = %lld rows do not fit the int32 row index", (long long)n * (k + 1));
    TODA_CHECK_ARG(table_host && range_lo_host && voxel_host && grid_host, "adv_edit: null host table, range, voxel size or grid");
    AdvGrid g;
    for (int a = 0; a < 3; ++a) {
        TODA_CHECK_ARG(voxel_host[a] > 0.f && grid_host[a] > 0 && grid_host[a] <= (1 << 20), "adv_edit: voxel sizes must be positive and grid sizes in [1, 2^20]");
        g.lo[a] = range_lo_host[a], g.voxel[a] = voxel_host[a], g.grid[a] = grid_host[a];
    }
    g.eps = eps;
    for (int j = 0; j < k; ++j) {
        const double* r = table_host + (size_t)j * ADV_COLS;
        TODA_CHECK_ARG(r[7] == 0.0 || r[7] == 1.0 || r[7] == 2.0 || r[7] == 3.0, "adv_edit: box %d has op %g, known are 0 modify, 1 add, 2 remove, 3 nothing", j, r[7]);
        TODA_CHECK_ARG(r[8] >= 0.0 && r[8] < 1.0, "adv_edit: box %d has frac %g outside [0, 1)", j, r[8]);
        TODA_CHECK_ARG(r[9] >= 0.0 && r[9] < 4294967296.0 && r[9] == floor(r[9]), "adv_edit: box %d has seed %g, not an integer below 2^32", j, r[9]);
    }
    const AdvLayout L = adv_layout(n, k);
    if (ws_bytes < L.end) {
        set_error("adv_edit: workspace %zu < required %zu", ws_bytes, L.end);
        return TODA_EWORKSPACE;
    }
    TODA_CHECK_ARG(points && table_dev && dst && cursor_dev && counts && ws && ((keys && grads) || m == 0), "adv_edit: null table");
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    uint32_t* bits = (uint32_t*)(w + L.bits);
    int32_t* hist = (int32_t*)(w + L.hist);
    AdvBox* boxes = (AdvBox*)(w + L.boxes);
    int32_t* sc = (int32_t*)(w + L.sc);
    int32_t* total = (int32_t*)(w + L.total);
    const int words = cdiv(k, 32), blocks = cdiv(n, PT_BLOCK);
    TODA_HIP(hipMemsetAsync(hist, 0, (size_t)k * ADV_BINS * sizeof(int32_t), s));
    hipLaunchKernelGGL(adv_member_kernel, dim3(blocks), dim3(PT_BLOCK), 0, s, points, n, c, table_dev, k, words, bits, hist);
    for (int pass = 0; pass < 4; ++pass) {
        if (pass) hipLaunchKernelGGL(adv_hist_kernel, dim3(blocks), dim3(PT_BLOCK), 0, s, n, words, (const uint32_t*)bits, (const AdvBox*)boxes, pass, hist);
        hipLaunchKernelGGL(adv_select_kernel, dim3(k), dim3(SCAN_BLOCK), 0, s, table_dev, pass, hist, boxes, counts);
    }
    TODA_LAUNCH_CHECK();
    hipLaunchKernelGGL(adv_walk_kernel<0>, dim3(blocks), dim3(PT_BLOCK), 0, s, points, n, c, words, (const uint32_t*)bits, (const AdvBox*)boxes, g,
                       keys, grads, m, sc, dst, cap_rows, (const int32_t*)cursor_dev);
    int rc = exclusive_scan(PlainAccess{sc}, 2 * (long long)n, (int32_t*)(w + L.partials), total, s);
    if (rc != TODA_OK) return rc;
    hipLaunchKernelGGL(adv_walk_kernel<1>, dim3(blocks), dim3(PT_BLOCK), 0, s, points, n, c, words, (const uint32_t*)bits, (const AdvBox*)boxes, g,
                       keys, grads, m, sc, dst, cap_rows, (const int32_t*)cursor_dev);
    hipLaunchKernelGGL(adv_cursor_add_kernel, dim3(1), dim3(1), 0, s, cursor_dev, (const int32_t*)total);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
