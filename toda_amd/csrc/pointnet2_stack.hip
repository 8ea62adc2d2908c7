// PV-RCNN's PointNet++ "stack" layer for gfx950 (reference pcdet/ops/pointnet2/pointnet2_stack/src/{sampling,ball_query,
// group_points}_gpu.cu, pointnet2_utils.py, pointnet2_modules.py:60-120, backbones_3d/pfe/voxel_set_abstraction.py:11-42).
//
// Farthest point sampling.  The reference runs one block of T = opt_n_threads(N) threads per sample; thread t owns the points
// k = t (mod T) and keeps the first of its maxima; the block tree halves the width each step and keeps the lower slot on a tie, so
// slot 0 prefers even threads over odd ones, then threads = 0 (mod 4) over = 2 (mod 4), and so on.  The pick of an iteration is
// the point of maximal temp with, among tied maxima, the smallest bit-reversed k mod T (log2 T bits), then the smallest k.  Here
// every point carries the key (temp bits << 32) | ~rank, rank = rev(k mod T) * ceil(N / T) + k / T: temp >= 0, so the largest key
// is the reference's pick whatever the thread layout, and an integer max is all the reduction needs.
//  - toda_fps mode 1, fps_one_kernel: one 1024-thread workgroup per sample re-reads the sample's points and a global temp on
//    every iteration (the reference's algorithm).
//  - toda_fps mode 2, fps_multi_kernel: G co-resident workgroups per sample hold FPS_PPT points per lane and their temp in
//    registers.  Per iteration each workgroup folds its keys, lane 0 publishes them with an agent-scope atomicMax into the
//    iteration's slot and arrives on the sample's monotonic counter (release), waits until all G have arrived (bounded spin,
//    acquire) and reads the slot back.  Both samples' groups run in one launch; the grid is checked against the occupancy
//    query.  A spin that gives up raises TODA_FAULT_FPS and every workgroup leaves the loop (invalid result, no hang).
// Ball query: one lane per query point scans its sample's points in ascending index, tiled through LDS, for up to FPS_MAX_R
// nested radii at once; d2 < r^2 in the reference's order, the first hit fills the row, later hits slots 1.., stop at nsample.
// SA pool pieces (the rest of the layer is GEMMs and ops.bn_rows): the gather z1[e] = P[idx[e]] + W_d . d_e of layer 1, the
// max over nsample with its arg-max, and their backwards: d P through the inverse neighbour table (toda_voxel_pool_table, built in
// voxel_pool.hip for that pool, this gather and the BEV backward), d W_d by the fp64 partials and fold of pool_common.cuh.
// BEV bilinear interpolation: the reference's clamped taps and weight formulas; the backward sums each pixel's taps in the same
// table over pixels.  The file is compiled with contraction off; no float atomics: every result is bit-reproducible.
#include <math.h>

#include "pool_common.cuh"

namespace toda {

constexpr int FPS_ONE_BLOCK = 1024;
constexpr int FPS_BLOCK = 256;
constexpr int FPS_PPT = 16;                  // points per lane of the multi-workgroup kernel
constexpr int FPS_MAX_B = 16;                // samples per launch (the host splits larger batches)
constexpr int FPS_MULTI_MIN_POINTS = 8192;   // auto mode: measured crossover (tools/bench_pv_rcnn.py): groups 1.17x at 8 k, 0.91x at 4 k
constexpr int BQ_BLOCK = 256;
constexpr int BQ_MAX_R = 4;
constexpr int BQ_MAX_NSAMPLE = 128;
constexpr int SA_BLOCK = 256;
constexpr int SA_MAX_NSAMPLE = 254;          // sa_max keeps its arg-max in a byte
constexpr int SB_LANES = 4;
constexpr int SB_BLOCKS = 256;

struct FpsSample {
    int start, n, T, Q, logT;
};

struct FpsPlan {
    FpsSample s[FPS_MAX_B];
    int blk0[FPS_MAX_B + 1];                 // first workgroup of each sample (multi kernel)
    int G[FPS_MAX_B];
    int batch;
};

// the residue r = k mod T with its log2 T bits reversed (an involution): the block tree's preference order
__device__ __forceinline__ unsigned fps_rev(unsigned r, int logT) { return logT ? __brev(r) >> (32 - logT) : 0u; }

__device__ __forceinline__ unsigned long long fps_key(float d, int k, const FpsSample& S) {
    const unsigned rank = fps_rev((unsigned)(k % S.T), S.logT) * (unsigned)S.Q + (unsigned)(k / S.T);
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(0xffffffffu - rank);
}

__device__ __forceinline__ int fps_key_index(unsigned long long key, const FpsSample& S) {
    const unsigned rank = 0xffffffffu - (unsigned)(key & 0xffffffffull);
    return (int)(rank % (unsigned)S.Q) * S.T + (int)fps_rev(rank / (unsigned)S.Q, S.logT);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// block-wide max of one key per lane; every lane gets the result
template <int BLOCK>
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* s_red) {
    v = wave_max_u64(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();                         // s_red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) s_red[wave] = v;
    __syncthreads();
    unsigned long long r = s_red[0];
    for (int w = 1; w < BLOCK / 64; ++w) r = s_red[w] > r ? s_red[w] : r;
    return r;
}

__global__ void __launch_bounds__(FPS_ONE_BLOCK)
fps_one_kernel(const float* __restrict__ xyz, FpsPlan plan, int npoint, float* __restrict__ temp, int* __restrict__ idx) {
    __shared__ unsigned long long s_red[FPS_ONE_BLOCK / 64];
    const FpsSample S = plan.s[blockIdx.x];
    int* out = idx + (size_t)blockIdx.x * npoint;
    if (S.n <= 0) {
        for (int j = threadIdx.x; j < npoint; j += FPS_ONE_BLOCK) out[j] = 0;
        return;
    }
    const float* p = xyz + (size_t)S.start * 3;
    float* t = temp + S.start;
    for (int k = threadIdx.x; k < S.n; k += FPS_ONE_BLOCK) t[k] = 1e10f;
    if (threadIdx.x == 0) out[0] = 0;
    int old = 0;
    for (int j = 1; j < npoint; ++j) {
        const float x1 = p[old * 3 + 0], y1 = p[old * 3 + 1], z1 = p[old * 3 + 2];
        unsigned long long best = 0;
        for (int k = threadIdx.x; k < S.n; k += FPS_ONE_BLOCK) {
            const float dx = p[k * 3 + 0] - x1, dy = p[k * 3 + 1] - y1, dz = p[k * 3 + 2] - z1;
            const float d = dx * dx + dy * dy + dz * dz;
            const float d2 = fminf(d, t[k]);
            t[k] = d2;
            const unsigned long long key = fps_key(d2, k, S);
            best = key > best ? key : best;
        }
        old = fps_key_index(block_max_u64<FPS_ONE_BLOCK>(best, s_red), S);
        if (threadIdx.x == 0) out[j] = old;
    }
}

__global__ void __launch_bounds__(FPS_BLOCK)
fps_multi_kernel(const float* __restrict__ xyz, FpsPlan plan, int npoint, unsigned long long* __restrict__ slots,
                 unsigned* __restrict__ counters, int* __restrict__ idx, unsigned* __restrict__ fault) {
    __shared__ unsigned long long s_red[FPS_BLOCK / 64];
    __shared__ int s_pick, s_abort;
    int b = 0;
    while (b + 1 < plan.batch && (int)blockIdx.x >= plan.blk0[b + 1]) ++b;
    const FpsSample S = plan.s[b];
    const int G = plan.G[b];
    const int g = blockIdx.x - plan.blk0[b];
    const float* p = xyz + (size_t)S.start * 3;
    int* out = idx + (size_t)b * npoint;
    unsigned long long* slot = slots + (size_t)b * npoint;
    unsigned* counter = counters + b;
    float px[FPS_PPT], py[FPS_PPT], pz[FPS_PPT], pt[FPS_PPT];
    const int base = g * FPS_BLOCK * FPS_PPT + threadIdx.x;
#pragma unroll
    for (int i = 0; i < FPS_PPT; ++i) {
        const int k = base + i * FPS_BLOCK;
        const bool ok = k < S.n;
        px[i] = ok ? p[k * 3 + 0] : 0.0f;
        py[i] = ok ? p[k * 3 + 1] : 0.0f;
        pz[i] = ok ? p[k * 3 + 2] : 0.0f;
        pt[i] = ok ? 1e10f : -1.0f;           // lanes past the sample never win (their key is below every real one)
    }
    if (g == 0 && threadIdx.x == 0) out[0] = 0;
    if (threadIdx.x == 0) s_abort = 0;
    int old = 0;
    for (int j = 1; j < npoint; ++j) {
        const float x1 = p[old * 3 + 0], y1 = p[old * 3 + 1], z1 = p[old * 3 + 2];
        unsigned long long best = 0;
#pragma unroll
        for (int i = 0; i < FPS_PPT; ++i) {
            const float dx = px[i] - x1, dy = py[i] - y1, dz = pz[i] - z1;
            const float d = dx * dx + dy * dy + dz * dz;
            if (pt[i] >= 0.0f) {
                pt[i] = fminf(d, pt[i]);
                const unsigned long long key = fps_key(pt[i], base + i * FPS_BLOCK, S);
                best = key > best ? key : best;
            }
        }
        best = block_max_u64<FPS_BLOCK>(best, s_red);
        if (threadIdx.x == 0) {
            __hip_atomic_fetch_max(&slot[j], best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned want = (unsigned)j * (unsigned)G;
            unsigned polls = 0;
            while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
                if (++polls > FAULT_SPIN_LIMIT) {
                    fault_raise(fault, TODA_FAULT_FPS);
                    s_abort = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");     // agent scope: pairs with the partners' release arrivals
            const unsigned long long key = __hip_atomic_load(&slot[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int k = fps_key_index(key, S);
            s_pick = (unsigned)k < (unsigned)S.n ? k : 0;
            if (g == 0) out[j] = s_pick;
        }
        __syncthreads();
        if (s_abort) break;                  // a partner never arrived: leave at once, the fault word says why
        old = s_pick;
    }
}

struct BqArgs {
    int nr;
    float r2[BQ_MAX_R];
    int ns[BQ_MAX_R];
    int* idx[BQ_MAX_R];
    uint8_t* empty[BQ_MAX_R];
};

__global__ void __launch_bounds__(BQ_BLOCK)
ball_query_kernel(const float* __restrict__ xyz, int N, const int* __restrict__ xyz_start, const float* __restrict__ new_xyz,
                  const int* __restrict__ new_start, int B, int M, BqArgs a) {
    __shared__ float s_p[BQ_BLOCK * 3];
    __shared__ int s_lo, s_hi;
    const int m = blockIdx.x * BQ_BLOCK + threadIdx.x;
    if (threadIdx.x == 0) {
        s_lo = 0x7fffffff;
        s_hi = 0;
    }
    __syncthreads();
    int lo = 0, hi = 0;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    int cnt[BQ_MAX_R];
#pragma unroll
    for (int r = 0; r < BQ_MAX_R; ++r) cnt[r] = 0;
    bool active = m < M;
    if (active) {
        int b = 0;
        while (b + 1 < B && m >= new_start[b + 1]) ++b;
        lo = max(0, min(xyz_start[b], N));
        hi = max(lo, min(xyz_start[b + 1], N));
        nx = new_xyz[(size_t)m * 3 + 0];
        ny = new_xyz[(size_t)m * 3 + 1];
        nz = new_xyz[(size_t)m * 3 + 2];
        atomicMin(&s_lo, lo);
        atomicMax(&s_hi, hi);
        active = hi > lo;
    }
    __syncthreads();
    const int wlo = s_lo, whi = s_hi;
    for (int base = wlo; base < whi; base += BQ_BLOCK) {
        if (!__syncthreads_or(active)) break;              // also: the previous tile has been read by every lane
        const int k = base + (int)threadIdx.x;
        if (k < whi) {
            s_p[threadIdx.x * 3 + 0] = xyz[(size_t)k * 3 + 0];
            s_p[threadIdx.x * 3 + 1] = xyz[(size_t)k * 3 + 1];
            s_p[threadIdx.x * 3 + 2] = xyz[(size_t)k * 3 + 2];
        }
        __syncthreads();
        if (active) {
            const int i0 = max(lo - base, 0), i1 = min(hi - base, min(BQ_BLOCK, whi - base));
            for (int i = i0; i < i1 && active; ++i) {
                const float x = s_p[i * 3 + 0], y = s_p[i * 3 + 1], z = s_p[i * 3 + 2];
                const float d2 = (nx - x) * (nx - x) + (ny - y) * (ny - y) + (nz - z) * (nz - z);
                bool full = true;
                for (int r = 0; r < a.nr; ++r) {
                    const int ns = a.ns[r];
                    if (cnt[r] < ns && d2 < a.r2[r]) {
                        int* row = a.idx[r] + (size_t)m * ns;
                        if (cnt[r] == 0)
                            for (int l = 1; l < ns; ++l) row[l] = base + i;
                        row[cnt[r]++] = base + i;
                    }
                    full = full && cnt[r] >= ns;
                }
                active = !full;
            }
        }
    }
    if (m < M) {
        for (int r = 0; r < a.nr; ++r) {
            if (cnt[r] == 0) {
                int* row = a.idx[r] + (size_t)m * a.ns[r];
                for (int l = 0; l < a.ns[r]; ++l) row[l] = 0;
            }
            a.empty[r][m] = cnt[r] == 0;
        }
    }
}

// z [E, C], E = M x ns: z[e, c] = P[idx[e], c] + wd[c] . d_e, 0 for an empty ball
__global__ void __launch_bounds__(SA_BLOCK)
sa_gather_fwd_kernel(const float* __restrict__ P, int N, int C, const float* __restrict__ wd, const int* __restrict__ idx,
                     const uint8_t* __restrict__ empty, int ns, long long E, const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                     float* __restrict__ z) {
    const long long i = (long long)blockIdx.x * SA_BLOCK + threadIdx.x;
    if (i >= E * C) return;
    const long long e = i / C;
    const int c = (int)(i - e * C);
    const int m = (int)(e / ns);
    const int row = idx[e];
    const bool ok = !empty[m] && (unsigned)row < (unsigned)N;
    float v = 0.0f;
    if (ok) {
        float d[3];
        rel_delta(xyz, new_xyz, row, N, m, false, d);
        v = P[(size_t)row * C + c] + (wd[c * 3 + 0] * d[0] + wd[c * 3 + 1] * d[1] + wd[c * 3 + 2] * d[2]);
    }
    z[i] = v;
}

// gP[n, c] = sum of gz[e, c] over the entries e of row n, in table order
__global__ void __launch_bounds__(SA_BLOCK)
sa_gather_bwd_feat_kernel(const float* __restrict__ gz, int C, const int32_t* __restrict__ off, const int32_t* __restrict__ ent, int N,
                          float* __restrict__ gP) {
    const long long i = (long long)blockIdx.x * SA_BLOCK + threadIdx.x;
    if (i >= (long long)N * C) return;
    const int n = (int)(i / C), c = (int)(i % C);
    float acc = 0.0f;
    for (int j = off[n], end = off[n + 1]; j < end; ++j) acc += gz[(size_t)ent[j] * C + c];
    gP[i] = acc;
}

// gwd[c, k] = sum_e gz[e, c] d_e[k]: lanes (entry lane, channel), fp64, a fixed set of entries per lane
__global__ void __launch_bounds__(SA_BLOCK)
sa_gather_bwd_pos_kernel(const float* __restrict__ gz, const int* __restrict__ idx, const uint8_t* __restrict__ empty, int ns, long long E,
                         int C, const float* __restrict__ xyz, int N, const float* __restrict__ new_xyz, double* __restrict__ part) {
    __shared__ double s_red[3][SA_BLOCK];
    const int lane = threadIdx.x / 64, c = blockIdx.y * 64 + (threadIdx.x & 63);
    double v[3] = {0, 0, 0};
    if (c < C) {
        for (long long e = (long long)blockIdx.x * SB_LANES + lane; e < E; e += (long long)gridDim.x * SB_LANES) {
            const int m = (int)(e / ns);
            if (empty[m]) continue;
            float d[3];
            rel_delta(xyz, new_xyz, idx[e], N, m, false, d);
            const double g = gz[(size_t)e * C + c];
            v[0] += g * d[0];
            v[1] += g * d[1];
            v[2] += g * d[2];
        }
    }
    for (int k = 0; k < 3; ++k) s_red[k][threadIdx.x] = v[k];
    __syncthreads();
    if (lane == 0 && c < C) {
        for (int k = 0; k < 3; ++k) {
            double acc = s_red[k][threadIdx.x];
            for (int l = 1; l < SB_LANES; ++l) acc += s_red[k][l * 64 + threadIdx.x];
            part[((size_t)blockIdx.x * C + c) * 3 + k] = acc;
        }
    }
}

// out[m, c] = max_s y[m, s, c], arg = first arg-max s whatever its sign (F.max_pool2d's gradient; the ReLU before it is an op of
// its own and masks its zeros in its own backward)
__global__ void __launch_bounds__(SA_BLOCK)
sa_max_fwd_kernel(const float* __restrict__ y, int M, int ns, int C, float* __restrict__ out, uint8_t* __restrict__ arg) {
    const long long i = (long long)blockIdx.x * SA_BLOCK + threadIdx.x;
    if (i >= (long long)M * C) return;
    const long long m = i / C;
    const int c = (int)(i - m * C);
    const float* p = y + (size_t)m * ns * C + c;
    float best = p[0];
    int at = 0;
    for (int s = 1; s < ns; ++s) {
        const float v = p[(size_t)s * C];
        if (v > best) {
            best = v;
            at = s;
        }
    }
    out[i] = best;
    if (arg) arg[i] = (uint8_t)at;
}

__global__ void __launch_bounds__(SA_BLOCK)
sa_max_bwd_kernel(const float* __restrict__ g, const uint8_t* __restrict__ arg, int M, int ns, int C, float* __restrict__ gy) {
    const long long i = (long long)blockIdx.x * SA_BLOCK + threadIdx.x;
    if (i >= (long long)M * ns * C) return;
    const long long e = i / C;
    const int c = (int)(i - e * C);
    const long long m = e / ns;
    const int s = (int)(e - m * ns);
    const size_t o = (size_t)m * C + c;
    gy[i] = arg[o] == s ? g[o] : 0.0f;
}

// out [K, C] from map [B, C, H, W] at (x, y) [K, 2] of sample bidx[k]; taps [K, 4] = pixel (b H + y) W + x of Ia Ib Ic Id, w the weights
__global__ void __launch_bounds__(SA_BLOCK)
bev_interp_fwd_kernel(const float* __restrict__ map, int B, int C, int H, int W, const float* __restrict__ xy, const int* __restrict__ bidx,
                      int K, float* __restrict__ out, int* __restrict__ taps, float* __restrict__ wts) {
    const long long i = (long long)blockIdx.x * SA_BLOCK + threadIdx.x;
    if (i >= (long long)K * C) return;
    const int k = (int)(i / C), c = (int)(i % C);
    const float x = xy[k * 2 + 0], y = xy[k * 2 + 1];
    const float fx = floorf(x), fy = floorf(y);
    const float x0 = fminf(fmaxf(fx, 0.0f), (float)(W - 1)), x1 = fminf(fmaxf(fx + 1.0f, 0.0f), (float)(W - 1));
    const float y0 = fminf(fmaxf(fy, 0.0f), (float)(H - 1)), y1 = fminf(fmaxf(fy + 1.0f, 0.0f), (float)(H - 1));
    const float wa = (x1 - x) * (y1 - y);
    const float wb = (x1 - x) * (y - y0);
    const float wc = (x - x0) * (y1 - y);
    const float wd = (x - x0) * (y - y0);
    const int b = min(max(bidx[k], 0), B - 1);
    const int ix0 = (int)x0, ix1 = (int)x1, iy0 = (int)y0, iy1 = (int)y1;
    const float* pl = map + ((size_t)b * C + c) * H * W;
    const float ia = pl[(size_t)iy0 * W + ix0], ib = pl[(size_t)iy1 * W + ix0], ic = pl[(size_t)iy0 * W + ix1], id = pl[(size_t)iy1 * W + ix1];
    out[i] = ia * wa + ib * wb + ic * wc + id * wd;
    if (c == 0 && taps) {
        const int pb = b * H;
        taps[k * 4 + 0] = (pb + iy0) * W + ix0;
        taps[k * 4 + 1] = (pb + iy1) * W + ix0;
        taps[k * 4 + 2] = (pb + iy0) * W + ix1;
        taps[k * 4 + 3] = (pb + iy1) * W + ix1;
        wts[k * 4 + 0] = wa;
        wts[k * 4 + 1] = wb;
        wts[k * 4 + 2] = wc;
        wts[k * 4 + 3] = wd;
    }
}

// gmap [B, C, H, W]: per pixel, its taps (table order = ascending k, tap) times the keypoints' gradients
__global__ void __launch_bounds__(SA_BLOCK)
bev_interp_bwd_kernel(const float* __restrict__ g, int C, const int32_t* __restrict__ off, const int32_t* __restrict__ ent,
                      const float* __restrict__ wts, int B, int H, int W, float* __restrict__ gmap) {
    const long long i = (long long)blockIdx.x * SA_BLOCK + threadIdx.x;
    const long long HW = (long long)H * W;
    if (i >= (long long)B * C * HW) return;
    const long long pix = i % HW;
    const long long bc = i / HW;
    const int c = (int)(bc % C), b = (int)(bc / C);
    const long long p = (long long)b * HW + pix;
    float acc = 0.0f;
    for (int j = off[p], end = off[p + 1]; j < end; ++j) {
        const int e = ent[j];
        acc += g[(size_t)(e >> 2) * C + c] * wts[e];
    }
    gmap[i] = acc;
}

// T = opt_n_threads(n) of sampling_gpu.cu:9-13, in its double arithmetic
static int fps_threads(int n) {
    const int pow_2 = (int)(std::log((double)n) / std::log(2.0));
    int t = 1 << pow_2;
    t = t < 1024 ? t : 1024;
    return t > 1 ? t : 1;
}

// co-resident workgroups of fps_multi_kernel on the current device: CUs x the occupancy query's blocks per CU, minus one block per
// CU (ROCm's query is advisory and has been seen to over-report by one block per CU for 256-thread kernels), at most 4 per CU
static int fps_resident_blocks() {
    constexpr int MAX_DEV = 64;
    static int cached[MAX_DEV] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) {
        (void)hipGetLastError();
        return 0;
    }
    if (dev < MAX_DEV && cached[dev] > 0) return cached[dev];
    int per = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fps_multi_kernel, FPS_BLOCK, 0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    per = per > 1 ? per - 1 : per;
    per = per > 4 ? 4 : per;
    const int blocks = cu_count() * per;
    if (dev < MAX_DEV) cached[dev] = blocks;
    return blocks;
}

}  // namespace toda

using namespace toda;

extern "C" int toda_fps_resident_blocks(void) { return fps_resident_blocks(); }

extern "C" size_t toda_fps_workspace_bytes(int batch, int npoint) {
    if (batch < 1 || npoint < 1) return 0;
    return align_up((size_t)batch * npoint * 8, 256) + align_up((size_t)batch * 4, 256);
}

extern "C" int toda_fps(const float* xyz, const int32_t* starts_host, int batch, int npoint, int mode, float* temp, int32_t* idx, void* ws,
                        size_t ws_bytes, void* stream) {
    TODA_CHECK_ARG(batch >= 1 && npoint >= 1, "fps: batch=%d npoint=%d", batch, npoint);
    TODA_CHECK_ARG(mode >= 0 && mode <= 2, "fps: mode %d (0 auto, 1 one workgroup per sample, 2 workgroup groups)", mode);
    TODA_CHECK_ARG(starts_host && idx, "fps: null pointer");
    const long long total = starts_host[batch];
    TODA_CHECK_ARG(starts_host[0] == 0 && total < (1LL << 31), "fps: sample offsets must start at 0");
    for (int b = 0; b < batch; ++b) TODA_CHECK_ARG(starts_host[b + 1] >= starts_host[b], "fps: sample offsets must not decrease");
    TODA_CHECK_ARG(total == 0 || xyz, "fps: null points");
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < batch; b0 += FPS_MAX_B) {
        const int nb = batch - b0 < FPS_MAX_B ? batch - b0 : FPS_MAX_B;
        FpsPlan plan;
        plan.batch = nb;
        int blocks = 0, nmax = 0;
        for (int i = 0; i < nb; ++i) {
            const int n = starts_host[b0 + i + 1] - starts_host[b0 + i];
            const int T = n > 0 ? fps_threads(n) : 1;
            int logT = 0;
            while ((1 << logT) < T) ++logT;
            plan.s[i] = FpsSample{starts_host[b0 + i], n, T, n > 0 ? (n + T - 1) / T : 1, logT};
            plan.G[i] = n > 0 ? cdiv(n, FPS_BLOCK * FPS_PPT) : 1;
            plan.blk0[i] = blocks;
            blocks += plan.G[i];
            nmax = n > nmax ? n : nmax;
        }
        plan.blk0[nb] = blocks;
        int use = mode;
        if (use == 0) use = nmax >= FPS_MULTI_MIN_POINTS ? 2 : 1;
        if (use == 2) {
            bool empty_sample = false;
            for (int i = 0; i < nb; ++i) empty_sample = empty_sample || plan.s[i].n == 0;
            const int cap = fps_resident_blocks();
            if (blocks > cap || empty_sample) {
                TODA_CHECK_ARG(mode == 0, "fps: %d workgroups do not fit the %d co-resident ones (or a sample is empty)", blocks, cap);
                use = 1;
            }
        }
        int32_t* out = idx + (size_t)b0 * npoint;
        if (use == 1) {
            TODA_CHECK_ARG(total == 0 || temp, "fps: the one-workgroup kernel needs temp [N]");
            hipLaunchKernelGGL(fps_one_kernel, dim3(nb), dim3(FPS_ONE_BLOCK), 0, s, xyz, plan, npoint, temp, (int*)out);
        } else {
            const size_t need = toda_fps_workspace_bytes(nb, npoint);
            if (!ws || ws_bytes < need) {
                set_error("fps: workspace of %zu bytes, need %zu", ws_bytes, need);
                return TODA_EWORKSPACE;
            }
            unsigned long long* slots = (unsigned long long*)ws;
            unsigned* counters = (unsigned*)((char*)ws + align_up((size_t)nb * npoint * 8, 256));
            TODA_HIP(hipMemsetAsync(ws, 0, need, s));
            hipLaunchKernelGGL(fps_multi_kernel, dim3(blocks), dim3(FPS_BLOCK), 0, s, xyz, plan, npoint, slots, counters, (int*)out,
                               fault_word_dev());
        }
        TODA_LAUNCH_CHECK();
    }
    return TODA_OK;
}

extern "C" int toda_ball_query_stack(const float* xyz, int N, const int32_t* xyz_start, const float* new_xyz, const int32_t* new_start,
                                     int batch, int M, int nr, const float* radii_host, const int32_t* nsample_host, int32_t* const* idx_host,
                                     uint8_t* const* empty_host, void* stream) {
    TODA_CHECK_ARG(N >= 0 && M >= 0 && batch >= 1, "ball_query_stack: N=%d M=%d batch=%d", N, M, batch);
    TODA_CHECK_ARG(nr >= 1 && nr <= BQ_MAX_R, "ball_query_stack: %d radii outside [1, %d]", nr, BQ_MAX_R);
    TODA_CHECK_ARG(radii_host && nsample_host && idx_host && empty_host, "ball_query_stack: null pointer");
    BqArgs a;
    a.nr = nr;
    for (int r = 0; r < nr; ++r) {
        TODA_CHECK_ARG(nsample_host[r] >= 1 && nsample_host[r] <= BQ_MAX_NSAMPLE, "ball_query_stack: nsample %d outside [1, %d]",
                       nsample_host[r], BQ_MAX_NSAMPLE);
        TODA_CHECK_ARG(radii_host[r] >= 0.0f, "ball_query_stack: negative radius");
        TODA_CHECK_ARG((long long)M * nsample_host[r] < (1LL << 31), "ball_query_stack: M x nsample too large");
        a.r2[r] = radii_host[r] * radii_host[r];           // fp32, as ball_query_gpu.cu
        a.ns[r] = nsample_host[r];
        a.idx[r] = (int*)idx_host[r];
        a.empty[r] = empty_host[r];
        TODA_CHECK_ARG(M == 0 || (a.idx[r] && a.empty[r]), "ball_query_stack: null output");
    }
    for (int r = nr; r < BQ_MAX_R; ++r) {
        a.r2[r] = 0.0f;
        a.ns[r] = 1;
        a.idx[r] = nullptr;
        a.empty[r] = nullptr;
    }
    if (M == 0) return TODA_OK;
    TODA_CHECK_ARG(new_xyz && xyz_start && new_start && (N == 0 || xyz), "ball_query_stack: null pointer");
    hipLaunchKernelGGL(ball_query_kernel, dim3(cdiv(M, BQ_BLOCK)), dim3(BQ_BLOCK), 0, (hipStream_t)stream, xyz, N, (const int*)xyz_start,
                       new_xyz, (const int*)new_start, batch, M, a);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_sa_gather_fwd(const float* P, int N, int C, const float* wd, const int32_t* idx, const uint8_t* empty, int M, int nsample,
                                  const float* xyz, const float* new_xyz, float* z, void* stream) {
    int rc = pool_check_sizes("sa_gather_fwd", M, nsample, SA_MAX_NSAMPLE, N, C);
    if (rc) return rc;
    if (M == 0) return TODA_OK;
    TODA_CHECK_ARG(wd && idx && empty && new_xyz && z && (N == 0 || (P && xyz)), "sa_gather_fwd: null pointer");
    const long long E = (long long)M * nsample;
    hipLaunchKernelGGL(sa_gather_fwd_kernel, dim3(cdiv(E * C, SA_BLOCK)), dim3(SA_BLOCK), 0, (hipStream_t)stream, P, N, C, wd, (const int*)idx,
                       empty, nsample, E, xyz, new_xyz, z);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_sa_gather_bwd_feat(const float* gz, int M, int nsample, int C, const int32_t* off, const int32_t* ent, int N, float* gP,
                                       void* stream) {
    int rc = pool_check_sizes("sa_gather_bwd_feat", M, nsample, SA_MAX_NSAMPLE, N, C);
    if (rc) return rc;
    if (N == 0) return TODA_OK;
    TODA_CHECK_ARG(off && gP && (M == 0 || (gz && ent)), "sa_gather_bwd_feat: null pointer");
    hipLaunchKernelGGL(sa_gather_bwd_feat_kernel, dim3(cdiv((long long)N * C, SA_BLOCK)), dim3(SA_BLOCK), 0, (hipStream_t)stream, gz, C, off,
                       ent, N, gP);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" size_t toda_sa_gather_bwd_pos_doubles(int C) { return C < 1 ? 0 : (size_t)SB_BLOCKS * C * 3; }

extern "C" int toda_sa_gather_bwd_pos(const float* gz, const int32_t* idx, const uint8_t* empty, int M, int nsample, int C, const float* xyz,
                                      int N, const float* new_xyz, double* ws, float* gwd, void* stream) {
    int rc = pool_check_sizes("sa_gather_bwd_pos", M, nsample, SA_MAX_NSAMPLE, N, C);
    if (rc) return rc;
    TODA_CHECK_ARG(ws && gwd && (M == 0 || (gz && idx && empty && new_xyz)) && (N == 0 || xyz), "sa_gather_bwd_pos: null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sa_gather_bwd_pos_kernel, dim3(SB_BLOCKS, cdiv(C, 64)), dim3(SA_BLOCK), 0, s, gz, (const int*)idx, empty, nsample,
                       (long long)M * nsample, C, xyz, N, new_xyz, ws);
    hipLaunchKernelGGL(pool_fold_partials_kernel, dim3(cdiv(C * 3, FOLD_BLOCK)), dim3(FOLD_BLOCK), 0, s, (const double*)ws, SB_BLOCKS, C * 3, gwd);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_sa_max_fwd(const float* y, int M, int nsample, int C, float* out, uint8_t* arg, void* stream) {
    int rc = pool_check_sizes("sa_max_fwd", M, nsample, SA_MAX_NSAMPLE, 0, C);
    if (rc) return rc;
    if (M == 0) return TODA_OK;
    TODA_CHECK_ARG(y && out, "sa_max_fwd: null pointer");
    hipLaunchKernelGGL(sa_max_fwd_kernel, dim3(cdiv((long long)M * C, SA_BLOCK)), dim3(SA_BLOCK), 0, (hipStream_t)stream, y, M, nsample, C, out,
                       arg);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_sa_max_bwd(const float* g, const uint8_t* arg, int M, int nsample, int C, float* gy, void* stream) {
    int rc = pool_check_sizes("sa_max_bwd", M, nsample, SA_MAX_NSAMPLE, 0, C);
    if (rc) return rc;
    if (M == 0) return TODA_OK;
    TODA_CHECK_ARG(g && arg && gy, "sa_max_bwd: null pointer");
    hipLaunchKernelGGL(sa_max_bwd_kernel, dim3(cdiv((long long)M * nsample * C, SA_BLOCK)), dim3(SA_BLOCK), 0, (hipStream_t)stream, g, arg, M,
                       nsample, C, gy);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_bev_interp_fwd(const float* map, int B, int C, int H, int W, const float* xy, const int32_t* bidx, int K, float* out,
                                   int32_t* taps, float* wts, void* stream) {
    TODA_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1 && K >= 0, "bev_interp_fwd: B=%d C=%d H=%d W=%d K=%d", B, C, H, W, K);
    TODA_CHECK_ARG((long long)B * H * W < (1LL << 31) && (long long)K * C < (1LL << 38) && (long long)K * 4 < (1LL << 31),
                   "bev_interp_fwd: too large");
    if (K == 0) return TODA_OK;
    TODA_CHECK_ARG(map && xy && bidx && out && (!taps || wts), "bev_interp_fwd: null pointer");
    hipLaunchKernelGGL(bev_interp_fwd_kernel, dim3(cdiv((long long)K * C, SA_BLOCK)), dim3(SA_BLOCK), 0, (hipStream_t)stream, map, B, C, H, W,
                       xy, (const int*)bidx, K, out, (int*)taps, wts);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_bev_interp_bwd(const float* g, int K, int C, const int32_t* off, const int32_t* ent, const float* wts, int B, int H, int W,
                                   float* gmap, void* stream) {
    TODA_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1 && K >= 0, "bev_interp_bwd: B=%d C=%d H=%d W=%d K=%d", B, C, H, W, K);
    TODA_CHECK_ARG((long long)B * H * W < (1LL << 31) && (long long)B * C * H * W < (1LL << 38), "bev_interp_bwd: too large");
    TODA_CHECK_ARG(off && gmap && (K == 0 || (g && ent && wts)), "bev_interp_bwd: null pointer");
    hipLaunchKernelGGL(bev_interp_bwd_kernel, dim3(cdiv((long long)B * C * H * W, SA_BLOCK)), dim3(SA_BLOCK), 0, (hipStream_t)stream, g, C, off,
                       ent, wts, B, H, W, gmap);
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}
