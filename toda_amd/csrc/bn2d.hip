// Single-pass BatchNorm2d(+ReLU) for the dense half (BEV neck, CenterHead): training-mode nn.BatchNorm2d on an NCHW fp32
// tensor followed by nn.ReLU (reference pcdet/models/backbones_2d/base_bev_backbone.py:37-58, dense_heads/center_head.py:20-28,73-80).
//
// One 1024-thread workgroup owns ONE channel: its B x H x W values (70 k floats at 2 x 188 x 188) are loaded once into
// registers (<= 18 float4 per thread), the mean and then the centred second moment are reduced from there (fp32 inside a
// thread, fp64 across the workgroup - the two-pass form costs nothing when the data sits in registers), and the normalised,
// rectified result is written straight from the registers: one read and one write of the tensor, no partial-sum buffers,
// no second launch.  Against the MIOpen BatchNorm + clamp pair that is half the traffic forward (72 instead of 144 MB at
// 2 x 128 x 188 x 188).  Backward keeps the masked dy in registers, reduces (sum g, sum g * xhat) while x streams past, then
// streams x a second time (it comes from the L2 / infinity cache: a channel is 283 KB) to write dx: x twice, dy once, dx once
// instead of MIOpen's BatchNorm backward + threshold_backward (216 MB -> 144 MB).  The ReLU mask is recomputed from x with
// the forward's own expression (x * scale + shift, same operation order, -ffp-contract=off), so y is never read back.
// Deterministic: fixed reduction tree, no atomics.
//
// Layout: the vector and reduction helpers; the partner exchange of the per-plane family; the steps every kernel shares, each
// written once (plane load, thread sum, centred squares, the forward map Bn2Map, the masked-dy accumulation, the write-backs); ONE
// forward and ONE backward kernel template <V, BB, K, RELU>, BB = 0 being the per-plane family, with the places where the
// families differ branching on BB in the open; the routing predicates (constexpr); a dispatch that instantiates exactly the
// (V, BB, K) those predicates can reach - 63, times two for RELU.
#include <type_traits>
#include <utility>

#include <stdlib.h>

#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace toda {
constexpr int BN2_BLOCK = 1024;

// sum of v over the workgroup in fp64, broadcast to every thread (two barriers)
__device__ __forceinline__ double bn2_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                    // sh may still be read from the previous call
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < BN2_BLOCK / 64; ++w) t += sh[w];      // same order in every thread
    return t;
}

// A plane (one channel of one sample) as a bounds-checked buffer: lanes past its end read zeros and their stores are dropped,
// so neither kernel has a branch (or an address select) around a memory instruction.  The whole offset goes into the VECTOR
// offset: the range check of a raw buffer covers vector + immediate offset only, a scalar offset would walk into the next plane.
template <int V>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bn2_plane(const float* base, size_t plane, int hwv) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + plane * (size_t)hwv * V), 0, hwv * V * 4, 0x00020000);
}
// V = 4: planes whose size is a multiple of 4 floats (16-byte loads); V = 1: any size, dword loads (a plane then starts at any
// 4-byte boundary).  Same code for both: a "vector" of V floats per load.
template <int V> struct bn2_vec { typedef f32x4 type; };
template <> struct bn2_vec<1> { typedef float type; };
__device__ __forceinline__ float bn2_get(const f32x4& v, int j) { return v[j]; }
__device__ __forceinline__ float bn2_get(const float& v, int) { return v; }
__device__ __forceinline__ void bn2_set(f32x4& v, int j, float a) { v[j] = a; }
__device__ __forceinline__ void bn2_set(float& v, int, float a) { v = a; }
template <int V, int AUX>
__device__ __forceinline__ typename bn2_vec<V>::type bn2_load(__amdgpu_buffer_rsrc_t rs, unsigned voff, int k) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    if constexpr (V == 4)
        return __builtin_bit_cast(f32x4, (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rs, voff + (unsigned)k * (BN2_BLOCK * 16u), 0, AUX));
    else
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff + (unsigned)k * (BN2_BLOCK * 4u), 0, AUX));
}
template <int V>
__device__ __forceinline__ void bn2_store(__amdgpu_buffer_rsrc_t rs, unsigned voff, int k, typename bn2_vec<V>::type v) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    if constexpr (V == 4)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, voff + (unsigned)k * (BN2_BLOCK * 16u), 0, 0);
    else
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs, voff + (unsigned)k * (BN2_BLOCK * 4u), 0, 0);
}
constexpr int BN2_NT = 2;      // aux bit 1 (slc / nt): streamed once

// ---- one workgroup per (channel, sample) plane, partners exchange their partial sums ------------------------------------
// With one workgroup per channel a 128-channel layer occupies half of the 256 CUs and a thread carries batch x K vectors (the
// backward kernel spills at 2 x 188 x 188).  Here the P = batch workgroups of a channel each hold ONE plane, publish two fp64
// partial results to a small workspace (agent-scope atomics: partners may sit on different XCDs whose L2s are not coherent
// for plain accesses) and wait for each other on per-workgroup epoch flags - `epoch` is a number the caller never repeats on a
// workspace, so nothing has to be reset between launches and launches with different channel counts can share it.  Partners
// get neighbouring workgroup ids (same XCD when the channel count is a multiple of 8): dispatch is in id order, so a waiting
// workgroup's partners are resident or next in line - no deadlock however full the GPU is.  Every partner adds the P
// partials in the same order: identical statistics in all of them, run-to-run deterministic.
constexpr int BN2_MAX_SYNC_C = 4096, BN2_MAX_P = 4;
struct Bn2Sync {
    unsigned long long val[BN2_MAX_SYNC_C * BN2_MAX_P][2];
    unsigned flag[BN2_MAX_SYNC_C * BN2_MAX_P];
};

__device__ __forceinline__ void bn2_plane_of_block(int C, int P, int* c, int* b) {
    const int id = blockIdx.x;
    if ((C & 7) == 0) {
        const int slot = id >> 3;
        *b = slot % P;
        *c = (slot / P) * 8 + (id & 7);
    } else {
        *c = id / P;
        *b = id - *c * P;
    }
}

// thread 0 of the block publishes (v0, v1) for (c, b), waits for the P - 1 partners and returns all P pairs through `sh` (LDS, 2 P doubles)
__device__ __forceinline__ void bn2_exchange(Bn2Sync* sy, int c, int b, int P, unsigned epoch, double v0, double v1, double* sh, unsigned* fault) {
    if (threadIdx.x == 0) {
        const int me = c * P + b;
        // relaxed agent-scope atomics only (they go through to memory past the XCD-private caches): a release / acquire pair
        // here means writing back and invalidating the whole L2 around the exchange - measured 8-10 us per kernel
        __hip_atomic_store(&sy->val[me][0], (unsigned long long)__double_as_longlong(v0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sy->val[me][1], (unsigned long long)__double_as_longlong(v1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the two values have left before the flag goes up
        __hip_atomic_store(&sy->flag[me], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int p = 0; p < P; ++p) {
            const int o = c * P + p;
            if (p != b) {
                // bounded: a partner that never becomes resident (fewer CUs than the ordering argument above assumes) must not
                // hang the GPU - after ~2 s the fault word goes up and the launch finishes with invalid statistics
                unsigned polls = 0;
                while (__hip_atomic_load(&sy->flag[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
                    if (++polls > FAULT_SPIN_LIMIT) {
                        fault_raise(fault, TODA_FAULT_BN2D);
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
            }
            asm volatile("" ::: "memory");
            sh[2 * p] = __longlong_as_double((long long)__hip_atomic_load(&sy->val[o][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            sh[2 * p + 1] = __longlong_as_double((long long)__hip_atomic_load(&sy->val[o][1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
    }
    __syncthreads();
}

// ---- the steps of both families and both directions, each written once ----------------------------------------------------
template <int V> using bn2_vec_t = typename bn2_vec<V>::type;

// a plane's K vectors into the register image; AUX is the cache hint
template <int V, int K, int AUX>
__device__ __forceinline__ void bn2_load_plane(bn2_vec_t<V> (&r)[K], __amdgpu_buffer_rsrc_t rs, unsigned voff) {
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = bn2_load<V, AUX>(rs, voff, k);
}
// The next two take one vector, by value: handed the register image by reference the compiler allocates the forward kernels
// differently (up to +21 VGPRs, new scratch at V = 1, BB = 4, K = 18).
// the floats of one vector added in fp32; V = 4 keeps the (r0 + r1) + (r2 + r3) order
template <int V>
__device__ __forceinline__ float bn2_vec_sum(bn2_vec_t<V> v) {
    if constexpr (V == 4) return (v[0] + v[1]) + (v[2] + v[3]);
    else return v;
}
// q + the (x - mean)^2 of vector k of a plane; a vector past the end of the plane holds zeros, not x: masked out
template <int V>
__device__ __forceinline__ float bn2_centred_squares(bn2_vec_t<V> v, int k, int hwv, float mean, float q) {
    const bool ok = (int)threadIdx.x + k * BN2_BLOCK < hwv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float d = ok ? bn2_get(v, j) - mean : 0.f;
        q += d * d;
    }
    return q;
}
// THE forward map.  The forward stores it (rectified or not) and the backward takes its ReLU mask from it: one expression, one
// operation order (-ffp-contract=off), so the mask is the forward's decision bit for bit and y is never read back.
struct Bn2Map {
    float scale, shift;
    __device__ __forceinline__ Bn2Map(float mean, float invstd, float gamma, float beta) : scale(gamma * invstd), shift(beta - mean * scale) {}
    __device__ __forceinline__ float operator()(float x) const { return x * scale + shift; }
};
__device__ __forceinline__ float bn2_xhat(float x, float mean, float invstd) { return (x - mean) * invstd; }
// one vector of the backward's first sweep: gv = dy where the forward let x through, xv = xhat, (s1, s2) += (g, g * xhat)
template <int V, bool RELU>
__device__ __forceinline__ void bn2_mask_dy(bn2_vec_t<V>& xv, bn2_vec_t<V>& gv, const Bn2Map& map, float mean, float invstd, float& s1, float& s2) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float xj = bn2_get(xv, j);
        const float gj = (!RELU || map(xj) > 0.f) ? bn2_get(gv, j) : 0.f;
        const float hj = bn2_xhat(xj, mean, invstd);
        bn2_set(gv, j, gj);
        bn2_set(xv, j, hj);
        s1 += gj;
        s2 += gj * hj;
    }
}

// Kernel arguments, one struct per direction.  P = batch and (sy, epoch, fault) are read by the per-plane instances only.
// y / dy may be a channel slice of a wider tensor (the concatenated BEV map): the pointer is the slice's first plane, yC / gC the
// channel count of the tensor it lives in (= C for a tensor of its own).
struct Bn2Fwd {
    const float* x;
    int C, P, hwv;
    const float *gamma, *beta;
    float *running_mean, *running_var;
    float momentum, eps;
    float* y;
    int yC;
    float* save;
    Bn2Sync* sy;
    unsigned epoch;
    unsigned* fault;
};
struct Bn2Bwd {
    const float *x, *dy;
    int gC, C, P, hwv;
    const float *gamma, *beta, *save;
    float *dx, *dgamma, *dbeta;
    Bn2Sync* sy;
    unsigned epoch;
    unsigned* fault;
};

__device__ __forceinline__ void bn2_write_stats(const Bn2Fwd& a, int c, float mean, float invstd, double var_d, double n) {
    a.save[c] = mean;
    a.save[a.C + c] = invstd;
    if (a.running_mean) {       // as nn.BatchNorm2d: biased variance normalises, the unbiased one goes into the running estimate
        const double unbiased = n > 1.0 ? var_d * n / (n - 1.0) : 0.0;
        a.running_mean[c] = (1.0f - a.momentum) * a.running_mean[c] + a.momentum * mean;
        a.running_var[c] = (1.0f - a.momentum) * a.running_var[c] + a.momentum * (float)unbiased;
    }
}
__device__ __forceinline__ void bn2_write_dparams(const Bn2Bwd& a, int c, double sum_g, double sum_gx) {
    a.dgamma[c] = (float)sum_gx;
    a.dbeta[c] = (float)sum_g;
}

// ---- the two kernels: <V, BB, K, RELU> ------------------------------------------------------------------------------------
// BB = 1, 2, 4: per channel - workgroup c holds the BB planes of channel c.  BB = 0: per plane - a workgroup holds ONE plane and
// exchanges with the P - 1 partners of its channel (the instances a kernel trace shows as bn2d_*_kernel<V, 0, K, RELU>).
template <int BB> constexpr int bn2_planes = BB ? BB : 1;
template <int BB>
__device__ __forceinline__ void bn2_first_plane(int C, int P, int* c, int* b) {
    if constexpr (BB == 0) bn2_plane_of_block(C, P, c, b);
    else *c = blockIdx.x, *b = 0;
}

template <int V, int BB, int K, bool RELU>
__global__ void __launch_bounds__(BN2_BLOCK) bn2d_fwd_kernel(const Bn2Fwd a) {
    constexpr int NB = bn2_planes<BB>;
    __shared__ double sh[BN2_BLOCK / 64];
    int c, b0;
    bn2_first_plane<BB>(a.C, a.P, &c, &b0);
    const unsigned voff = threadIdx.x * (V * 4u);
    bn2_vec_t<V> r[NB][K];
#pragma unroll
    for (int b = 0; b < NB; ++b) bn2_load_plane<V, K, BN2_NT>(r[b], bn2_plane<V>(a.x, (size_t)(b0 + b) * a.C + c, a.hwv), voff);
    // moments of what this workgroup holds, from the registers: mean, then the squares centred on its fp32 rounding
    const double n_wg = (double)NB * a.hwv * V;
    float s = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int k = 0; k < K; ++k) s += bn2_vec_sum<V>(r[b][k]);
    const double mean_wg_d = bn2_block_sum((double)s, sh) / n_wg;
    const float mean_wg = (float)mean_wg_d;
    float q = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int k = 0; k < K; ++k) q = bn2_centred_squares<V>(r[b][k], k, a.hwv, mean_wg, q);
    // sum (x - mean_f)^2 = sum (x - mean_d)^2 + n (mean_d - mean_f)^2: take the rounding of the fp32 mean out again
    const double dm = mean_wg_d - (double)mean_wg;
    const double sum_q = bn2_block_sum((double)q, sh);
    // The one place where the families differ forward.  The two combinations round differently in fp64: both stay.
    double mean_d, var_d, n;
    if constexpr (BB != 0) {
        const double v = sum_q / n_wg - dm * dm;
        mean_d = mean_wg_d, var_d = v > 0.0 ? v : 0.0, n = n_wg;
    } else {
        __shared__ double part[2 * BN2_MAX_P];
        const double m2_b = sum_q - n_wg * dm * dm;        // sum (x - mean_b)^2 of this plane
        // planes -> channel (Chan et al.): mean = sum n_b mean_b / n, M2 = sum M2_b + sum n_b (mean_b - mean)^2; all n_b are equal
        bn2_exchange(a.sy, c, b0, a.P, a.epoch, mean_wg_d, m2_b, part, a.fault);
        mean_d = 0.0;
        for (int p = 0; p < a.P; ++p) mean_d += part[2 * p];
        mean_d /= a.P;
        double m2 = 0.0;
        for (int p = 0; p < a.P; ++p) m2 += part[2 * p + 1] + n_wg * (part[2 * p] - mean_d) * (part[2 * p] - mean_d);
        n = n_wg * a.P;
        var_d = m2 > 0.0 ? m2 / n : 0.0;
    }
    const float mean = (float)mean_d;
    const float invstd = 1.0f / sqrtf((float)var_d + a.eps);
    const Bn2Map map(mean, invstd, a.gamma[c], a.beta[c]);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const __amdgpu_buffer_rsrc_t ry = bn2_plane<V>(a.y, (size_t)(b0 + b) * a.yC + c, a.hwv);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            bn2_vec_t<V> o;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float z = map(bn2_get(r[b][k], j));
                bn2_set(o, j, RELU ? (z > 0.f ? z : 0.f) : z);
            }
            bn2_store<V>(ry, voff, k, o);
        }
    }
    if (threadIdx.x == 0 && b0 == 0) bn2_write_stats(a, c, mean, invstd, var_d, n);      // sample 0's workgroup writes for the channel
}

// The backward's body takes x, dy and dx once more as __restrict__ parameters: struct members cannot promise that the tensors do
// not overlap, and without the promise the second sweep queues every x load behind the dx store before it (measured at V = 1,
// BB = 4, K = 18: 62 -> 78 us).
template <int V, int BB, int K, bool RELU>
__device__ __forceinline__ void bn2_bwd(const Bn2Bwd& a, const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx) {
    constexpr int NB = bn2_planes<BB>;
    constexpr bool PLANE = BB == 0;
    __shared__ double sh[BN2_BLOCK / 64];
    int c, b0;
    bn2_first_plane<BB>(a.C, a.P, &c, &b0);
    const unsigned voff = threadIdx.x * (V * 4u);
    const float mean = a.save[c], invstd = a.save[a.C + c];
    const Bn2Map map(mean, invstd, a.gamma[c], a.beta[c]);
    // The families differ in what they do with x.  Per plane: xhat stays in registers next to the masked dy, nothing is read
    // twice.  Per channel: there is no room for it, x is read un-hinted (kept in the caches) and streamed a second time for dx.
    bn2_vec_t<V> g[NB][K], xh[PLANE ? K : 1];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const __amdgpu_buffer_rsrc_t rx = bn2_plane<V>(x, (size_t)(b0 + b) * a.C + c, a.hwv), rg = bn2_plane<V>(dy, (size_t)(b0 + b) * a.gC + c, a.hwv);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            bn2_vec_t<V> xv = bn2_load<V, PLANE ? BN2_NT : 0>(rx, voff, k);
            bn2_vec_t<V> gv = bn2_load<V, BN2_NT>(rg, voff, k);                // past the end of the plane: zeros
            bn2_mask_dy<V, RELU>(xv, gv, map, mean, invstd, s1, s2);
            g[b][k] = gv;
            if constexpr (PLANE) xh[k] = xv;
            // at most three (x, dy) pairs in flight on top of the g image (128 registers at 16 waves per workgroup)
            else if ((b * K + k) % 3 == 2) __builtin_amdgcn_sched_barrier(0);
        }
    }
    double sum_g = bn2_block_sum((double)s1, sh);
    double sum_gx = bn2_block_sum((double)s2, sh);
    if constexpr (PLANE) {
        __shared__ double part[2 * BN2_MAX_P];
        bn2_exchange(a.sy, c, b0, a.P, a.epoch, sum_g, sum_gx, part, a.fault);
        sum_g = 0.0, sum_gx = 0.0;
        for (int p = 0; p < a.P; ++p) sum_g += part[2 * p], sum_gx += part[2 * p + 1];
    }
    const double n = (double)a.hwv * V * (PLANE ? a.P : BB);
    const float m1 = (float)(sum_g / n), m2 = (float)(sum_gx / n);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const __amdgpu_buffer_rsrc_t rx = bn2_plane<V>(x, (size_t)(b0 + b) * a.C + c, a.hwv), rd = bn2_plane<V>(dx, (size_t)(b0 + b) * a.C + c, a.hwv);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            bn2_vec_t<V> hv;
            if constexpr (PLANE) {
                hv = xh[k];
            } else {
                hv = bn2_load<V, BN2_NT>(rx, voff, k);
#pragma unroll
                for (int j = 0; j < V; ++j) bn2_set(hv, j, bn2_xhat(bn2_get(hv, j), mean, invstd));
            }
            bn2_vec_t<V> o;
#pragma unroll
            for (int j = 0; j < V; ++j) bn2_set(o, j, map.scale * (bn2_get(g[b][k], j) - m1 - bn2_get(hv, j) * m2));
            bn2_store<V>(rd, voff, k, o);
            if constexpr (!PLANE)
                if ((b * K + k) % 3 == 2) __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (threadIdx.x == 0 && b0 == 0) bn2_write_dparams(a, c, sum_g, sum_gx);
}

template <int V, int BB, int K, bool RELU>
__global__ void __launch_bounds__(BN2_BLOCK) bn2d_bwd_kernel(const Bn2Bwd a) {
    bn2_bwd<V, BB, K, RELU>(a, a.x, a.dy, a.dx);
}

// ---- routing: which family serves (batch, hw), as constexpr predicates of (batch, V, K) --------------------------------------
// hw enters only through V (16-byte or dword vectors) and K, the smallest rung of V's ladder >= vectors per plane and thread.
template <int V> struct Bn2Ladder { typedef std::integer_sequence<int, 1, 2, 3, 4, 8, 9> type; };
template <> struct Bn2Ladder<1> { typedef std::integer_sequence<int, 4, 9, 18, 36> type; };
template <int... Ks>
constexpr int bn2_first_rung(int need, std::integer_sequence<int, Ks...>) {
    int k = 0;
    ((k = (k == 0 && Ks >= need) ? Ks : k), ...);
    return k;      // 0: none
}
constexpr int bn2_vec_of(int hw) { return (hw & 3) ? 1 : 4; }
constexpr int bn2_pick_k(int hwv, int v) {
    const int need = (int)(((long long)hwv + BN2_BLOCK - 1) / BN2_BLOCK);
    return v == 4 ? bn2_first_rung(need, Bn2Ladder<4>::type{}) : bn2_first_rung(need, Bn2Ladder<1>::type{});
}
constexpr int bn2_channel_floats(int batch, int v, int k) {      // per channel: the register image of 72 floats per thread; 0: unsupported
    if (!k || !(batch == 1 || batch == 2 || batch == 4)) return 0;
    return batch * k * v <= 72 ? batch * k * v : 0;
}
constexpr bool bn2_plane_fits(int batch, int v, int k) {         // per plane: 36 floats of x (and of dy) per thread
    return (batch == 2 || batch == 4) && k > 0 && k * v <= 36;
}
constexpr int bn2_floats_per_thread(int batch, int hw) {
    if (batch < 1 || hw < 1) return 0;
    return bn2_channel_floats(batch, bn2_vec_of(hw), bn2_pick_k(hw / bn2_vec_of(hw), bn2_vec_of(hw)));
}
constexpr bool bn2_split_ok(int batch, int c, int hw) {
    if (c < 1 || c > BN2_MAX_SYNC_C || hw < 1) return false;
    return bn2_plane_fits(batch, bn2_vec_of(hw), bn2_pick_k(hw / bn2_vec_of(hw), bn2_vec_of(hw)));
}
// per_channel = bn2_floats_per_thread, can_plane = a workspace and an epoch were given and bn2_split_ok
// forward: the exchange costs 2-3 us, the single workgroup per channel only half-fills the GPU on <= 128 channels - measured
// 19.1 vs 21.3 us at 2 x 128 x 188 x 188, 9.9 vs 12.6 at 2 x 256 x 94 x 94: one workgroup per channel wherever it fits
constexpr bool bn2_fwd_per_plane(int per_channel, bool can_plane) { return can_plane && per_channel == 0; }
// backward: per plane when a channel's dy no longer leaves room for anything else in the registers (the channel kernel then
// spills and reads x twice: 51.6 vs 28.5 us at 2 x 128 x 188 x 188; at 2 x 256 x 94 x 94 it is 12.8 vs 17.7 the other way)
constexpr bool bn2_bwd_per_plane(int per_channel, bool can_plane, bool env_split) {
    return can_plane && (per_channel == 0 || (per_channel > 36 && env_split));
}

// Does any call reach <V, BB, K> of this direction?  Per channel: one without a workspace.  Per plane: one with, at batch 2 or 4.
template <class Args, int V, int BB, int K>
constexpr bool bn2_reachable() {
    if (BB) return bn2_channel_floats(BB, V, K) > 0;
    for (int batch : {2, 4}) {
        const int pc = bn2_channel_floats(batch, V, K);
        const bool fits = bn2_plane_fits(batch, V, K);
        if (std::is_same<Args, Bn2Bwd>::value ? bn2_bwd_per_plane(pc, fits, true) : bn2_fwd_per_plane(pc, fits)) return true;
    }
    return false;
}

// ---- dispatch: (v, bb, k, relu) -> the instance, over exactly the reachable ones ---------------------------------------------
template <int V, int BB, int K, bool RELU> constexpr auto bn2_kernel(const Bn2Fwd&) { return &bn2d_fwd_kernel<V, BB, K, RELU>; }
template <int V, int BB, int K, bool RELU> constexpr auto bn2_kernel(const Bn2Bwd&) { return &bn2d_bwd_kernel<V, BB, K, RELU>; }

template <int V, int BB, int K, class Args>
static bool bn2_launch(bool relu, int grid, hipStream_t s, const Args& a) {
    if constexpr (bn2_reachable<Args, V, BB, K>()) {
        hipLaunchKernelGGL((relu ? bn2_kernel<V, BB, K, true>(a) : bn2_kernel<V, BB, K, false>(a)), dim3(grid), dim3(BN2_BLOCK), 0, s, a);
        return true;
    }
    return false;
}
template <int V, int BB, class Args, int... Ks>
static bool bn2_by_k(std::integer_sequence<int, Ks...>, int k, bool relu, int grid, hipStream_t s, const Args& a) {
    return ((k == Ks && bn2_launch<V, BB, Ks>(relu, grid, s, a)) || ...);
}
template <int V, class Args, int... BBs>
static bool bn2_by_bb(std::integer_sequence<int, BBs...>, int bb, int k, bool relu, int grid, hipStream_t s, const Args& a) {
    return ((bb == BBs && bn2_by_k<V, BBs>(typename Bn2Ladder<V>::type{}, k, relu, grid, s, a)) || ...);
}
// bb = 0: per plane, one workgroup per (channel, sample); else bb = batch, one workgroup per channel.  false: no such instance
template <class Args>
static bool bn2_dispatch(int v, int bb, int k, bool relu, hipStream_t s, const Args& a) {
    typedef std::integer_sequence<int, 0, 1, 2, 4> BBs;
    const int grid = bb ? a.C : a.C * a.P;
    return v == 4 ? bn2_by_bb<4>(BBs{}, bb, k, relu, grid, s, a) : bn2_by_bb<1>(BBs{}, bb, k, relu, grid, s, a);
}
}  // namespace toda

using namespace toda;

extern "C" size_t toda_bn2d_sync_bytes(void) { return sizeof(Bn2Sync); }

extern "C" int toda_bn2d_supported(int batch, int c, int hw) {
    return c >= 1 && (bn2_floats_per_thread(batch, hw) > 0 || bn2_split_ok(batch, c, hw)) ? 1 : 0;
}

// a fault raised by an earlier launch (bounded spin gave up) is reported by the next call; the message names the kernels
static int bn2_fault_poll(const char* who) {
    const unsigned v = fault_take();
    if (!v) return TODA_OK;
    toda::set_error("%s: device fault word 0x%x raised by an earlier launch (bounded inter-workgroup wait gave up: %s) - its results are invalid",
                    who, v, fault_names(v));
    return TODA_EFAULT;
}

// y = channels [y_channel0, y_channel0 + c) of a [batch][y_channels][hw] tensor (the deblocks of the BEV neck write straight into the
// concatenated map: reference base_bev_backbone.py:104-107 torch.cat(ups, dim=1))
extern "C" int toda_bn2d_fwd_into(const float* x, int batch, int c, int hw, const float* gamma, const float* beta, float* running_mean,
                                  float* running_var, float momentum, float eps, int relu, float* y, int y_channels, int y_channel0,
                                  float* save, void* sync, unsigned epoch, void* stream) {
    TODA_CHECK_ARG(x && gamma && beta && y && save, "bn2d_fwd: null argument");
    TODA_CHECK_ARG(y_channel0 >= 0 && y_channel0 + c <= y_channels, "bn2d_fwd: channels [%d, %d) outside the %d channels of y", y_channel0,
                   y_channel0 + c, y_channels);
    TODA_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "bn2d_fwd: running_mean and running_var go together");
    if (int rc = bn2_fault_poll("bn2d_fwd")) return rc;
    const int per_channel = bn2_floats_per_thread(batch, hw);
    const bool split = bn2_fwd_per_plane(per_channel, sync != nullptr && epoch != 0 && bn2_split_ok(batch, c, hw));
    TODA_CHECK_ARG(split || per_channel > 0, "bn2d_fwd: unsupported shape (batch %d, channels %d, hw %d)%s", batch, c, hw,
                   sync ? "" : " without a sync workspace");
    const int v = bn2_vec_of(hw), hwv = hw / v;
    const Bn2Fwd a = {x, c, batch, hwv, gamma, beta, running_mean, running_var, momentum, eps, y + (size_t)y_channel0 * hw, y_channels, save,
                      (Bn2Sync*)sync, epoch, split ? fault_word_dev() : nullptr};
    TODA_CHECK_ARG(bn2_dispatch(v, split ? 0 : batch, bn2_pick_k(hwv, v), relu != 0, (hipStream_t)stream, a), "bn2d_fwd: no kernel instance");
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_bn2d_fwd(const float* x, int batch, int c, int hw, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, float momentum, float eps, int relu, float* y, float* save, void* sync, unsigned epoch,
                             void* stream) {
    return toda_bn2d_fwd_into(x, batch, c, hw, gamma, beta, running_mean, running_var, momentum, eps, relu, y, c, 0, save, sync, epoch, stream);
}

// dy = channels [dy_channel0, dy_channel0 + c) of a [batch][dy_channels][hw] gradient (a slice of the concatenated map's gradient)
extern "C" int toda_bn2d_bwd_from(const float* x, const float* dy, int dy_channels, int dy_channel0, int batch, int c, int hw, const float* gamma,
                                  const float* beta, const float* save, int relu, float* dx, float* dgamma, float* dbeta, void* sync,
                                  unsigned epoch, void* stream) {
    TODA_CHECK_ARG(x && dy && gamma && beta && save && dx && dgamma && dbeta, "bn2d_bwd: null argument");
    TODA_CHECK_ARG(dy_channel0 >= 0 && dy_channel0 + c <= dy_channels, "bn2d_bwd: channels [%d, %d) outside the %d channels of dy", dy_channel0,
                   dy_channel0 + c, dy_channels);
    const int per_channel = bn2_floats_per_thread(batch, hw);
    if (int rc = bn2_fault_poll("bn2d_bwd")) return rc;
    // TODA_BN2D_SPLIT=0: never the partner-exchange kernel where the per-channel one exists (it spills there, it cannot wait)
    static const int env_split = getenv("TODA_BN2D_SPLIT") ? atoi(getenv("TODA_BN2D_SPLIT")) : 1;
    const bool split = bn2_bwd_per_plane(per_channel, sync != nullptr && epoch != 0 && bn2_split_ok(batch, c, hw), env_split != 0);
    TODA_CHECK_ARG(split || per_channel > 0, "bn2d_bwd: unsupported shape (batch %d, channels %d, hw %d)%s", batch, c, hw,
                   sync ? "" : " without a sync workspace");
    const int v = bn2_vec_of(hw), hwv = hw / v;
    const Bn2Bwd a = {x, dy + (size_t)dy_channel0 * hw, dy_channels, c, batch, hwv, gamma, beta, save, dx, dgamma, dbeta,
                      (Bn2Sync*)sync, epoch, split ? fault_word_dev() : nullptr};
    TODA_CHECK_ARG(bn2_dispatch(v, split ? 0 : batch, bn2_pick_k(hwv, v), relu != 0, (hipStream_t)stream, a), "bn2d_bwd: no kernel instance");
    TODA_LAUNCH_CHECK();
    return TODA_OK;
}

extern "C" int toda_bn2d_bwd(const float* x, const float* dy, int batch, int c, int hw, const float* gamma, const float* beta,
                             const float* save, int relu, float* dx, float* dgamma, float* dbeta, void* sync, unsigned epoch, void* stream) {
    return toda_bn2d_bwd_from(x, dy, c, 0, batch, c, hw, gamma, beta, save, relu, dx, dgamma, dbeta, sync, epoch, stream);
}
