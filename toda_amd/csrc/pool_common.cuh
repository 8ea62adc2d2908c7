// What voxel_pool.hip and pointnet2_stack.hip share: the relative position of an entry, the fixed-order fold of per-workgroup fp64
// partials, the size checks.  The kernel is static: every translation unit that includes this header compiles its own copy.
#pragma once
#include "common.h"

namespace toda {

constexpr int FOLD_BLOCK = 256;

// relative position of entry (m, s): xyz[row] - new_xyz[m], zero for an empty ball or a row outside the table
__device__ __forceinline__ void rel_delta(const float* __restrict__ xyz, const float* __restrict__ new_xyz, int row, int N, int m,
                                          bool empty, float d[3]) {
    const bool ok = !empty && (unsigned)row < (unsigned)N;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = ok ? xyz[(size_t)row * 3 + k] - new_xyz[(size_t)m * 3 + k] : 0.0f;
}

// out[i] = sum over the nblk workgroups, ascending, of part[b, i], i < n (fold_partials_kernel is dense.hip's BatchNorm fold)
static __global__ void __launch_bounds__(FOLD_BLOCK)
pool_fold_partials_kernel(const double* __restrict__ part, int nblk, int n, float* __restrict__ out) {
    const int i = blockIdx.x * FOLD_BLOCK + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int b = 0; b < nblk; ++b) acc += part[(size_t)b * n + i];
    out[i] = (float)acc;
}

static int pool_check_sizes(const char* what, long long M, int ns, int ns_max, int N, int C) {
    TODA_CHECK_ARG(M >= 0 && N >= 0, "%s: negative sizes (M=%lld N=%d)", what, M, N);
    TODA_CHECK_ARG(ns >= 1 && ns <= ns_max, "%s: nsample %d outside [1, %d]", what, ns, ns_max);
    TODA_CHECK_ARG(C >= 1 && C <= 4096, "%s: channels %d outside [1, 4096]", what, C);
    // the 1-D launches take cdiv(elements, 256) workgroups as an int: keep every element count below 2^38
    TODA_CHECK_ARG(M * ns < (1LL << 31) && M * ns * C < (1LL << 38) && (long long)N * C < (1LL << 38),
                   "%s: too many entries (M=%lld nsample=%d C=%d)", what, M, ns, C);
    return TODA_OK;
}

}  // namespace toda
