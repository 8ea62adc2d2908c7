// The fixed-order fold of per-workgroup partial sums and the BatchNorm statistics bookkeeping of dense.hip, each written once:
// the conv-epilogue route (fold_partials_kernel, then bn_finalize_kernel) and the one-launch route (bn_fold_finalize_kernel)
// give the same bits because they run this code.  spconv.hip launches fold_partials_kernel through the prototype below.
#pragma once
#include "common.h"

namespace toda {

constexpr int DN_BLOCK = 256;

// sum of src[0 .. blocks) by one workgroup of DN_BLOCK threads, in a fixed order: thread-strided partial sums, then an LDS
// halving tree over part[DN_BLOCK].  Every thread gets the result; a barrier must stand before part is written again.
__device__ __forceinline__ double fold_column(const double* __restrict__ src, int blocks, double* part) {
    double acc = 0.0;
    for (int g = threadIdx.x; g < blocks; g += DN_BLOCK) acc += src[g];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = DN_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    return part[0];
}

// (mean, var) of channel ch -> (mean, invstd, scale, shift)
__device__ __forceinline__ void bn_write_channel(int ch, float mean, float var, float eps, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float* __restrict__ mean_out,
                                                 float* __restrict__ invstd_out, float* __restrict__ scale_out,
                                                 float* __restrict__ shift_out) {
    const float invstd = 1.0f / sqrtf(var + eps);
    const float g = gamma ? gamma[ch] : 1.0f, b = beta ? beta[ch] : 0.0f;
    mean_out[ch] = mean;
    invstd_out[ch] = invstd;
    scale_out[ch] = g * invstd;
    shift_out[ch] = b - mean * g * invstd;
}

// batch sums of channel ch over n rows -> (mean, invstd, scale, shift) + running-stat update, exactly nn.BatchNorm1d's
// training-mode bookkeeping (biased variance for normalisation, unbiased for running_var, running = (1-m)*running + m*batch)
__device__ __forceinline__ void bn_train_channel(int ch, double sum, double sumsq, int n, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float* __restrict__ running_mean,
                                                 float* __restrict__ running_var, float momentum, float eps,
                                                 float* __restrict__ mean_out, float* __restrict__ invstd_out,
                                                 float* __restrict__ scale_out, float* __restrict__ shift_out) {
    const double m = sum / (double)n;
    double v = sumsq / (double)n - m * m;
    if (v < 0.0) v = 0.0;
    const float mean = (float)m, var = (float)v;
    if (running_mean) {
        const double unbiased = n > 1 ? v * (double)n / (double)(n - 1) : v;
        running_mean[ch] = (1.0f - momentum) * running_mean[ch] + momentum * mean;
        running_var[ch] = (1.0f - momentum) * running_var[ch] + momentum * (float)unbiased;
    }
    bn_write_channel(ch, mean, var, eps, gamma, beta, mean_out, invstd_out, scale_out, shift_out);
}

// dense.hip.  sums[col] = sum_g scratch[col][g], scratch [cols][blocks] behind the cols results: grid = cols, block = DN_BLOCK
__global__ void __launch_bounds__(DN_BLOCK) fold_partials_kernel(double* __restrict__ sums, int blocks, int cols);

}  // namespace toda
