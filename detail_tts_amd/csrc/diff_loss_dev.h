// Device pieces the evaluation-loss kernels share (diff_loss.hip, diff_bpd.hip): the fixed-order block sums and one element of the
// variational-bound term.  Included by kernels only.
#pragma once
#include <hip/hip_runtime.h>

#include "diff_loss.h"

namespace dtts {
namespace loss_dev {

constexpr int LOSS_THREADS = 256;
static_assert(LOSS_THREADS * 4 == DIFF_LOSS_SPAN, "one float4 per thread");

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sums of NV values over the block; the totals are valid in thread 0.  sm: NV * (LOSS_THREADS / 64) floats
template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float* sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = wave_sum(v[i]);
        if (lane == 0) sm[i * (LOSS_THREADS / 64) + wave] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float t = sm[i * (LOSS_THREADS / 64)];
#pragma unroll
            for (int w = 1; w < LOSS_THREADS / 64; ++w) t += sm[i * (LOSS_THREADS / 64) + w];
            v[i] = t;
        }
    }
}

// sum of part[0 .. n) * stride in index order per thread, then over the block (fp64: a few hundred terms, free of the partials' own rounding)
__device__ __forceinline__ double finish_sum(const float* part, int n, int stride, double* sm) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += LOSS_THREADS) acc += (double)part[(long long)i * stride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    __syncthreads();                                      // (sm may still be read from a previous call)
    if (lane == 0) sm[wave] = acc;
    __syncthreads();
    double t = sm[0];
#pragma unroll
    for (int w = 1; w < LOSS_THREADS / 64; ++w) t += sm[w];
    return t;
}

// approx_standard_normal_cdf (vqvae/utils/diffusion.py:38-43)
__device__ __forceinline__ float approx_cdf(float x) {
#pragma clang fp contract(off)
    return 0.5f * (1.f + tanhf(0.7978845608028654f * (x + 0.044715f * (x * x * x))));
}

// one element of the variational-bound term in nats (_vb_terms_bpd with the frozen model output, :903-928, 978-987)
__device__ __forceinline__ float vb_element(const DiffLossCoefs& k, float eps, float v, float x0, float xt, float& pred_x0) {
#pragma clang fp contract(off)
    pred_x0 = k.sqrt_recip_ac * xt - k.sqrt_recipm1_ac * eps;                      // _predict_xstart_from_eps
    const float x0c = fminf(fmaxf(pred_x0, -1.f), 1.f);                            // clip_denoised = True
    const float mean = k.coef1 * x0c + k.coef2 * xt;                                // q_posterior_mean_variance of the predicted start
    const float true_mean = k.coef1 * x0 + k.coef2 * xt;                            // ... and of the true one
    const float frac = (v + 1.f) / 2.f;                                             // learned range (:329-335)
    const float logvar = frac * k.max_log + (1.f - frac) * k.min_log;
    if (!k.t0) {                                                                    // normal_kl (:17-35)
        const float d = true_mean - mean;
        return 0.5f * (-1.f + logvar - k.min_log + expf(k.min_log - logvar) + (d * d) * expf(-logvar));
    }
    // -discretized_gaussian_log_likelihood(x_start, means = mean, log_scales = 0.5 logvar) (:46-73)
    const float centered = x0 - mean;
    const float inv_stdv = expf(-(0.5f * logvar));
    const float cdf_plus = approx_cdf(inv_stdv * (centered + (float)(1.0 / 255.0)));
    const float cdf_min = approx_cdf(inv_stdv * (centered - (float)(1.0 / 255.0)));
    float lp;
    if (x0 < -0.999f) lp = logf(fmaxf(cdf_plus, 1e-12f));
    else if (x0 > 0.999f) lp = logf(fmaxf(1.f - cdf_min, 1e-12f));
    else lp = logf(fmaxf(cdf_plus - cdf_min, 1e-12f));
    return -lp;
}

}  // namespace loss_dev
}  // namespace dtts
