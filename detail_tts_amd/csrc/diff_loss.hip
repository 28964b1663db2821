// Evaluation losses of the diffusion and VQ stages (diff_loss.h).  Memory-bound elementwise passes with a two-level, fixed-order sum:
// a block of 256 threads covers DIFF_LOSS_SPAN contiguous elements of one row (16-byte loads, 4 elements per thread), sums them lane
// by lane (xor shuffles), wave by wave, and writes one partial per sum; a finishing block per row adds the row's partials in index order.
#include "diff_loss.h"

#include "common.h"
#include "diff_loss_dev.h"
#include "philox.h"

namespace dtts {

namespace {

using namespace loss_dev;

__global__ __launch_bounds__(LOSS_THREADS) void diff_q_sample_kernel(const float* __restrict__ mel, int normalize,
                                                                      const DiffLossCoefs* __restrict__ coefs,
                                                                      const float* __restrict__ noise, unsigned long long seed,
                                                                      const int* __restrict__ sample_ids, int n, float* __restrict__ x_start_out,
                                                                      float* __restrict__ x_t_out, float* __restrict__ noise_out) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int e = (blockIdx.x * LOSS_THREADS + threadIdx.x) * 4;
    if (e >= n) return;                                   // n % 4 == 0: a thread's four elements are all inside or all outside
    const long long o = (long long)b * n + e;
    const DiffLossCoefs k = coefs[b];
    const float4 m4 = *reinterpret_cast<const float4*>(mel + o);
    float m[4] = {m4.x, m4.y, m4.z, m4.w}, z[4], xs[4], xt[4];
    if (noise) {
        const float4 n4 = *reinterpret_cast<const float4*>(noise + o);
        z[0] = n4.x; z[1] = n4.y; z[2] = n4.z; z[3] = n4.w;
    } else {
        philox_normal4(seed, (unsigned)sample_ids[b], STAGE_DIFF_QSAMPLE, 0, (unsigned)(e >> 2), z);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // normalize_torch_mel (vqvae/model_24k.py:500-505): 2 ((mel - MEL_MIN) / (TORCH_MEL_MAX - MEL_MIN)) - 1, each operation rounded
        xs[i] = normalize ? 2.f * ((m[i] - (-11.512925465f)) / (float)(2.7 - (-11.512925465))) - 1.f : m[i];
        xt[i] = k.sqrt_ac * xs[i] + k.sqrt_1m_ac * z[i];
    }
    if (x_start_out) *reinterpret_cast<float4*>(x_start_out + o) = make_float4(xs[0], xs[1], xs[2], xs[3]);
    *reinterpret_cast<float4*>(x_t_out + o) = make_float4(xt[0], xt[1], xt[2], xt[3]);
    if (noise_out && !noise) *reinterpret_cast<float4*>(noise_out + o) = make_float4(z[0], z[1], z[2], z[3]);
}

__global__ __launch_bounds__(LOSS_THREADS) void diff_loss_partials_kernel(const float* __restrict__ model_out, const float* __restrict__ x_start,
                                                                           const float* __restrict__ x_t, const float* __restrict__ noise,
                                                                           const DiffLossCoefs* __restrict__ coefs, int n,
                                                                           float* __restrict__ partials, float* __restrict__ pred_xstart) {
    __shared__ float sm[2 * (LOSS_THREADS / 64)];
    const int b = blockIdx.y;
    const int e = (blockIdx.x * LOSS_THREADS + threadIdx.x) * 4;
    const DiffLossCoefs k = coefs[b];
    float acc[2] = {0.f, 0.f};                            // (sum of (noise - eps)^2, sum of the vb elements) of this thread's four
    if (e < n) {
        const long long o = (long long)b * n + e, om = (long long)b * 2 * n + e;
        const float4 e4 = *reinterpret_cast<const float4*>(model_out + om);
        const float4 v4 = *reinterpret_cast<const float4*>(model_out + om + n);
        const float4 s4 = *reinterpret_cast<const float4*>(x_start + o);
        const float4 t4 = *reinterpret_cast<const float4*>(x_t + o);
        const float4 z4 = *reinterpret_cast<const float4*>(noise + o);
        const float ep[4] = {e4.x, e4.y, e4.z, e4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w}, xs[4] = {s4.x, s4.y, s4.z, s4.w},
                    xt[4] = {t4.x, t4.y, t4.z, t4.w}, zz[4] = {z4.x, z4.y, z4.z, z4.w};
        float p0[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = zz[i] - ep[i];
            acc[0] += d * d;
            acc[1] += vb_element(k, ep[i], vv[i], xs[i], xt[i], p0[i]);
        }
        if (pred_xstart) *reinterpret_cast<float4*>(pred_xstart + o) = make_float4(p0[0], p0[1], p0[2], p0[3]);
    }
    block_sum<2>(acc, sm);
    if (threadIdx.x == 0) {
        float* p = partials + ((long long)b * gridDim.x + blockIdx.x) * 2;
        p[0] = acc[0];
        p[1] = acc[1];
    }
}

// terms[b] = (mse, vb, mse + vb): mean_flat of both sums, the vb term in bits (:917, 923)
__global__ __launch_bounds__(LOSS_THREADS) void diff_loss_finish_kernel(const float* __restrict__ partials, int nblk, int n, float* __restrict__ terms) {
    __shared__ double sm[LOSS_THREADS / 64];
    const int b = blockIdx.x;
    const float* p = partials + (long long)b * nblk * 2;
    const double mse = finish_sum(p, nblk, 2, sm);
    const double vb = finish_sum(p + 1, nblk, 2, sm);
    if (threadIdx.x == 0) {
        const float m = (float)(mse / (double)n), v = (float)(vb / (double)n / 0.6931471805599453);
        terms[b * 3 + 0] = m;
        terms[b * 3 + 1] = v;
        terms[b * 3 + 2] = m + v;
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void l1_partials_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                                                    float* __restrict__ partials) {
    __shared__ float sm[LOSS_THREADS / 64];
    const long long e = ((long long)blockIdx.x * LOSS_THREADS + threadIdx.x) * 4;
    float acc[1] = {0.f};
    if (e < n) {
        const float4 a4 = *reinterpret_cast<const float4*>(a + e);
        const float4 b4 = *reinterpret_cast<const float4*>(b + e);
        acc[0] = ((fabsf(a4.x - b4.x) + fabsf(a4.y - b4.y)) + fabsf(a4.z - b4.z)) + fabsf(a4.w - b4.w);
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(LOSS_THREADS) void l1_finish_kernel(const float* __restrict__ partials, int nblk, long long n, float* __restrict__ out) {
    __shared__ double sm[LOSS_THREADS / 64];
    const double t = finish_sum(partials, nblk, 1, sm);
    if (threadIdx.x == 0) out[0] = (float)(t / (double)n);
}

}  // namespace

void launch_diff_q_sample(const float* mel, int normalize, const DiffLossCoefs* coefs, const float* noise, unsigned long long seed,
                          const int* sample_ids, int B, int n, float* x_start_out, float* x_t_out, float* noise_out, hipStream_t s) {
    DTTS_REQUIRE(B >= 1 && n >= 4 && n % 4 == 0, "q_sample: rows of a multiple of 4 elements");
    DTTS_REQUIRE(mel && coefs && x_t_out && (noise || sample_ids), "q_sample: null argument");
    hipLaunchKernelGGL(diff_q_sample_kernel, dim3(diff_loss_blocks(n), B), dim3(LOSS_THREADS), 0, s, mel, normalize, coefs, noise, seed,
                       sample_ids, n, x_start_out, x_t_out, noise_out);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_diff_loss_terms(const float* model_out, const float* x_start, const float* x_t, const float* noise, const DiffLossCoefs* coefs,
                            int B, int n, float* partials, float* terms, float* pred_xstart, hipStream_t s) {
    DTTS_REQUIRE(B >= 1 && n >= 4 && n % 4 == 0, "diff_loss_terms: rows of a multiple of 4 elements");
    DTTS_REQUIRE(model_out && x_start && x_t && noise && coefs && partials && terms, "diff_loss_terms: null argument");
    const int nblk = diff_loss_blocks(n);
    hipLaunchKernelGGL(diff_loss_partials_kernel, dim3(nblk, B), dim3(LOSS_THREADS), 0, s, model_out, x_start, x_t, noise, coefs, n, partials,
                       pred_xstart);
    DTTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(diff_loss_finish_kernel, dim3(B), dim3(LOSS_THREADS), 0, s, partials, nblk, n, terms);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_l1_mean(const float* a, const float* b, long long n, float* partials, float* out, hipStream_t s) {
    DTTS_REQUIRE(n >= 4 && n % 4 == 0 && n / DIFF_LOSS_SPAN < (1ll << 30), "l1_mean: a multiple of 4 elements");
    DTTS_REQUIRE(a && b && partials && out, "l1_mean: null argument");
    const int nblk = diff_loss_blocks(n);
    hipLaunchKernelGGL(l1_partials_kernel, dim3(nblk), dim3(LOSS_THREADS), 0, s, a, b, n, partials);
    DTTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(l1_finish_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, partials, nblk, n, out);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
