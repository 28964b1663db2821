// Elementwise kernels of the flow-VAE stage forward (flowvae_fwd.h).  Memory-bound passes over [B, C, T] buffers of a few hundred KB:
// lanes run along the time axis (coalesced rows), every output element is written exactly once, tails included.
#include "flowvae_fwd.h"

#include "philox.h"

namespace dtts {

namespace {

constexpr int FV_THREADS = 256;

// z = (m + eps exp(logs)) mask, m, logs: the valid part in the row's own [C, len] element order (four Philox normals per counter
// block, as flow_prior_kernel), then the tails of the three outputs
__global__ __launch_bounds__(FV_THREADS) void posterior_sample_kernel(const float* __restrict__ stats, long long s_bs, int s_cs,
                                                                       const int* __restrict__ lens, int T, int C, unsigned long long seed,
                                                                       const int* __restrict__ sample_ids, const float* __restrict__ noise,
                                                                       float* __restrict__ z, float* __restrict__ m_q, float* __restrict__ logs_q) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int len = min(max(lens ? lens[b] : T, 0), T);
    const float* sb = stats + (long long)b * s_bs;
    const long long ob = (long long)b * C * T;
    const int n = C * len, nblk = (n + 3) / 4;
    const int stride = gridDim.x * blockDim.x, first = blockIdx.x * blockDim.x + threadIdx.x;
    for (int blk = first; blk < nblk; blk += stride) {
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (!noise) philox_normal4(seed, (unsigned)sample_ids[b], STAGE_POSTERIOR, 0, (unsigned)blk, nz);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = blk * 4 + i;
            if (e >= n) break;
            const int c = e / len, t = e - c * len;
            const float m = sb[(long long)c * s_cs + t], logs = sb[(long long)(C + c) * s_cs + t];
            const long long o = ob + (long long)c * T + t;
            const float eps = noise ? noise[o] : nz[i];
            m_q[o] = m;
            logs_q[o] = logs;
            z[o] = m + eps * expf(logs);
        }
    }
    const int tail = T - len, ntail = C * tail;
    for (int e = first; e < ntail; e += stride) {
        const int c = e / tail, t = len + (e - c * tail);
        const long long o = ob + (long long)c * T + t;
        m_q[o] = 0.f;
        logs_q[o] = 0.f;
        z[o] = 0.f;
    }
}

// y = flip_channels(cat(x0, m + x1)), zero beyond len: one block row per (channel, sample)
__global__ __launch_bounds__(FV_THREADS) void coupling_forward_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                                       float* __restrict__ y, long long bs, int cs,
                                                                       const int* __restrict__ lens, int T, int Ctot, int flip) {
    const int c = blockIdx.y, b = blockIdx.z;
    const int len = min(max(lens ? lens[b] : T, 0), T);
    const int half = Ctot / 2;
    const float* xr = x + (long long)b * bs + (long long)c * cs;
    const float* mr = (c >= half) ? m + (long long)b * (long long)half * cs + (long long)(c - half) * cs : nullptr;
    const int co = flip ? (Ctot - 1 - c) : c;
    float* yr = y + (long long)b * bs + (long long)co * cs;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < T; t += gridDim.x * blockDim.x)
        yr[t] = t < len ? (mr ? mr[t] + xr[t] : xr[t]) : 0.f;
}

__global__ __launch_bounds__(FV_THREADS) void slice_segments_kernel(const float* __restrict__ x, const int* __restrict__ ids, int C, int T,
                                                                     int seg, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int start = ids[b];
    const int n = C * seg;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int c = e / seg, j = e - c * seg;
        out[(long long)b * n + e] = x[((long long)b * C + c) * T + start + j];
    }
}

__global__ __launch_bounds__(FV_THREADS) void masked_copy_kernel(const float* __restrict__ x, long long x_bs, int x_cs,
                                                                  const int* __restrict__ lens, int T, int C, const float* __restrict__ tail,
                                                                  float* __restrict__ y) {
    const int c = blockIdx.y, b = blockIdx.z;
    const int len = min(max(lens ? lens[b] : T, 0), T);
    const float* xr = x + (long long)b * x_bs + (long long)c * x_cs;
    float* yr = y + ((long long)b * C + c) * T;
    const float tv = tail ? tail[c] : 0.f;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < T; t += gridDim.x * blockDim.x) yr[t] = t < len ? xr[t] : tv;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one partial per (row, KL_SPAN elements): thread i adds its elements i, i + 256, i + 512, i + 768 in that order, then lanes, then waves
__global__ __launch_bounds__(FV_THREADS) void kl_partials_kernel(const float* __restrict__ z_p, const float* __restrict__ logs_q,
                                                                  const float* __restrict__ m_p, const float* __restrict__ logs_p,
                                                                  const int* __restrict__ lens, int T, int n, float* __restrict__ partials) {
#pragma clang fp contract(off)
    static_assert(KL_SPAN == 4 * FV_THREADS, "four elements per thread");
    __shared__ float sm[FV_THREADS / 64];
    const int b = blockIdx.y;
    const int len = min(max(lens[b], 0), T);
    const long long ob = (long long)b * n;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = blockIdx.x * KL_SPAN + i * FV_THREADS + threadIdx.x;
        if (e < n && e % T < len) {
            const float lp = logs_p[ob + e], d = z_p[ob + e] - m_p[ob + e];
            float kl = (lp - logs_q[ob + e]) - 0.5f;
            kl += (0.5f * (d * d)) * expf(-2.f * lp);
            acc += kl;
        }
    }
    acc = wave_sum(acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = sm[0];
#pragma unroll
        for (int w = 1; w < FV_THREADS / 64; ++w) t += sm[w];
        partials[(long long)b * gridDim.x + blockIdx.x] = t;
    }
}

// out = (sum of the partials in index order, fp64) / frames
__global__ __launch_bounds__(FV_THREADS) void kl_finish_kernel(const float* __restrict__ partials, int npart, double frames,
                                                                float* __restrict__ out) {
    __shared__ double sm[FV_THREADS / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < npart; i += FV_THREADS) acc += (double)partials[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sm[0];
#pragma unroll
        for (int w = 1; w < FV_THREADS / 64; ++w) t += sm[w];
        out[0] = (float)(t / frames);
    }
}

int row_blocks(int T) { return cdiv(T, FV_THREADS) > 8 ? 8 : cdiv(T, FV_THREADS); }

}  // namespace

void launch_posterior_sample(const float* stats, long long s_bs, int s_cs, const int* lens, int T, int B, int C, unsigned long long seed,
                             const int* sample_ids, const float* noise, float* z, float* m_q, float* logs_q, hipStream_t s) {
    DTTS_REQUIRE(stats && z && m_q && logs_q && (noise || sample_ids), "posterior_sample: null argument");
    DTTS_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && T >= 1 && (long long)C * T < (1ll << 30), "posterior_sample: sizes");
    const int nblk = (C * T + 3) / 4;
    hipLaunchKernelGGL(posterior_sample_kernel, dim3(cdiv(nblk, FV_THREADS) > 64 ? 64 : cdiv(nblk, FV_THREADS), B), dim3(FV_THREADS), 0, s,
                       stats, s_bs, s_cs, lens, T, C, seed, sample_ids, noise, z, m_q, logs_q);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_coupling_forward(const float* x, const float* m, float* y, long long bs, int cs, const int* lens, int T, int B, int Ctot,
                             int flip, hipStream_t s) {
    DTTS_REQUIRE(x && m && y && x != y, "coupling_forward: null or aliased argument");
    DTTS_REQUIRE(B >= 1 && B <= 65535 && Ctot >= 2 && Ctot % 2 == 0 && Ctot <= 65535 && T >= 1 && T <= cs, "coupling_forward: sizes");
    hipLaunchKernelGGL(coupling_forward_kernel, dim3(row_blocks(T), Ctot, B), dim3(FV_THREADS), 0, s, x, m, y, bs, cs, lens, T, Ctot, flip);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_slice_segments(const float* x, const int* ids, int B, int C, int T, int seg, float* out, hipStream_t s) {
    DTTS_REQUIRE(x && ids && out, "slice_segments: null argument");
    DTTS_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && seg >= 1 && seg <= T && (long long)C * T < (1ll << 30), "slice_segments: sizes");
    const int n = C * seg;
    hipLaunchKernelGGL(slice_segments_kernel, dim3(cdiv(n, FV_THREADS) > 64 ? 64 : cdiv(n, FV_THREADS), B), dim3(FV_THREADS), 0, s, x, ids, C,
                       T, seg, out);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_masked_copy(const float* x, long long x_bs, int x_cs, const int* lens, int T, int B, int C, const float* tail, float* y,
                        hipStream_t s) {
    DTTS_REQUIRE(x && y, "masked_copy: null argument");
    DTTS_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && C <= 65535 && T >= 1 && T <= x_cs, "masked_copy: sizes");
    hipLaunchKernelGGL(masked_copy_kernel, dim3(row_blocks(T), C, B), dim3(FV_THREADS), 0, s, x, x_bs, x_cs, lens, T, C, tail, y);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_kl_loss(const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, const int* lens, int B, int C, int T,
                    double frames, float* partials, float* out, hipStream_t s) {
    DTTS_REQUIRE(z_p && logs_q && m_p && logs_p && lens && partials && out, "kl_loss: null argument");
    DTTS_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && T >= 1 && (long long)C * T < (1ll << 30) && frames >= 1.0, "kl_loss: sizes");
    const int n = C * T, nblk = kl_partials(n);
    DTTS_REQUIRE((long long)B * nblk < (1ll << 30), "kl_loss: sizes");
    hipLaunchKernelGGL(kl_partials_kernel, dim3(nblk, B), dim3(FV_THREADS), 0, s, z_p, logs_q, m_p, logs_p, lens, T, n, partials);
    DTTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(kl_finish_kernel, dim3(1), dim3(FV_THREADS), 0, s, partials, B * nblk, frames, out);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
