// Kernels of the discriminator forward and its losses (disc.h).  Lanes run along the time axis everywhere (coalesced rows); every
// output element is written exactly once and nothing is written outside [0, Nout) of a row.
#include "disc.h"

#include "../../include/detail_hip.h"

namespace dtts {

namespace {

constexpr int DT = 256;

__device__ __forceinline__ float lrelu(float v, float slope) { return v >= 0.f ? v : v * slope; }

__global__ __launch_bounds__(DT) void period_split_kernel(const float* __restrict__ y, const float* __restrict__ y_hat, int B, int t, int p,
                                                          int H, float* __restrict__ out) {
    const int h = blockIdx.x * DT + threadIdx.x, r = blockIdx.y;
    if (h >= H) return;
    const int n = r / p, w = r - n * p;
    int i = h * p + w;
    if (i >= t) i = 2 * (t - 1) - i;                    // reflect at the right end; i < t + p - 1 and t > p - 1, so 0 <= 2 (t - 1) - i < t
    const float* src = n < B ? y + (long long)n * t : y_hat + (long long)(n - B) * t;
    out[(long long)r * H + h] = src[i];
}

template <int K>
__global__ __launch_bounds__(DT) void disc_first_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                        int Tin, int Cout, int stride, int pad, float slope, float* __restrict__ y, int Nout) {
    const int n = blockIdx.x * DT + threadIdx.x, r = blockIdx.y;
    if (n >= Nout) return;
    const float* xr = x + (long long)r * Tin;
    float xv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int ti = n * stride + k - pad;
        xv[k] = (ti >= 0 && ti < Tin) ? xr[ti] : 0.f;
    }
    float* yr = y + (long long)r * Cout * Nout + n;
    for (int co = 0; co < Cout; ++co) {                 // w, b: wave-uniform addresses
        float acc = b[co];
#pragma unroll
        for (int k = 0; k < K; ++k) acc = fmaf(w[co * K + k], xv[k], acc);
        yr[(long long)co * Nout] = lrelu(acc, slope);
    }
}

// CO_PER output channels of one column per thread: wave q of the 4 owns channels [q CO_PER, (q + 1) CO_PER) of the group
template <int CO_PER>
__global__ __launch_bounds__(DT) void conv1d_grouped_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                            int Cin, int Tin, int Cout, int groups, int K, int stride, int pad, float slope,
                                                            float* __restrict__ y, int Nout) {
    extern __shared__ float sm[];
    const int cin_g = Cin / groups, cout_g = 4 * CO_PER;
    const int g = blockIdx.y, r = blockIdx.z, n0 = blockIdx.x * GC_TN;
    const int win = (GC_TN - 1) * stride + K;
    float* xs = sm;                                     // [cin_g][win]
    float* ws = sm + cin_g * win;                       // [cout_g][cin_g][K]
    const int t0 = n0 * stride - pad;
    const float* xg = x + ((long long)r * Cin + (long long)g * cin_g) * Tin;
    for (int i = threadIdx.x; i < cin_g * win; i += DT) {
        const int ci = i / win, ti = t0 + (i - ci * win);
        xs[i] = (ti >= 0 && ti < Tin) ? xg[(long long)ci * Tin + ti] : 0.f;
    }
    const int nw = cout_g * cin_g * K;
    const float* wg = w + (long long)g * nw;
    for (int i = threadIdx.x; i < nw; i += DT) ws[i] = wg[i];
    __syncthreads();
    const int col = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int co0 = g * cout_g + q * CO_PER;
    float acc[CO_PER];
#pragma unroll
    for (int j = 0; j < CO_PER; ++j) acc[j] = b ? b[co0 + j] : 0.f;
    for (int ci = 0; ci < cin_g; ++ci) {
        const float* xp = xs + ci * win + col * stride;
        const float* wp = ws + ((q * CO_PER) * cin_g + ci) * K;      // wave-uniform: LDS broadcast
        for (int k = 0; k < K; ++k) {
            const float xv = xp[k];
#pragma unroll
            for (int j = 0; j < CO_PER; ++j) acc[j] = fmaf(wp[j * cin_g * K + k], xv, acc[j]);
        }
    }
    const int n = n0 + col;
    if (n < Nout) {
#pragma unroll
        for (int j = 0; j < CO_PER; ++j) y[((long long)r * Cout + co0 + j) * Nout + n] = lrelu(acc[j], slope);
    }
}

__global__ __launch_bounds__(DT) void deinterleave3_kernel(const float* __restrict__ x, int C, int H, int M, float* __restrict__ out) {
    const int m = blockIdx.x * DT + threadIdx.x, cj = blockIdx.y, r = blockIdx.z;
    if (m >= M) return;
    const int c = cj / 3, j = cj - 3 * c, h = 3 * m + j;
    out[((long long)r * 3 * C + cj) * M + m] = h < H ? x[((long long)r * C + c) * H + h] : 0.f;
}

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(DT) void loss_partials_kernel(const LossItems L, float* __restrict__ partials) {
#pragma clang fp contract(off)
    static_assert(LOSS_SPAN == 4 * DT, "four elements per thread");
    __shared__ float sm[DT / 64];
    const int blk = blockIdx.x;
    int k = 0;
    while (k + 1 < L.n && L.it[k + 1].blk0 <= blk) ++k;
    const float* a = L.it[k].a;
    const float* b = L.it[k].b;
    const long long n = L.it[k].n, base = (long long)(blk - L.it[k].blk0) * LOSS_SPAN;
    const int mode = L.it[k].mode;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long e = base + i * DT + threadIdx.x;
        if (e < n) {
            const float v = a[e];
            float d;
            if (mode == LOSS_ABS_DIFF) d = fabsf(v - b[e]);
            else if (mode == LOSS_ONE_MINUS_SQ) d = (1.f - v) * (1.f - v);
            else d = v * v;
            acc += d;
        }
    }
    acc = wave_sum_f(acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = sm[0];
#pragma unroll
        for (int w = 1; w < DT / 64; ++w) t += sm[w];
        partials[blk] = t;
    }
}

__global__ __launch_bounds__(DT) void loss_finish_kernel(const LossItems L, const float* __restrict__ partials, float* __restrict__ means) {
    __shared__ double sm[DT / 64];
    const int k = blockIdx.x;
    const int b0 = L.it[k].blk0, nb = (int)((L.it[k].n + LOSS_SPAN - 1) / LOSS_SPAN);
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += DT) acc += (double)partials[b0 + i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sm[0];
#pragma unroll
        for (int w = 1; w < DT / 64; ++w) t += sm[w];
        means[k] = (float)(t / (double)L.it[k].n);
    }
}

__global__ void disc_combine_kernel(const float* __restrict__ means, int n_maps, int n_scores, int has_real, float* __restrict__ out) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float fm = 0.f;
    for (int k = 0; k < n_maps; ++k) {
        fm += means[k];
        out[DTTS_DISC_MAP_MEANS + k] = means[k];
    }
    out[DTTS_DISC_LOSS_FM] = fm * 2.f;
    const float* mr = means + n_maps;
    const float* mg = mr + (has_real ? n_scores : 0);
    const float* mgen = mg + n_scores;
    float ld = 0.f, lg = 0.f;
    for (int k = 0; k < n_scores; ++k) {
        if (has_real) {
            ld += mr[k] + mg[k];
            out[DTTS_DISC_LOSSES_R + k] = mr[k];
        }
        out[DTTS_DISC_LOSSES_G + k] = mg[k];
        lg += mgen[k];
        out[DTTS_DISC_LOSSES_GEN + k] = mgen[k];
    }
    out[DTTS_DISC_LOSS_DISC] = ld;
    out[DTTS_DISC_LOSS_GEN] = lg;
}

__global__ void stage_combine_kernel(const float* __restrict__ mel_l1, const float* __restrict__ kl, float* __restrict__ out) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float mel = mel_l1[0] * 45.f, k = kl[0];
    out[DTTS_DISC_LOSS_MEL] = mel;
    out[DTTS_DISC_LOSS_KL] = k;
    out[DTTS_DISC_LOSS_GEN_ALL] = ((out[DTTS_DISC_LOSS_GEN] + out[DTTS_DISC_LOSS_FM]) + mel) + k;
}

}  // namespace

void launch_period_split(const float* y, const float* y_hat, int B, int N, int t, int p, float* out, hipStream_t s) {
    DTTS_REQUIRE(y && out && (N == B || (N == 2 * B && y_hat)), "period_split: null argument");
    DTTS_REQUIRE(B >= 1 && p >= 1 && t >= p && t < (1 << 28) && (long long)N * p <= 65535, "period_split: sizes");
    const int H = cdiv(t, p);
    hipLaunchKernelGGL(period_split_kernel, dim3(cdiv(H, DT), N * p), dim3(DT), 0, s, y, y_hat, B, t, p, H, out);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_disc_first(const float* x, const float* w, const float* b, int R, int Tin, int Cout, int K, int stride, int pad, float slope,
                       float* y, int Nout, hipStream_t s) {
    DTTS_REQUIRE(x && w && b && y, "disc_first: null argument");
    DTTS_REQUIRE(R >= 1 && R <= 65535 && Tin >= 1 && Cout >= 1 && stride >= 1 && pad >= 0, "disc_first: sizes");
    DTTS_REQUIRE(Nout >= 1 && Nout == (Tin + 2 * pad - K) / stride + 1, "disc_first: output length");
    const dim3 grid(cdiv(Nout, DT), R);
    if (K == 5) hipLaunchKernelGGL(disc_first_kernel<5>, grid, dim3(DT), 0, s, x, w, b, Tin, Cout, stride, pad, slope, y, Nout);
    else if (K == 15) hipLaunchKernelGGL(disc_first_kernel<15>, grid, dim3(DT), 0, s, x, w, b, Tin, Cout, stride, pad, slope, y, Nout);
    else DTTS_REQUIRE(false, "disc_first: kernel size 5 or 15");
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_conv1d_grouped(const float* x, const float* w, const float* b, int R, int Cin, int Tin, int Cout, int groups, int K, int stride,
                           int pad, float slope, float* y, int Nout, hipStream_t s) {
    DTTS_REQUIRE(x && w && y, "conv1d_grouped: null argument");
    DTTS_REQUIRE(R >= 1 && R <= 65535 && groups >= 1 && groups <= 65535 && Cin >= 1 && Cout >= 1 && Tin >= 1 && K >= 1 && stride >= 1 && pad >= 0,
                 "conv1d_grouped: sizes");
    DTTS_REQUIRE(Cin % groups == 0 && Cout % groups == 0, "conv1d_grouped: groups must divide both channel counts");
    const int cin_g = Cin / groups, cout_g = Cout / groups;
    DTTS_REQUIRE(cout_g == 4 || cout_g == 16, "conv1d_grouped: 4 or 16 output channels per group");
    DTTS_REQUIRE(Tin + 2 * pad >= K && Nout == (Tin + 2 * pad - K) / stride + 1, "conv1d_grouped: output length");
    const long long lds = 4ll * ((long long)cin_g * ((GC_TN - 1) * stride + K) + (long long)cout_g * cin_g * K);
    DTTS_REQUIRE(lds <= 48 * 1024, "conv1d_grouped: a group's window and weights must fit 48 KiB of LDS");
    const dim3 grid(cdiv(Nout, GC_TN), groups, R);
    if (cout_g == 16)
        hipLaunchKernelGGL(conv1d_grouped_kernel<4>, grid, dim3(DT), (size_t)lds, s, x, w, b, Cin, Tin, Cout, groups, K, stride, pad, slope, y, Nout);
    else
        hipLaunchKernelGGL(conv1d_grouped_kernel<1>, grid, dim3(DT), (size_t)lds, s, x, w, b, Cin, Tin, Cout, groups, K, stride, pad, slope, y, Nout);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_deinterleave3(const float* x, int R, int C, int H, float* out, hipStream_t s) {
    DTTS_REQUIRE(x && out && x != out, "deinterleave3: null or aliased argument");
    DTTS_REQUIRE(R >= 1 && R <= 65535 && C >= 1 && 3 * C <= 65535 && H >= 1, "deinterleave3: sizes");
    const int M = cdiv(H, 3);
    hipLaunchKernelGGL(deinterleave3_kernel, dim3(cdiv(M, DT), 3 * C, R), dim3(DT), 0, s, x, C, H, M, out);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_loss_means(const LossItems& items, float* partials, float* means, hipStream_t s) {
    DTTS_REQUIRE(partials && means && items.n >= 1 && items.n <= LOSS_MAX_ITEMS && items.blocks >= items.n, "loss_means: arguments");
    for (int k = 0; k < items.n; ++k)
        DTTS_REQUIRE(items.it[k].a && items.it[k].n >= 1 && (items.it[k].mode != LOSS_ABS_DIFF || items.it[k].b), "loss_means: an empty or null item");
    hipLaunchKernelGGL(loss_partials_kernel, dim3(items.blocks), dim3(DT), 0, s, items, partials);
    DTTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loss_finish_kernel, dim3(items.n), dim3(DT), 0, s, items, partials, means);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_disc_combine(const float* means, int n_maps, int n_scores, int has_real, float* out, hipStream_t s) {
    DTTS_REQUIRE(means && out && n_maps >= 0 && n_maps <= DISC_MAPS && n_scores >= 0 && n_scores <= DISC_COUNT, "disc_combine: arguments");
    hipLaunchKernelGGL(disc_combine_kernel, dim3(1), dim3(64), 0, s, means, n_maps, n_scores, has_real, out);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_stage_combine(const float* mel_l1, const float* kl, float* out, hipStream_t s) {
    DTTS_REQUIRE(mel_l1 && kl && out, "stage_combine: null argument");
    hipLaunchKernelGGL(stage_combine_kernel, dim3(1), dim3(64), 0, s, mel_l1, kl, out);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
