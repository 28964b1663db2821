// The variational bound in bits per dimension (diff_bpd.h).  The same memory-bound passes and two-level, fixed-order sums as
// diff_loss.hip: a block of 256 threads covers DIFF_LOSS_SPAN contiguous elements of one virtual row, one partial per sum and block,
// and a finishing block per row adds the row's partials in index order.
#include "diff_bpd.h"

#include "common.h"
#include "diff_loss_dev.h"
#include "philox.h"

namespace dtts {

namespace {

using namespace loss_dev;

__global__ __launch_bounds__(LOSS_THREADS) void bpd_q_sample_kernel(const float* __restrict__ x_start, const DiffBpdRow* __restrict__ rows,
                                                                     const float* __restrict__ noise, unsigned long long seed, int B, int n,
                                                                     float* __restrict__ x_t_out, float* __restrict__ noise_out) {
#pragma clang fp contract(off)
    const int r = blockIdx.y;
    const int e = (blockIdx.x * LOSS_THREADS + threadIdx.x) * 4;
    if (e >= n) return;                                   // n % 4 == 0: a thread's four elements are all inside or all outside
    const DiffBpdRow row = rows[r];
    const long long o = (long long)r * n + e;
    const float4 s4 = *reinterpret_cast<const float4*>(x_start + (long long)row.b * n + e);
    const float xs[4] = {s4.x, s4.y, s4.z, s4.w};
    float z[4], xt[4];
    if (noise) {
        const float4 n4 = *reinterpret_cast<const float4*>(noise + ((long long)row.t * B + row.b) * n + e);
        z[0] = n4.x; z[1] = n4.y; z[2] = n4.z; z[3] = n4.w;
    } else {
        philox_normal4(seed, (unsigned)row.sid, STAGE_DIFF_BPD, (unsigned)row.t, (unsigned)(e >> 2), z);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) xt[i] = row.k.sqrt_ac * xs[i] + row.k.sqrt_1m_ac * z[i];
    *reinterpret_cast<float4*>(x_t_out + o) = make_float4(xt[0], xt[1], xt[2], xt[3]);
    *reinterpret_cast<float4*>(noise_out + o) = make_float4(z[0], z[1], z[2], z[3]);
}

// dst[r] = src[b(r)] over n4 float4 per row
__global__ __launch_bounds__(LOSS_THREADS) void bpd_gather_rows_kernel(const float4* __restrict__ src, const DiffBpdRow* __restrict__ rows,
                                                                        long long n4, float4* __restrict__ dst) {
    const int r = blockIdx.y;
    const float4* s = src + (long long)rows[r].b * n4;
    float4* d = dst + (long long)r * n4;
    for (long long i = (long long)blockIdx.x * LOSS_THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * LOSS_THREADS) d[i] = s[i];
}

__global__ __launch_bounds__(LOSS_THREADS) void bpd_terms_partials_kernel(const float* __restrict__ model_out, const float* __restrict__ x_start,
                                                                           int x_start_rows, const float* __restrict__ x_t,
                                                                           const float* __restrict__ noise, const DiffBpdRow* __restrict__ rows,
                                                                           int n, float* __restrict__ partials, float* __restrict__ pred_xstart) {
#pragma clang fp contract(off)
    __shared__ float sm[3 * (LOSS_THREADS / 64)];
    const int r = blockIdx.y;
    const int e = (blockIdx.x * LOSS_THREADS + threadIdx.x) * 4;
    const DiffBpdRow row = rows[r];
    float acc[3] = {0.f, 0.f, 0.f};                       // sums of this thread's four: vb elements, (x0' - x0)^2, (eps' - noise)^2
    if (e < n) {
        const long long o = (long long)r * n + e, om = (long long)r * 2 * n + e;
        const float4 e4 = *reinterpret_cast<const float4*>(model_out + om);
        const float4 v4 = *reinterpret_cast<const float4*>(model_out + om + n);
        const float4 s4 = *reinterpret_cast<const float4*>(x_start + (long long)(x_start_rows ? r : row.b) * n + e);
        const float4 t4 = *reinterpret_cast<const float4*>(x_t + o);
        const float4 z4 = *reinterpret_cast<const float4*>(noise + o);
        const float ep[4] = {e4.x, e4.y, e4.z, e4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w}, xs[4] = {s4.x, s4.y, s4.z, s4.w},
                    xt[4] = {t4.x, t4.y, t4.z, t4.w}, zz[4] = {z4.x, z4.y, z4.z, z4.w};
        float p0[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float raw;
            acc[0] += vb_element(row.k, ep[i], vv[i], xs[i], xt[i], raw);
            p0[i] = fminf(fmaxf(raw, -1.f), 1.f);                                         // p_mean_variance's pred_xstart, clip_denoised (:357-375)
            const float dx = p0[i] - xs[i];
            acc[1] += dx * dx;
            const float eps1 = (row.k.sqrt_recip_ac * xt[i] - p0[i]) / row.k.sqrt_recipm1_ac;   // _predict_eps_from_xstart (:402-405)
            const float de = eps1 - zz[i];
            acc[2] += de * de;
        }
        if (pred_xstart) *reinterpret_cast<float4*>(pred_xstart + o) = make_float4(p0[0], p0[1], p0[2], p0[3]);
    }
    block_sum<3>(acc, sm);
    if (threadIdx.x == 0) {
        float* p = partials + ((long long)r * gridDim.x + blockIdx.x) * 3;
        p[0] = acc[0];
        p[1] = acc[1];
        p[2] = acc[2];
    }
}

// mean_flat of the three sums of row r, the vb term in bits (:917, 923), to its place in the three outputs
__global__ __launch_bounds__(LOSS_THREADS) void bpd_terms_finish_kernel(const float* __restrict__ partials, const DiffBpdRow* __restrict__ rows,
                                                                         int nblk, int n, float* __restrict__ vb, float* __restrict__ xstart_mse,
                                                                         float* __restrict__ mse, int stride) {
    __shared__ double sm[LOSS_THREADS / 64];
    const int r = blockIdx.x;
    const float* p = partials + (long long)r * nblk * 3;
    const double v = finish_sum(p, nblk, 3, sm);
    const double xm = finish_sum(p + 1, nblk, 3, sm);
    const double m = finish_sum(p + 2, nblk, 3, sm);
    if (threadIdx.x == 0) {
        const long long d = (long long)rows[r].dst * stride;
        vb[d] = (float)(v / (double)n / 0.6931471805599453);
        xstart_mse[d] = (float)(xm / (double)n);
        mse[d] = (float)(m / (double)n);
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void bpd_prior_partials_kernel(const float* __restrict__ x_start, float sqrt_ac, float log_1m_ac, int n,
                                                                           float* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ float sm[LOSS_THREADS / 64];
    const int b = blockIdx.y;
    const int e = (blockIdx.x * LOSS_THREADS + threadIdx.x) * 4;
    float acc[1] = {0.f};
    if (e < n) {
        const float4 s4 = *reinterpret_cast<const float4*>(x_start + (long long)b * n + e);
        const float xs[4] = {s4.x, s4.y, s4.z, s4.w};
        const float ex = expf(log_1m_ac - 0.f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // normal_kl(mean1 = sqrt_ac x, logvar1 = log_1m_ac, mean2 = 0, logvar2 = 0) (:17-35), the reference's order of operations
            const float m = sqrt_ac * xs[i] - 0.f;
            acc[0] += 0.5f * (-1.f + 0.f - log_1m_ac + ex + (m * m) * 1.f);
        }
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) partials[(long long)b * gridDim.x + blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(LOSS_THREADS) void bpd_prior_finish_kernel(const float* __restrict__ partials, int nblk, int n, float* __restrict__ prior) {
    __shared__ double sm[LOSS_THREADS / 64];
    const int b = blockIdx.x;
    const double t = finish_sum(partials + (long long)b * nblk, nblk, 1, sm);
    if (threadIdx.x == 0) prior[b] = (float)(t / (double)n / 0.6931471805599453);
}

__global__ __launch_bounds__(LOSS_THREADS) void bpd_total_kernel(const float* __restrict__ vb, const float* __restrict__ prior, int B, int S,
                                                                  float* __restrict__ total) {
    const int b = blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (b >= B) return;
    double acc = 0.0;                                     // 200 terms in column order: the correctly rounded fp32 sum
    for (int j = 0; j < S; ++j) acc += (double)vb[(long long)b * S + j];
    total[b] = (float)acc + prior[b];
}

}  // namespace

void launch_diff_bpd_q_sample(const float* x_start, const DiffBpdRow* rows, const float* noise, unsigned long long seed, int B, int R,
                              int n, float* x_t_out, float* noise_out, const float* code_emb, float* code_out, long long ncode,
                              hipStream_t s) {
    DTTS_REQUIRE(B >= 1 && R >= 1 && R <= 65535 && n >= 4 && n % 4 == 0, "bpd q_sample: 1 .. 65535 rows of a multiple of 4 elements");
    DTTS_REQUIRE(x_start && rows && x_t_out && noise_out, "bpd q_sample: null argument");
    DTTS_REQUIRE((code_emb == nullptr) == (code_out == nullptr) && (!code_emb || (ncode >= 4 && ncode % 4 == 0)), "bpd q_sample: code rows");
    hipLaunchKernelGGL(bpd_q_sample_kernel, dim3(diff_loss_blocks(n), R), dim3(LOSS_THREADS), 0, s, x_start, rows, noise, seed, B, n, x_t_out,
                       noise_out);
    DTTS_CHECK_HIP(hipGetLastError());
    if (code_emb) {
        const long long n4 = ncode / 4;
        const int gx = (int)std::min<long long>((n4 + LOSS_THREADS - 1) / LOSS_THREADS, 64);
        hipLaunchKernelGGL(bpd_gather_rows_kernel, dim3(gx, R), dim3(LOSS_THREADS), 0, s, reinterpret_cast<const float4*>(code_emb), rows, n4,
                           reinterpret_cast<float4*>(code_out));
        DTTS_CHECK_HIP(hipGetLastError());
    }
}

void launch_diff_bpd_terms(const float* model_out, const float* x_start, int x_start_rows, const float* x_t, const float* noise,
                           const DiffBpdRow* rows, int R, int n, float* partials, float* vb, float* xstart_mse, float* mse, int stride,
                           float* pred_xstart, hipStream_t s) {
    DTTS_REQUIRE(R >= 1 && R <= 65535 && n >= 4 && n % 4 == 0 && stride >= 1, "bpd_terms: 1 .. 65535 rows of a multiple of 4 elements");
    DTTS_REQUIRE(model_out && x_start && x_t && noise && rows && partials && vb && xstart_mse && mse, "bpd_terms: null argument");
    const int nblk = diff_loss_blocks(n);
    hipLaunchKernelGGL(bpd_terms_partials_kernel, dim3(nblk, R), dim3(LOSS_THREADS), 0, s, model_out, x_start, x_start_rows, x_t, noise, rows, n,
                       partials, pred_xstart);
    DTTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(bpd_terms_finish_kernel, dim3(R), dim3(LOSS_THREADS), 0, s, partials, rows, nblk, n, vb, xstart_mse, mse, stride);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_diff_prior_bpd(const float* x_start, float sqrt_ac, float log_1m_ac, int B, int n, float* partials, float* prior, hipStream_t s) {
    DTTS_REQUIRE(B >= 1 && B <= 65535 && n >= 4 && n % 4 == 0, "prior_bpd: 1 .. 65535 rows of a multiple of 4 elements");
    DTTS_REQUIRE(x_start && partials && prior, "prior_bpd: null argument");
    const int nblk = diff_loss_blocks(n);
    hipLaunchKernelGGL(bpd_prior_partials_kernel, dim3(nblk, B), dim3(LOSS_THREADS), 0, s, x_start, sqrt_ac, log_1m_ac, n, partials);
    DTTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(bpd_prior_finish_kernel, dim3(B), dim3(LOSS_THREADS), 0, s, partials, nblk, n, prior);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_diff_bpd_total(const float* vb, const float* prior, int B, int S, float* total, hipStream_t s) {
    DTTS_REQUIRE(vb && prior && total && B >= 1 && S >= 1, "bpd_total: null argument");
    hipLaunchKernelGGL(bpd_total_kernel, dim3((B + LOSS_THREADS - 1) / LOSS_THREADS), dim3(LOSS_THREADS), 0, s, vb, prior, B, S, total);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
