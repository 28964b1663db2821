// Attention probabilities of a (query, key) window of one causal fp32 attention layer, for gfx950 (attn_probs.h).
//
// flash_attn_kernel keeps P in registers by design; this kernel is its read-out.  The score tile is computed exactly as there - transposed,
// S^T[s, t] = K^T Q on v_mfma_f32_16x16x4_f32 (exact fp32, q pre-scaled by scale * log2(e), softmax on exp2) - so that a query's scores
// sit in the 4 x 4 registers of 4 lanes.  Two passes per 64-query tile and head: (1) the row statistics (m, l) over ALL keys s <= t of the
// row, online over 64-key tiles; (2) the key tiles that meet the window once more, written as exp2(S - m) / l.  K is staged K-major
// [D][64] (pitch 80) in LDS as in attention.hip.  A workgroup is 4 waves x 16 queries; wave w owns window rows i0 + 16 w .. + 15.
#include "attn_probs.h"
#include "prof.h"

namespace dtts {

typedef float floatx4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int KT = 64;        // keys per LDS tile
constexpr int KPITCH = 80;    // K tile row pitch (== 16 mod 32)
constexpr int QPW = 16;       // queries per wave
constexpr int QPB = 64;       // queries per workgroup
}  // namespace

template <int D>
__global__ __launch_bounds__(256) void attn_probs_kernel(const AttnProbsParams p) {
    constexpr int DS = D / 4;
    constexpr int NLD = (D * KT) / 256;
    constexpr float LOG2E = 1.4426950408889634f;
    __shared__ float Ks[D * KPITCH];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int b = blockIdx.z;
    const int len = p.lens[b], q0 = p.q0[b], nq = p.nq[b], k0 = p.k0[b], nk = p.nk[b];
    const int i0 = blockIdx.x * QPB;
    if (i0 >= nq || nk <= 0 || q0 + i0 >= len) return;          // workgroup-uniform: nothing of this tile is written
    const int h0 = p.mode == ATTN_PROBS_MEAN ? 0 : blockIdx.y;
    const int h1 = p.mode == ATTN_PROBS_MEAN ? p.H : h0 + 1;

    const int iw = i0 + wave * QPW + j;                          // this lane's window row
    const int t = q0 + iw;
    const bool row_ok = iw < nq && t < len;
    const int tc = t < len ? t : len - 1;                        // (rows that are not written still load valid columns)
    const bool wave_active = (i0 + wave * QPW < nq) && (q0 + i0 + wave * QPW < len);
    const int ilast = (i0 + QPB < nq ? i0 + QPB : nq) - 1;
    const int tlast = q0 + ilast < len ? q0 + ilast : len - 1;   // the last live query of the tile: keys beyond it never matter
    const int nt1 = tlast / KT + 1;
    const int kta = k0 / KT, ktb = (k0 + nk - 1) / KT;

    const float* base = p.qkv + (long long)b * p.bs;
    const int sl = tid & (KT - 1), c0 = tid / KT;
    const float qs = p.scale * LOG2E;

    for (int h = h0; h < h1; ++h) {
        const float* qp = base + (long long)(p.q_off + h * p.head_stride) * p.cs;
        const float* kp = base + (long long)(p.k_off + h * p.head_stride) * p.cs;
        float qreg[DS];
#pragma unroll
        for (int st = 0; st < DS; ++st) qreg[st] = qp[(long long)(4 * st + g) * p.cs + tc] * qs;

        // K tile kt -> LDS (keys >= len read column len - 1: finite, and masked by s > t wherever they are used)
        auto stage = [&](int kt) {
            const int s = kt * KT + sl;
            const int sc = s < len ? s : len - 1;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NLD; ++i) Ks[(c0 + 4 * i) * KPITCH + sl] = kp[(long long)(c0 + 4 * i) * p.cs + sc];
            __syncthreads();
        };
        // S^T = K^T Q of the staged tile: sacc[ks][r] = score of key ks * 16 + 4 g + r and query j (log2 domain)
        auto scores = [&](floatx4 (&sacc)[4]) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) sacc[ks] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < DS; ++st)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    sacc[ks] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[(4 * st + g) * KPITCH + ks * 16 + j], qreg[st], sacc[ks], 0, 0, 0);
        };

        // ---- pass 1: (m, l) of every row over ALL its keys s <= t
        float m_run = -INFINITY, l_run = 0.f;
        for (int kt = 0; kt < nt1; ++kt) {
            stage(kt);
            if (!wave_active) continue;
            floatx4 sacc[4];
            scores(sacc);
            float mx = -INFINITY;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = kt * KT + ks * 16 + 4 * g + r;
                    const float v = (s > tc) ? -INFINITY : sacc[ks][r];
                    sacc[ks][r] = v;
                    mx = fmaxf(mx, v);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m_run, mx);
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
            float sum = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int r = 0; r < 4; ++r) sum += __builtin_amdgcn_exp2f(sacc[ks][r] - m_use);
            sum += __shfl_xor(sum, 16);
            sum += __shfl_xor(sum, 32);
            l_run = l_run * alpha + sum;
            m_run = m_new;
        }
        const float inv = 1.f / l_run;           // key 0 is live for every row: l_run >= 1 ulp-wise, m_run finite

        // ---- pass 2: the key tiles that meet the window
        const float wh = p.mode == ATTN_PROBS_MEAN ? p.w[h] : 0.f;
        const bool store = p.mode == ATTN_PROBS_MEAN && p.first && h == 0;
        float* orow = p.mode == ATTN_PROBS_MEAN ? p.out + ((long long)b * p.nq_max + iw) * p.nk_max
                                                : p.out + (((long long)b * p.H + h) * p.nq_max + iw) * p.nk_max;
        for (int kt = kta; kt <= ktb; ++kt) {
            stage(kt);
            if (!wave_active) continue;
            floatx4 sacc[4];
            scores(sacc);
            if (!row_ok) continue;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = kt * KT + ks * 16 + 4 * g + r;
                    const int jj = s - k0;
                    if (jj < 0 || jj >= nk) continue;
                    const float pv = (s > t) ? 0.f : __builtin_amdgcn_exp2f(sacc[ks][r] - m_run) * inv;
                    if (p.mode == ATTN_PROBS_MEAN) {
                        const float prev = store ? 0.f : orow[jj];
                        orow[jj] = prev + wh * pv;
                    } else {
                        orow[jj] = pv;
                    }
                }
        }
    }
}

// out[b][i] = sum_j x[b][i][j] over the row's nk_b columns, j ascending in fp32; one thread per row, rows i >= nq_b untouched
__global__ void window_row_sums_kernel(const float* __restrict__ x, const int* __restrict__ nq, const int* __restrict__ nk, int nq_max, int nk_max,
                                       float* __restrict__ out) {
    const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq[b]) return;
    const float* r = x + ((long long)b * nq_max + i) * nk_max;
    float acc = 0.f;
    for (int jj = 0; jj < nk[b]; ++jj) acc += r[jj];
    out[(long long)b * nq_max + i] = acc;
}

void launch_window_row_sums(const float* x, const int* nq, const int* nk, int B, int nq_max, int nk_max, float* out, hipStream_t stream) {
    if (B <= 0 || nq_max <= 0) return;
    hipLaunchKernelGGL(window_row_sums_kernel, dim3(cdiv(nq_max, 128), B), dim3(128), 0, stream, x, nq, nk, nq_max, nk_max, out);
    DTTS_CHECK_HIP(hipGetLastError());
}

void launch_attn_probs(const AttnProbsParams& p, hipStream_t stream) {
    DTTS_REQUIRE(p.D == 48, "attention probabilities: head dim 48 (the GPT) is the only instantiation");
    DTTS_REQUIRE(p.B > 0 && p.B <= 65535 && p.H > 0 && p.H <= 65535, "attention probabilities: B, H");
    DTTS_REQUIRE(p.mode == ATTN_PROBS_HEADS || p.mode == ATTN_PROBS_MEAN, "attention probabilities: mode");
    DTTS_REQUIRE(p.qkv && p.lens && p.q0 && p.nq && p.k0 && p.nk && p.out && (p.mode == ATTN_PROBS_HEADS || p.w), "attention probabilities: null argument");
    if (p.nq_max <= 0 || p.nk_max <= 0) return;
    dim3 grid(cdiv(p.nq_max, QPB), p.mode == ATTN_PROBS_MEAN ? 1 : p.H, p.B);
    const double pairs = (double)p.B * p.H * p.nq_max * ((double)p.cs + p.nk_max);      // an upper bound: rows are causal and ragged
    ProfScope ps("attn_probs_kernel<48>", 2.0 * pairs * p.D, 4.0 * pairs, stream);
    hipLaunchKernelGGL(attn_probs_kernel<48>, grid, dim3(256), 0, stream, p);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
