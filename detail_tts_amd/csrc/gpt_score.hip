// Log-probability of given mel codes under the GPT's own (unprocessed) distribution, from latents the project already has:
//     logprob[b][k] = log_softmax(mel_head(latents_cm[b, :, k]))[targets[b][k]]        (gpt/model.py:408-415 + log_softmax + gather)
// mel_head (768 -> V = 8194, bias) as an fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32, the staging of conv_gemm_kernel.h) FUSED with an
// online log-sum-exp over V and the gather of the target's logit: the [B, V, n] logits (20 MB per row at n = 600) never exist unless
// the caller asks for them (logits_out).
//
// Tiling.  A workgroup (4 waves) owns 128 columns (positions) of ONE row of the batch and one SPLIT of V: SCORE_CHUNKS chunks of 128
// packed weight rows.  Wave w owns columns [32 w, 32 w + 32) against all 128 rows of the chunk (4 MFMA tiles of 32 x 32), so a
// column's 128 logits of a chunk sit in ONE wave: in the 64 accumulator registers of lanes l and l ^ 32.  The per-column reduction is
// therefore 64 values in registers + one shuffle - no LDS, no atomics.  Each lane keeps the running (max, sum, target logit) of its
// column over the chunks of the split; the split's result goes to part[split][column][3].  A second kernel merges the splits of a
// column IN SPLIT ORDER and writes target - (max + log(sum)), or 0.0 for columns at / beyond ntargets[b]: the summation order is a
// function of the shapes only, two runs give the same bits, and a column's value does not depend on what else is in the batch.
//
// V tail.  The packed weights are zero-padded to CoutP = ceil128(V) rows (8320 for 8194): rows >= V are computed by the MFMAs (their
// logit is bias padding = 0) and masked out of the max, the sum, the gather and logits_out.
//
// LDS: 2 x [16][128] weights (LDS-DMA) + 2 x [16][129] latents = 32.5 KB, double-buffered over the K steps of 16 channels.
#include "gpt_kernels.h"
#include "prof.h"

namespace dtts {

typedef float floatx16s __attribute__((ext_vector_type(16)));

constexpr int SC_BM = 128, SC_BN = 128, SC_BK = 16, SC_XP = SC_BN + 1;

__global__ __launch_bounds__(256) void gpt_score_kernel(const ScoreParams p) {
    __shared__ float Ws[2 * SC_BK * SC_BM];
    __shared__ float Xs[2 * SC_BK * SC_XP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int b = p.tiles[2 * blockIdx.x], n0 = p.tiles[2 * blockIdx.x + 1];
    const int split = blockIdx.y;
    const int nt = p.ntargets[b];                          // > n0 (the host lists live tiles only)
    const int chunk0 = split * SCORE_CHUNKS;
    const int nch = min(SCORE_CHUNKS, p.CoutP / SC_BM - chunk0);
    const int KS = p.CinP / SC_BK;
    const int S = nch * KS;

    const float* xb = p.lat + (long long)b * p.lat_bs;
    // this thread's staged latent columns (wave w stages channel rows 4 w .. 4 w + 3 of a K step, lanes stride over the 128 columns)
    int xoff[2];
    bool xok[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int col = n0 + lane + 64 * c;
        xok[c] = col < nt;
        xoff[c] = min(col, nt - 1);
    }
    float xreg[4][2];
    auto load_w = [&](int chunk, int ks, int buf) {       // [16][128] tile, lane-linear in LDS (conv_gemm_kernel.h)
        const float* wp = p.w + (long long)(ks * SC_BK) * p.CoutP + (long long)(chunk0 + chunk) * SC_BM;
        float* lbase = Ws + buf * SC_BK * SC_BM;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * 256;
            const int row = idx / (SC_BM / 4), c4 = idx - row * (SC_BM / 4);
            const float* g = wp + (long long)row * p.CoutP + c4 * 4;
            float* l = lbase + (wave * 64 + i * 256) * 4;      // wave-uniform base; hardware adds lane * 16
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0,
                                             0);
        }
    };
    auto load_x = [&](int ks) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ci = ks * SC_BK + wave * 4 + r;
            const bool cok = ci < p.C;
            const float* xr = xb + (long long)(cok ? ci : p.C - 1) * p.lat_cs;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float v = xr[xoff[c]];
                xreg[r][c] = (cok && xok[c]) ? v : 0.f;
            }
        }
    };
    auto store_x = [&](int buf) {
        float* dst = Xs + buf * SC_BK * SC_XP + (wave * 4) * SC_XP + lane;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) dst[r * SC_XP + 64 * c] = xreg[r][c];
    };

    floatx16s acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    const int col = n0 + wave * 32 + l31;                  // this lane's column (shared with lane ^ 32)
    const bool colok = col < nt;
    const int tgt = p.targets[(long long)b * p.n_max + min(col, nt - 1)];
    float run_m = -INFINITY, run_s = 0.f, run_t = -INFINITY;

    load_w(0, 0, 0);
    load_x(0);
    store_x(0);
    __syncthreads();

    int chunk = 0, ks = 0;
    for (int s = 0; s < S; ++s) {
        const bool has_next = (s + 1) < S;
        int nks = ks + 1, nchunk = chunk;
        if (nks == KS) { nks = 0; nchunk = chunk + 1; }
        if (has_next) {
            load_w(nchunk, nks, (s + 1) & 1);
            load_x(nks);
        }
        const float* wq = Ws + (s & 1) * SC_BK * SC_BM + lhi * SC_BM + l31;
        const float* xq = Xs + (s & 1) * SC_BK * SC_XP + lhi * SC_XP + wave * 32 + l31;
        float af[SC_BK / 2][4], bf[SC_BK / 2];
#pragma unroll
        for (int kk = 0; kk < SC_BK / 2; ++kk) {
#pragma unroll
            for (int i = 0; i < 4; ++i) af[kk][i] = wq[kk * 2 * SC_BM + i * 32];
            bf[kk] = xq[kk * 2 * SC_XP];
        }
#pragma unroll
        for (int kk = 0; kk < SC_BK / 2; ++kk)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk][i], bf[kk], acc[i], 0, 0, 0);

        if (ks == KS - 1) {
            // ---- the chunk's 128 logits of this lane's column: rows m0 + 32 i + (r & 3) + 8 (r >> 2) + 4 lhi  (32 x 32 MFMA C layout)
            const int m0 = (chunk0 + chunk) * SC_BM;
            float cm = -INFINITY, ct = -INFINITY;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                    const float v = acc[i][r] + p.bias[row];          // bias is padded to CoutP
                    acc[i][r] = v;
                    if (row < p.V) {
                        cm = fmaxf(cm, v);
                        if (row == tgt) ct = v;
                        if (p.logits_out && colok) p.logits_out[((long long)b * p.V + row) * p.n_max + col] = v;
                    }
                }
            cm = fmaxf(cm, __shfl_xor(cm, 32));
            ct = fmaxf(ct, __shfl_xor(ct, 32));
            if (cm > -INFINITY) {                                     // (every chunk has a valid row: the last one starts below V)
                const float nm = fmaxf(run_m, cm);
                float cs = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                        if (row < p.V) cs += expf(acc[i][r] - nm);
                    }
                cs += __shfl_xor(cs, 32);
                run_s = run_s * expf(run_m - nm) + cs;                // run_m = -inf at first: exp(-inf) = 0, run_s = 0
                run_m = nm;
            }
            run_t = fmaxf(run_t, ct);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        }

        if (has_next) store_x((s + 1) & 1);
        __syncthreads();
        ks = nks;
        chunk = nchunk;
    }
    if (lhi == 0 && colok) {
        float* q = p.part + ((long long)split * p.B * p.n_max + (long long)b * p.n_max + col) * 3;
        q[0] = run_m;
        q[1] = run_s;
        q[2] = run_t;
    }
}

// splits of a column merged in split order; columns at / beyond ntargets[b]: 0.0
__global__ void gpt_score_merge_kernel(const float* part, int nsplit, const int* ntargets, int B, int n_max, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * n_max) return;
    const int b = i / n_max, k = i - b * n_max;
    if (k >= ntargets[b]) {
        out[i] = 0.f;
        return;
    }
    const long long stride = (long long)B * n_max * 3;
    float m = -INFINITY, t = -INFINITY;
    for (int s = 0; s < nsplit; ++s) {
        m = fmaxf(m, part[s * stride + (long long)i * 3]);
        t = fmaxf(t, part[s * stride + (long long)i * 3 + 2]);
    }
    float sum = 0.f;
    for (int s = 0; s < nsplit; ++s) sum += part[s * stride + (long long)i * 3 + 1] * expf(part[s * stride + (long long)i * 3] - m);
    out[i] = t - (m + logf(sum));
}

int gpt_score_splits(int CoutP) { return cdiv(CoutP / SC_BM, SCORE_CHUNKS); }

size_t gpt_score_part_floats(int B, int n_max, int CoutP) { return (size_t)gpt_score_splits(CoutP) * B * n_max * 3; }

void launch_gpt_score(const ScoreParams& p, int ntiles, hipStream_t s) {
    DTTS_REQUIRE(p.CoutP % SC_BM == 0 && p.CinP % SC_BK == 0 && p.C <= p.CinP && p.V <= p.CoutP && p.V > p.CoutP - SC_BM, "gpt_score: packed mel_head shape");
    DTTS_REQUIRE(p.bias && p.w && p.part, "gpt_score: operands");
    const int nsplit = gpt_score_splits(p.CoutP);
    if (ntiles > 0) {
        const double cols = (double)ntiles * SC_BN;
        ProfScope ps("gpt_score", 2.0 * p.V * p.C * cols, 4.0 * ((double)p.CoutP * p.CinP * ntiles + cols * p.C), s);
        hipLaunchKernelGGL(gpt_score_kernel, dim3(ntiles, nsplit), dim3(256), 0, s, p);
        DTTS_CHECK_HIP(hipGetLastError());
    }
    const int total = p.B * p.n_max;
    hipLaunchKernelGGL(gpt_score_merge_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, p.part, nsplit, p.ntargets, p.B, p.n_max, p.out);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
