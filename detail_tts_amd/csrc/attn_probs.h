// Attention probabilities of a window, and the monotone path over a score matrix (attn_probs.hip, align_path.hip).
#pragma once
#include "common.h"

namespace dtts {

enum AttnProbsMode : int { ATTN_PROBS_HEADS = 0, ATTN_PROBS_MEAN = 1 };

// P_h[t, s] = softmax_s(scale q_t . k_s) under the causal rule s <= t, s < len_b, of ONE layer's fp32 qkv rows (addressed as in
// AttnParams: row of (head h, dim c) = off + h * head_stride + c).  The denominator runs over ALL of the row's keys; only the window
// queries [q0_b, q0_b + nq_b) x keys [k0_b, k0_b + nk_b) is written (element (i, j) <-> t = q0_b + i, s = k0_b + j):
//   HEADS  out[b][h][i][j] = P_h                                  out [B][H][nq_max][nk_max]
//   MEAN   out[b][i][j] (= | +=) sum_h w[h] P_h                    out [B][nq_max][nk_max]; `first` stores, else adds to what is there
// A key s > t inside the window is written as exactly 0 (in MEAN mode it contributes exactly 0).  Elements outside a sample's
// nq_b x nk_b and rows t >= len_b are never touched.  One thread owns an element for every head (ascending h, fp32): no atomics.
// A struct of its own: AttnParams is the flash kernels' argument and its layout is frozen (attention.h).
struct AttnProbsParams {
    const float* qkv = nullptr;   // [B, rows, cs]
    long long bs = 0;
    int cs = 0;
    int q_off = 0, k_off = 0, head_stride = 0;
    const int* lens = nullptr;    // [B] device
    const int* q0 = nullptr;      // [B] device, each of the four
    const int* nq = nullptr;
    const int* k0 = nullptr;
    const int* nk = nullptr;
    int B = 0, H = 0, D = 0;
    int nq_max = 0, nk_max = 0;
    float scale = 1.f;
    int mode = ATTN_PROBS_HEADS;
    float* out = nullptr;
    const float* w = nullptr;     // [H] device (MEAN)
    int first = 1;                // MEAN: 1 = store, 0 = accumulate
};
void launch_attn_probs(const AttnProbsParams& p, hipStream_t stream);      // D == 48 only; anything else throws before the launch
// out[b][i] = sum_j x[b][i][j], j < nk_b ascending in fp32, rows i < nq_b (the text mass of an alignment row); the rest is untouched
void launch_window_row_sums(const float* x, const int* nq, const int* nk, int B, int nq_max, int nk_max, float* out, hipStream_t stream);

// dp[0][i] = score[0][i]; dp[j][i] = score[j][i] + max_{i' <= i} dp[j-1][i'] (prefix argmax: the lowest index on ties); the path ends at
// the lowest argmax of row n_b - 1 and is backtracked on the device.  score [B][n_max][m_max] fp32, n / m device [B] (m_b >= 1 where
// n_b >= 1), back [B][n_max][m_max] int16 workspace, path [B][n_max] int32 (-1 at j >= n_b).  One workgroup per sample; m_max <= 1024.
constexpr int ALIGN_PATH_MAX_M = 1024;
void launch_monotone_path(const float* score, const int* n, const int* m, int B, int n_max, int m_max, short* back, int* path,
                          hipStream_t stream);

}  // namespace dtts
