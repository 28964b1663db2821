// Kernels of the MultiPeriodDiscriminator forward (vqvae/model_24k.py:298-431) and of the losses that consume it
// (vqvae/modules/losses.py:4-40): the period split with its reflect pad, the Cin = 1 first layers, DiscriminatorS' grouped strided
// convs, the time de-interleave that turns a stride-3 conv into a stride-1 GEMM operand, and one fixed-order reduction for every
// mean the three loss functions take.  All fp32, plain FMAs (no packed-fp32 instructions: DESIGN.md par. 4.9).  The dense convs and
// the conv_posts are conv_gemm.h launches (model_disc.hip).
#pragma once
#include "common.h"

namespace dtts {

constexpr int DISC_COUNT = 6;                      // DiscriminatorS + DiscriminatorP of periods 2, 3, 5, 7, 11
constexpr int DISC_MAPS = 37;                      // feature maps: 7 of DiscriminatorS (6 convs + conv_post), 6 of each DiscriminatorP
constexpr float DISC_SLOPE = 0.1f;                 // modules.LRELU_SLOPE

// DiscriminatorP.forward's head (vqvae/model_24k.py:359-364) for N = B (+ B) waveforms of t samples: rows n < B come from y, the
// others from y_hat (null: N == B).  out [N * p][H], H = ceil(t / p): out[n * p + w][h] = x[n][h * p + w], the index reflected at the
// right end (i >= t -> 2 (t - 1) - i: F.pad(x, (0, p - t % p), "reflect")).  The caller has checked t > p - 1.  p = 1 is a plain gather
// of the 2B rows (DiscriminatorS' input).
void launch_period_split(const float* y, const float* y_hat, int B, int N, int t, int p, float* out, hipStream_t s);

// Conv1d(1, Cout, K, stride, pad) + leaky-relu on R rows: x [R][Tin], w [Cout][K], b [Cout] -> y [R][Cout][Nout].  K = 5 or 15.
void launch_disc_first(const float* x, const float* w, const float* b, int R, int Tin, int Cout, int K, int stride, int pad, float slope,
                       float* y, int Nout, hipStream_t s);

// Grouped Conv1d + leaky-relu (slope 1: none): x [R][Cin][Tin], w [Cout][Cin / groups][K] (the reference's layout), b [Cout] (or null)
// -> y [R][Cout][Nout], Nout = (Tin + 2 pad - K) / stride + 1.  A workgroup owns GC_TN output columns of one (row, group): the group's
// input window [Cin / groups][(GC_TN - 1) stride + K] and its weights are staged in LDS once, then each thread accumulates, in fp32,
// one column of (Cout / groups) / 4 output channels (16 or 4 channels per group).
constexpr int GC_TN = 64;
void launch_conv1d_grouped(const float* x, const float* w, const float* b, int R, int Cin, int Tin, int Cout, int groups, int K, int stride,
                           int pad, float slope, float* y, int Nout, hipStream_t s);

// out [R][3 C][M], M = ceil(H / 3): out[r][3 c + j][m] = x[r][c][3 m + j] (0 beyond H).  A (5, stride 3, pad 2) conv over x is the
// (2 taps, stride 1, left pad 1) conv over `out` with weights (0, w0, w1 | w2, w3, w4) (packing.pack_discriminator), which the conv
// GEMM's input staging can hold (its tile is at most 192 input columns wide; 64 outputs at stride 3 with 5 taps need 194).
void launch_deinterleave3(const float* x, int R, int C, int H, float* out, hipStream_t s);

// ---- the reductions.  An item is one mean over n elements: mode 0 |a - b|, 1 (1 - a)^2, 2 a^2.  Two levels, fixed order: a block adds
// LOSS_SPAN elements of one item in fp32 (thread, lane, wave order), one finishing block per item adds the item's partials in index
// order in fp64 and divides by n - two calls give the same bits.
constexpr int LOSS_SPAN = 1024;
constexpr int LOSS_MAX_ITEMS = 64;
enum LossMode : int { LOSS_ABS_DIFF = 0, LOSS_ONE_MINUS_SQ = 1, LOSS_SQ = 2 };
struct LossItem {
    const float* a;
    const float* b;
    long long n;
    int blk0;          // first partial of this item
    int mode;
};
struct LossItems {
    LossItem it[LOSS_MAX_ITEMS];
    int n = 0;
    int blocks = 0;
    void add(const float* a, const float* b, long long n_, int mode) {
        it[n].a = a; it[n].b = b; it[n].n = n_; it[n].blk0 = blocks; it[n].mode = mode;
        blocks += (int)((n_ + LOSS_SPAN - 1) / LOSS_SPAN);
        ++n;
    }
};
// means [items.n]; partials [items.blocks]
void launch_loss_means(const LossItems& items, float* partials, float* means, hipStream_t s);

// Layout of the scalars the loss entries return (floats): see include/detail_hip.h (DTTS_DISC_LOSS_FM and the slots after it).
// means: n_maps |r - g| means, then (n_scores > 0) n_scores (1 - dr)^2, n_scores dg^2, n_scores (1 - dg)^2, in this order; has_real = 0:
// the dr items are absent (generator_loss alone).  The sums are taken in list order in fp32, as the reference's `loss += ...` does.
void launch_disc_combine(const float* means, int n_maps, int n_scores, int has_real, float* out, hipStream_t s);
// out[LOSS_MEL] = 45 mel_l1, out[LOSS_KL] = kl, out[LOSS_GEN_ALL] = loss_gen + loss_fm + loss_mel + loss_kl (train.py:307-312)
void launch_stage_combine(const float* mel_l1, const float* kl, float* out, hipStream_t s);

}  // namespace dtts
