// Elementwise kernels of the flow-VAE stage forward (SynthesizerTrn.forward_flowvae, vqvae/model_24k.py:706-737): the posterior
// sample of enc_q, the forward-direction coupling step, the segment gather and the KL loss.  All fp32, memory-bound; every output
// buffer [B, C, T] is written in full - zeros beyond each row's length, as the reference's `* x_mask` leaves them.
#pragma once
#include "common.h"

namespace dtts {

// PosteriorEncoder.forward's tail (vqvae/model_24k.py:215-217) in one pass: stats [B, 2C, T] = (m | logs), live columns only are read ->
// m_q, logs_q and z = m + eps * exp(logs), each [B, C, T] contiguous with zero tails.  eps = noise[b][c][t] ([B, C, T] contiguous) or,
// noise == null, Philox STAGE_POSTERIOR keyed (seed, sample_ids[b]) over the row's own [C, len] element order (as flow_prior_kernel:
// a row draws the same noise alone and inside a batch).
void launch_posterior_sample(const float* stats, long long s_bs, int s_cs, const int* lens, int T, int B, int C, unsigned long long seed,
                             const int* sample_ids, const float* noise, float* z, float* m_q, float* logs_q, hipStream_t s);

// ResidualCouplingLayer.forward with mean_only (logs = 0), reverse = False, and the Flip that follows it fused into the store
// (vqvae/modules/modules.py:456-471, 393-398): y = flip_channels(cat(x0, m + x1)) on live columns, zeros beyond them.  x, y [B, Ctot, T]
// with strides (bs, cs), m [B, Ctot / 2, T] with the same cs.  y must not alias x.
void launch_coupling_forward(const float* x, const float* m, float* y, long long bs, int cs, const int* lens, int T, int B, int Ctot,
                             int flip, hipStream_t s);

// commons.slice_segments (vqvae/modules/commons.py:67-73): out[b, c, j] = x[b, c, ids[b] + j], j < seg.  The caller has checked
// 0 <= ids[b] and ids[b] + seg <= T.
void launch_slice_segments(const float* x, const int* ids, int B, int C, int T, int seg, float* out, hipStream_t s);

// y[b, c, t] = x[b, c, t] (x strided) for t < len, else tail[c] (tail == null: 0); y [B, C, T] contiguous
void launch_masked_copy(const float* x, long long x_bs, int x_cs, const int* lens, int T, int B, int C, const float* tail, float* y,
                        hipStream_t s);

// losses.kl_loss (vqvae/modules/losses.py:43-58): out[0] = sum_{b, c, t < len_b} (logs_p - logs_q - 1/2 + 1/2 (z_p - m_p)^2 exp(-2 logs_p))
// / frames, frames = sum_b len_b (frames, not frames x channels).  Inputs [B, C, T] contiguous.  Fixed-order reduction: a block sums
// KL_SPAN elements of one row (thread, lane, wave order), a finishing block adds the partials in index order in fp64 - two calls give
// the same bits.  partials: kl_partials(C * T) * B floats.
constexpr int KL_SPAN = 1024;
static inline int kl_partials(long long n) { return (int)((n + KL_SPAN - 1) / KL_SPAN); }
void launch_kl_loss(const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, const int* lens, int B, int C, int T,
                    double frames, float* partials, float* out, hipStream_t s);

}  // namespace dtts
