// The variational bound of the diffusion decoder in bits per dimension (diff_bpd.hip): GaussianDiffusion.calc_bpd_loop with
// _vb_terms_bpd and _prior_bpd beneath it (vqvae/utils/diffusion.py:903-928, 1098-1169).  The loop's 200 timesteps of an utterance run
// as "virtual rows" of the per-row trunk forward: row r stands for (utterance b(r), timestep t(r)).  fp32, no atomics: every sum is
// block partials in a fixed order, then one finishing pass (diff_loss.h) - two calls give the same bits, and a row's values depend
// neither on the other rows of its pass nor on how the (b, t) pairs were grouped into passes.
#pragma once
#include <hip/hip_runtime.h>

#include "diff_loss.h"

namespace dtts {

// one virtual row: its timestep's column of the schedule, the utterance it reads, and where its three terms go
struct DiffBpdRow {
    DiffLossCoefs k;
    int b;                                  // utterance: x_start[b]
    int t;                                  // timestep: the Philox step of the row's noise / the index into a given noise [S][B][n]
    int dst;                                // the row's terms land at out[dst * stride]
    int sid;                                // the utterance's Philox stream (sample_ids[b])
};
static constexpr int DIFF_BPD_ROW_WORDS = sizeof(DiffBpdRow) / 4;

// x_t[r] = sqrt_ac[t(r)] x_start[b(r)] + sqrt_1m_ac[t(r)] z over [R][n]; z = noise[t(r)][b(r)] of a given [S][B][n] array, or (noise
// null) drawn from Philox (STAGE_DIFF_BPD, step t(r), stream sid(r), element order [C, T]).  z is written to noise_out [R][n].
// code_emb / code_out (both or neither): code_out[r] = code_emb[b(r)] over ncode elements per row, the trunk's per-row conditioning.
void launch_diff_bpd_q_sample(const float* x_start, const DiffBpdRow* rows, const float* noise, unsigned long long seed, int B, int R,
                              int n, float* x_t_out, float* noise_out, const float* code_emb, float* code_out, long long ncode,
                              hipStream_t s);

// per row r, of model_out [R][2n] (eps | v) against x_start[b(r)] (x_start_rows != 0: x_start[r]), x_t [R][n], noise [R][n]:
//   vb = _vb_terms_bpd's output (:903-928) as launch_diff_loss_terms computes it;
//   xstart_mse = mean (pred_xstart - x_start)^2 with pred_xstart = clamp(_predict_xstart_from_eps, -1, 1) (:1153);
//   mse = mean (eps' - noise)^2, eps' = _predict_eps_from_xstart of that clamped start (:1154-1155)
// written to vb[dst(r) * stride], xstart_mse[...], mse[...].  pred_xstart (optional) [R][n]: the clamped start.
// partials: R * diff_loss_blocks(n) * 3 floats of scratch.
void launch_diff_bpd_terms(const float* model_out, const float* x_start, int x_start_rows, const float* x_t, const float* noise,
                           const DiffBpdRow* rows, int R, int n, float* partials, float* vb, float* xstart_mse, float* mse, int stride,
                           float* pred_xstart, hipStream_t s);

// _prior_bpd (:1098-1112): prior[b] = mean normal_kl(sqrt_ac x_start[b], log_1m_ac, 0, 0) / ln 2 with the LAST column's two table
// values.  partials: B * diff_loss_blocks(n) floats of scratch.
void launch_diff_prior_bpd(const float* x_start, float sqrt_ac, float log_1m_ac, int B, int n, float* partials, float* prior, hipStream_t s);

// total[b] = (vb[b][0] + vb[b][1] + ... + vb[b][S - 1]) + prior[b], one thread per utterance, fp32 in column order (:1162)
void launch_diff_bpd_total(const float* vb, const float* prior, int B, int S, float* total, hipStream_t s);

}  // namespace dtts
