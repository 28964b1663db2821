// Evaluation losses of the diffusion and VQ stages (diff_loss.hip): the forward process and the loss arithmetic of
// GaussianDiffusion.training_losses (vqvae/utils/diffusion.py:930-1012), and the L1 mean of forward_vq (vqvae/model_24k.py:664).
// fp32, no atomics: every sum is block partials in a fixed order, then one finishing pass - two calls give the same bits, and a row's
// values do not depend on the rest of the batch.
#pragma once
#include <hip/hip_runtime.h>

namespace dtts {

// what one batch row reads of its timestep's column of a kind-0 schedule (fp32 casts of the float64 tables, :1315)
struct DiffLossCoefs {
    float sqrt_ac, sqrt_1m_ac;             // q_sample (:243-260)
    float sqrt_recip_ac, sqrt_recipm1_ac;  // _predict_xstart_from_eps (:402-405)
    float coef1, coef2;                    // q_posterior_mean_variance (:262-285)
    float min_log, max_log;                // posterior_log_variance_clipped, log(betas): the learned-range ends (:329-335)
    int t0, pad;                           // t == 0: the decoder NLL stands in for the KL (:927)
};
static constexpr int DIFF_LOSS_COEF_WORDS = sizeof(DiffLossCoefs) / 4;

// elements one block of the reductions below covers (256 threads x 4 contiguous floats)
static constexpr int DIFF_LOSS_SPAN = 1024;
static inline int diff_loss_blocks(long long n) { return (int)((n + DIFF_LOSS_SPAN - 1) / DIFF_LOSS_SPAN); }

// x_start = normalize ? normalize_torch_mel(mel) : mel; x_t = sqrt_ac[t_b] x_start + sqrt_1m_ac[t_b] noise  over [B][n] (n = C T).
// noise == null: drawn from Philox (STAGE_DIFF_QSAMPLE, step 0, sample_ids[b], element order [C, T]) and written to noise_out.
// x_start_out / noise_out may be null.  n % 4 == 0, 16-byte aligned rows.
void launch_diff_q_sample(const float* mel, int normalize, const DiffLossCoefs* coefs, const float* noise, unsigned long long seed,
                          const int* sample_ids, int B, int n, float* x_start_out, float* x_t_out, float* noise_out, hipStream_t s);

// per row b: terms[b] = (mse, vb, mse + vb) of model_out [B][2n] (eps | v) against (x_start, x_t, noise) [B][n]; pred_xstart (optional)
// [B][n] = _predict_xstart_from_eps, unclamped as training_losses returns it.  partials: B * diff_loss_blocks(n) * 2 floats of scratch.
void launch_diff_loss_terms(const float* model_out, const float* x_start, const float* x_t, const float* noise, const DiffLossCoefs* coefs,
                            int B, int n, float* partials, float* terms, float* pred_xstart, hipStream_t s);

// out[0] = mean |a - b| over n elements.  partials: diff_loss_blocks(n) floats of scratch.
void launch_l1_mean(const float* a, const float* b, long long n, float* partials, float* out, hipStream_t s);

}  // namespace dtts
