// Evaluation losses of the diffusion and VQ stages on the model runtime (see model.h, diff_loss.h): GaussianDiffusion.q_sample and
// training_losses (vqvae/utils/diffusion.py:243-260, 930-1012) around the per-row trunk forward, and forward_vq's L1 mean.
#include "model.h"

namespace dtts {

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

const Schedule& Model::loss_schedule(int sched_id, const int* t_host, int B, const char* who) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(B >= 1 && t_host, std::string(who) + ": B, t");
    const Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, std::string(who) + " runs on an integer-timestep schedule (dtts_diff_schedule)");
    for (int b = 0; b < B; ++b) DTTS_REQUIRE(t_host[b] >= 0 && t_host[b] < sc.n, std::string(who) + ": t outside [0, steps of the schedule)");
    return sc;
}

const DiffLossCoefs* Model::upload_loss_coefs(const Schedule& sc, const int* t_host, int B, hipStream_t s) {
    std::vector<DiffLossCoefs> k(B);
    for (int b = 0; b < B; ++b) {
        const int i = t_host[b];
        const DiffStepCoefs& p = sc.p[i];
        k[b] = {sc.sqrt_ac[i], sc.sqrt_1m_ac[i], p.sqrt_recip_ac, p.sqrt_recipm1_ac, p.coef1, p.coef2, p.min_log, p.max_log, i == 0 ? 1 : 0, 0};
    }
    return reinterpret_cast<const DiffLossCoefs*>(upload_ints(reinterpret_cast<const int*>(k.data()), B * DIFF_LOSS_COEF_WORDS, s));
}

int Model::diff_schedule_qtable(int sched_id, float* out, int cap) {
    const Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, "diff_schedule_qtable: not an integer-timestep schedule");
    for (int i = 0; i < sc.n && i < cap && out; ++i) {
        out[2 * i] = sc.sqrt_ac[i];
        out[2 * i + 1] = sc.sqrt_1m_ac[i];
    }
    return sc.n;
}

void Model::diff_q_sample(int sched_id, const float* mel, int normalize, const int* t_host, const float* noise, unsigned long long seed,
                          const int* sample_ids_host, int B, int T, float* x_start_out, float* x_t_out, float* noise_out, hipStream_t s) {
    const Schedule& sc = loss_schedule(sched_id, t_host, B, "diff_q_sample");
    DTTS_REQUIRE(mel && x_t_out && T >= 1 && (noise || sample_ids_host), "diff_q_sample: mel, x_t, noise or sample_ids");
    DTTS_REQUIRE(aligned16(mel) && aligned16(noise) && aligned16(x_start_out) && aligned16(x_t_out) && aligned16(noise_out),
                 "diff_q_sample: 16-byte aligned buffers");
    const DiffLossCoefs* k = upload_loss_coefs(sc, t_host, B, s);
    const int* sids = noise ? nullptr : upload_ints(sample_ids_host, B, s);
    launch_diff_q_sample(mel, normalize, k, noise, seed, sids, B, cfg.mel_channels * T, x_start_out, x_t_out, noise_out, s);
}

void Model::diff_loss_terms(int sched_id, const float* model_out, const float* x_start, const float* x_t, const float* noise, const int* t_host,
                            int B, int T, float* terms_out, float* pred_xstart, hipStream_t s) {
    const Schedule& sc = loss_schedule(sched_id, t_host, B, "diff_loss_terms");
    DTTS_REQUIRE(model_out && x_start && x_t && noise && terms_out && T >= 1, "diff_loss_terms: null argument");
    DTTS_REQUIRE(cfg.diff_out_channels == 2 * cfg.mel_channels, "diff_loss_terms: the model output is (eps | var) over the mel channels");
    DTTS_REQUIRE(aligned16(model_out) && aligned16(x_start) && aligned16(x_t) && aligned16(noise) && aligned16(pred_xstart),
                 "diff_loss_terms: 16-byte aligned buffers");
    const int n = cfg.mel_channels * T;
    ws().ensure(sizeof(float) * (size_t)B * diff_loss_blocks(n) * 2 + 4096);
    float* partials = ws().f32((size_t)B * diff_loss_blocks(n) * 2);
    launch_diff_loss_terms(model_out, x_start, x_t, noise, upload_loss_coefs(sc, t_host, B, s), B, n, partials, terms_out, pred_xstart, s);
}

// training_losses on the frozen model: q_sample -> the conditional trunk forward, row b at column t[b] -> the loss terms
void Model::diff_training_losses(int sched_id, const float* x_start, const int* t_host, const float* noise, unsigned long long seed,
                                 const int* sample_ids_host, const float* code_emb, const int* lens_host, int B, int T, float* terms_out,
                                 float* pred_xstart, hipStream_t s) {
    const Schedule& sc = loss_schedule(sched_id, t_host, B, "diff_training_losses");
    DTTS_REQUIRE(x_start && code_emb && terms_out && T >= 1 && (noise || sample_ids_host), "diff_training_losses: null argument");
    DTTS_REQUIRE(!opt_trunk_fp16_, "diff_training_losses runs the three-product trunk only: set trunk_fp16 = 0 for this call");
    DTTS_REQUIRE(cfg.diff_out_channels == 2 * cfg.mel_channels, "diff_training_losses: the model output is (eps | var) over the mel channels");
    DTTS_REQUIRE(aligned16(x_start) && aligned16(noise) && aligned16(pred_xstart), "diff_training_losses: 16-byte aligned buffers");
    const int C = cfg.diff_channels, MC = cfg.mel_channels, n = MC * T;
    const size_t row = (size_t)B * n, npart = (size_t)B * diff_loss_blocks(n) * 2;
    ws().ensure(rows_ws_bytes(B, C, T) + sizeof(float) * (4 * row + npart) + 8192);
    float* x_t = ws().f32(row);
    float* drawn = noise ? nullptr : ws().f32(row);
    float* model_out = ws().f32(2 * row);
    float* partials = ws().f32(npart);
    const DiffLossCoefs* k = upload_loss_coefs(sc, t_host, B, s);
    const int* sids = noise ? nullptr : upload_ints(sample_ids_host, B, s);
    launch_diff_q_sample(x_start, 0, k, noise, seed, sids, B, n, nullptr, x_t, drawn, s);
    diff_forward_rows_s(sc, x_t, code_emb, lens_host, B, T, t_host, model_out, s);
    launch_diff_loss_terms(model_out, x_start, x_t, noise ? noise : drawn, k, B, n, partials, terms_out, pred_xstart, s);
}

void Model::l1_mean(const float* a, const float* b, int B, int C, int T, float* out, hipStream_t s) {
    DTTS_REQUIRE(a && b && out && B >= 1 && C >= 1 && T >= 1, "l1_mean: null argument");
    DTTS_REQUIRE(aligned16(a) && aligned16(b), "l1_mean: 16-byte aligned buffers");
    const long long n = (long long)B * C * T;
    DTTS_REQUIRE(n % 4 == 0, "l1_mean: B C T must be a multiple of 4");
    ws().ensure(sizeof(float) * (size_t)diff_loss_blocks(n) + 4096);
    float* partials = ws().f32((size_t)diff_loss_blocks(n));
    launch_l1_mean(a, b, n, partials, out, s);
}

}  // namespace dtts
