// The diffusion decoder's variational bound in bits per dimension on the model runtime (see model.h, diff_bpd.h):
// GaussianDiffusion.calc_bpd_loop, _vb_terms_bpd and _prior_bpd (vqvae/utils/diffusion.py:903-928, 1098-1169) around the per-row trunk
// forward, with the loop's (utterance, timestep) pairs batched as rows of one launch sequence.
#include "diff_bpd.h"
#include "model.h"

namespace dtts {

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static DiffBpdRow bpd_row(const Schedule& sc, int t, int b, int sid, int dst) {
    const DiffStepCoefs& p = sc.p[t];
    return {{sc.sqrt_ac[t], sc.sqrt_1m_ac[t], p.sqrt_recip_ac, p.sqrt_recipm1_ac, p.coef1, p.coef2, p.min_log, p.max_log, t == 0 ? 1 : 0, 0},
            b, t, dst, sid};
}

void Model::diff_bpd_terms(int sched_id, const float* model_out, const float* x_start, const float* x_t, const float* noise, const int* t_host,
                           int R, int T, float* terms_out, float* pred_xstart, hipStream_t s) {
    const Schedule& sc = loss_schedule(sched_id, t_host, R, "diff_bpd_terms");
    DTTS_REQUIRE(model_out && x_start && x_t && noise && terms_out && T >= 1 && R <= 65535, "diff_bpd_terms: null argument, or more than 65535 rows");
    DTTS_REQUIRE(cfg.diff_out_channels == 2 * cfg.mel_channels, "diff_bpd_terms: the model output is (eps | var) over the mel channels");
    DTTS_REQUIRE(aligned16(model_out) && aligned16(x_start) && aligned16(x_t) && aligned16(noise) && aligned16(pred_xstart),
                 "diff_bpd_terms: 16-byte aligned buffers");
    const int n = cfg.mel_channels * T;
    const size_t npart = (size_t)R * diff_loss_blocks(n) * 3;
    ws().ensure(sizeof(float) * npart + 4096);
    float* partials = ws().f32(npart);
    std::vector<DiffBpdRow> rows(R);
    for (int r = 0; r < R; ++r) rows[r] = bpd_row(sc, t_host[r], r, 0, r);
    const DiffBpdRow* rd = reinterpret_cast<const DiffBpdRow*>(upload_ints(reinterpret_cast<const int*>(rows.data()), R * DIFF_BPD_ROW_WORDS, s));
    launch_diff_bpd_terms(model_out, x_start, 1, x_t, noise, rd, R, n, partials, terms_out, terms_out + 1, terms_out + 2, 3, pred_xstart, s);
}

void Model::diff_prior_bpd(int sched_id, const float* x_start, int B, int T, float* prior_out, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(x_start && prior_out && B >= 1 && B <= 65535 && T >= 1, "diff_prior_bpd: x_start, prior, 1 .. 65535 rows");
    DTTS_REQUIRE(aligned16(x_start), "diff_prior_bpd: 16-byte aligned buffers");
    const Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, "diff_prior_bpd runs on an integer-timestep schedule (dtts_diff_schedule)");
    const int n = cfg.mel_channels * T;
    const size_t npart = (size_t)B * diff_loss_blocks(n);
    ws().ensure(sizeof(float) * npart + 4096);
    launch_diff_prior_bpd(x_start, sc.sqrt_ac[sc.n - 1], sc.log_1m_ac[sc.n - 1], B, n, ws().f32(npart), prior_out, s);
}

// rows per pass when the caller leaves the choice to the library: about 32, fewer for long utterances (the pass's activations grow with
// rows x T)
static int bpd_default_rows(int T) { return std::max(1, std::min(32, 32768 / T)); }

// calc_bpd_loop: the (b, t) pairs in the reference's order (t = S - 1 first, b within t), rows_per_pass at a time:
// q_sample of the pass's rows -> the conditional trunk forward, every row at its own column -> the rows' three terms to [b][S - 1 - t];
// then the prior and the totals
void Model::diff_calc_bpd(int sched_id, const float* x_start, const float* code_emb, const int* lens_host, int B, int T, const float* noise,
                          unsigned long long seed, const int* sample_ids_host, int rows_per_pass, float* vb, float* xstart_mse, float* mse,
                          float* prior, float* total, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && rows_per_pass >= 0 && rows_per_pass <= 65535, "diff_calc_bpd: B, T, rows_per_pass");
    DTTS_REQUIRE(x_start && code_emb && vb && xstart_mse && mse && prior && total && (noise || sample_ids_host), "diff_calc_bpd: null argument");
    DTTS_REQUIRE(!opt_trunk_fp16_, "diff_calc_bpd runs the three-product trunk only: set trunk_fp16 = 0 for this call");
    DTTS_REQUIRE(cfg.diff_out_channels == 2 * cfg.mel_channels, "diff_calc_bpd: the model output is (eps | var) over the mel channels");
    DTTS_REQUIRE(aligned16(x_start) && aligned16(code_emb) && aligned16(noise), "diff_calc_bpd: 16-byte aligned buffers");
    const Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, "diff_calc_bpd runs on an integer-timestep schedule (dtts_diff_schedule)");
    DTTS_REQUIRE(use_x3(), "diff_calc_bpd runs the split-precision trunk (conv_x3 = 1): the exact fp32 convs choose their tile, and with it a "
                           "row's summation order, by the launch size");
    if (lens_host)
        for (int b = 0; b < B; ++b) DTTS_REQUIRE(lens_host[b] >= 1 && lens_host[b] <= T, "diff_calc_bpd: lens outside [1, T]");
    const int S = sc.n, C = cfg.diff_channels, n = cfg.mel_channels * T;
    const long long pairs = (long long)B * S;
    DTTS_REQUIRE(pairs < (1ll << 31), "diff_calc_bpd: B x steps too large");
    const int R = (int)std::min<long long>(pairs, rows_per_pass ? rows_per_pass : bpd_default_rows(T));
    const size_t row = (size_t)R * n, ncode = (size_t)C * T, npart = (size_t)R * diff_loss_blocks(n) * 3;
    const size_t nprior = (size_t)B * diff_loss_blocks(n);
    ws().ensure(rows_ws_bytes(R, C, T) + sizeof(float) * (4 * row + R * ncode + npart + nprior) + 16384);
    float* x_t = ws().f32(row);
    float* z = ws().f32(row);
    float* model_out = ws().f32(2 * row);
    float* code_rows = ws().f32(R * ncode);
    float* partials = ws().f32(npart);
    float* prior_part = ws().f32(nprior);
    const size_t mark = ws().mark();
    // the trunk's split-K and key-split rules go by the number of samples in a launch; pinned, a row's bits do not depend on its pass
    RowInvariantLaunches pin;
    std::vector<DiffBpdRow> rows(R);
    std::vector<int> steps(R), lens(R);
    for (long long p0 = 0; p0 < pairs; p0 += R) {
        const int Rp = (int)std::min<long long>(R, pairs - p0);
        for (int r = 0; r < Rp; ++r) {
            const long long p = p0 + r;
            const int t = S - 1 - (int)(p / B), b = (int)(p % B);
            rows[r] = bpd_row(sc, t, b, sample_ids_host ? sample_ids_host[b] : 0, b * S + (S - 1 - t));
            steps[r] = t;
            lens[r] = lens_host ? lens_host[b] : T;
        }
        const DiffBpdRow* rd =
            reinterpret_cast<const DiffBpdRow*>(upload_ints(reinterpret_cast<const int*>(rows.data()), Rp * DIFF_BPD_ROW_WORDS, s));
        launch_diff_bpd_q_sample(x_start, rd, noise, seed, B, Rp, n, x_t, z, code_emb, code_rows, (long long)ncode, s);
        ws().rewind(mark);
        diff_forward_rows_s(sc, x_t, code_rows, lens.data(), Rp, T, steps.data(), model_out, s);
        launch_diff_bpd_terms(model_out, x_start, 0, x_t, z, rd, Rp, n, partials, vb, xstart_mse, mse, 1, nullptr, s);
    }
    launch_diff_prior_bpd(x_start, sc.sqrt_ac[S - 1], sc.log_1m_ac[S - 1], B, n, prior_part, prior, s);
    launch_diff_bpd_total(vb, prior, B, S, total, s);
}

}  // namespace dtts
