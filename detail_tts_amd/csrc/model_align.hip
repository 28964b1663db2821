// Text-to-audio alignment from the GPT's attention: the teacher-forced pass (model_gpt.hip, gpt_teacher_forced) with the read-out of
// attn_probs.hip hooked behind the qkv conv of the selected layers, and the unit entries of the two kernels.  Reference: the maps are
// those of get_logits(..., get_attns=True) (gpt/model.py:392-400: GPT2Model(output_attentions=True).attentions, one [B, H, L, L] per layer).
#include <algorithm>
#include <cmath>

#include "model.h"

namespace dtts {

static void check_layers(const char* who, const int* layers_host, int n_layers, int gpt_layers) {
    const std::string w(who);
    DTTS_REQUIRE(layers_host && n_layers >= 1 && n_layers <= gpt_layers, (w + ": layers (1 .. gpt_layers entries)").c_str());
    for (int k = 0; k < n_layers; ++k) {
        DTTS_REQUIRE(layers_host[k] >= 0 && layers_host[k] < gpt_layers, (w + ": layer outside [0, gpt_layers)").c_str());
        for (int q = 0; q < k; ++q) DTTS_REQUIRE(layers_host[q] != layers_host[k], (w + ": a layer is listed twice").c_str());
    }
}

// Every selected layer's per-head maps of the teacher-forced pass over [cond | 255, text, 0 | 8192, codes, 8193]:
// out DEVICE [n_layers][B][H][L_out][L_out], zeroed by the caller; row b fills its own top-left lt_b x lt_b, lt_b = 1 + (text_b + 2) +
// (codes_b + 2), L_out >= max lt_b.
void Model::gpt_attentions(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host, int Lt_max,
                           const int* codes_host, const int* ncodes_host, int n_max, int B, const int* layers_host, int n_layers, float* out,
                           int L_out, hipStream_t s, const float* cond_in) {
    DTTS_REQUIRE(bound_ && has_gpt_, "gpt weights not bound");
    DTTS_REQUIRE(B >= 1 && Lt_max >= 0 && n_max >= 0 && out && L_out >= 1, "gpt_attentions: B, Lt_max, n_max, out");
    DTTS_REQUIRE(text_host && (codes_host || n_max == 0), "gpt_attentions: null argument");
    DTTS_REQUIRE(cfg.gpt_dim == 48 * cfg.gpt_heads, "gpt_attentions: head dim 48 is the only instantiation of the probabilities kernel");
    check_layers("gpt_attentions", layers_host, n_layers, cfg.gpt_layers);
    for (int b = 0; b < B; ++b) {       // (the pass checks every length again, with the ids; here for the output's size alone)
        const int tlb = text_lens_host ? text_lens_host[b] : Lt_max, nb = ncodes_host ? ncodes_host[b] : n_max;
        DTTS_REQUIRE(tlb >= 0 && tlb <= Lt_max && nb >= 0 && nb <= n_max, "gpt_attentions: lengths");
        DTTS_REQUIRE(1 + tlb + 2 + nb + 2 <= L_out, "gpt_attentions: a row is longer than the output's L");
    }
    GptAttnRequest rq;
    rq.mode = ATTN_PROBS_HEADS;
    rq.layers = layers_host;
    rq.n_layers = n_layers;
    rq.out = out;
    rq.nq_max = rq.nk_max = L_out;
    gpt_teacher_forced(refer, refer_lens_host, Tr, text_host, text_lens_host, Lt_max, codes_host, ncodes_host, n_max, B, 0, s, cond_in, &rq);
}

// attn[b][j][i] = sum over (selected layer, head) of w[layer][head] * P(column predicting code j -> text column 1 + i), text_mass its row sum.
// attn DEVICE [B][n_max][Lt_max + 2], text_mass DEVICE [B][n_max], both zeroed by the caller; head_weights HOST [n_layers][H] or null
// (uniform 1 / (n_layers H)).
void Model::gpt_text_alignment(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host,
                               int Lt_max, const int* codes_host, const int* ncodes_host, int n_max, int B, const int* layers_host,
                               int n_layers, const float* head_weights_host, float* attn_out, float* text_mass_out, hipStream_t s,
                               const float* cond_in) {
    DTTS_REQUIRE(bound_ && has_gpt_, "gpt weights not bound");
    DTTS_REQUIRE(B >= 1 && Lt_max >= 0 && n_max >= 1 && attn_out && text_mass_out, "gpt_text_alignment: B, Lt_max, n_max, outputs");
    DTTS_REQUIRE(text_host && codes_host, "gpt_text_alignment: null argument");
    DTTS_REQUIRE(cfg.gpt_dim == 48 * cfg.gpt_heads, "gpt_text_alignment: head dim 48 is the only instantiation of the probabilities kernel");
    check_layers("gpt_text_alignment", layers_host, n_layers, cfg.gpt_layers);
    const int H = cfg.gpt_heads;
    std::vector<float> w((size_t)n_layers * H, 1.f / (float)(n_layers * H));
    if (head_weights_host)
        for (size_t k = 0; k < w.size(); ++k) {
            DTTS_REQUIRE(std::isfinite(head_weights_host[k]), "gpt_text_alignment: head_weights must be finite");
            w[k] = head_weights_host[k];
        }
    GptAttnRequest rq;
    rq.mode = ATTN_PROBS_MEAN;
    rq.layers = layers_host;
    rq.n_layers = n_layers;
    rq.w = w.data();             // host: the pass uploads them next to the windows, after it has range-checked the ids and codes
    rq.out = attn_out;
    rq.nq_max = n_max;
    rq.nk_max = Lt_max + 2;
    // (a batch whose longest text is shorter than Lt_max would give tl_max < Lt_max + 2: the pass requires equality, so say it here)
    int lt_seen = 0;
    for (int b = 0; b < B; ++b) lt_seen = std::max(lt_seen, text_lens_host ? text_lens_host[b] : Lt_max);
    DTTS_REQUIRE(lt_seen == Lt_max, "gpt_text_alignment: Lt_max has to be the longest row's text length");
    const GptForced f = gpt_teacher_forced(refer, refer_lens_host, Tr, text_host, text_lens_host, Lt_max, codes_host, ncodes_host, n_max, B, 0, s,
                                           cond_in, &rq);
    std::vector<int> nn(B);
    for (int b = 0; b < B; ++b) nn[b] = f.ml[b] - 2;
    launch_window_row_sums(attn_out, upload_ints(nn.data(), B, s), upload_ints(f.tl.data(), B, s), B, n_max, Lt_max + 2, text_mass_out, s);
}

// ONE launch of attn_probs_kernel on the caller's fp32 rows (tests/test_gpu_attn_probs.py).  qkv DEVICE [B][rows][cs]; lens and the four
// window arrays HOST; out DEVICE [B][H][nq_max][nk_max] (HEADS) or [B][nq_max][nk_max] (MEAN, w HOST [H]).  Everything is checked
// before the first launch or upload.
void Model::op_attn_probs(const float* qkv, const int* lens_host, int B, int rows, int cs, int T, int H, int D, int q_off, int k_off,
                          int head_stride, float scale, const int* q0_host, const int* nq_host, const int* k0_host, const int* nk_host, int nq_max,
                          int nk_max, int mode, const float* w_host, int first, float* out, hipStream_t s) {
    DTTS_REQUIRE(qkv && out && q0_host && nq_host && k0_host && nk_host, "op_attn_probs: null argument");
    DTTS_REQUIRE(D == 48, "op_attn_probs: head dim 48 (the GPT) is the only instantiation");
    DTTS_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= (1 << 16) && H > 0 && H <= 64 && rows > 0 && rows <= (1 << 16), "op_attn_probs: sizes");
    DTTS_REQUIRE(cs >= T && cs <= (1 << 17), "op_attn_probs: the row stride must be at least T");
    DTTS_REQUIRE(head_stride >= 0 && head_stride <= rows, "op_attn_probs: head stride");
    const int offs[2] = {q_off, k_off};
    for (int off : offs)
        DTTS_REQUIRE(off >= 0 && (long long)off + (long long)(H - 1) * head_stride + D <= rows, "op_attn_probs: q / k rows leave the tensor");
    DTTS_REQUIRE(mode == ATTN_PROBS_HEADS || mode == ATTN_PROBS_MEAN, "op_attn_probs: mode is 0 (heads) or 1 (mean)");
    DTTS_REQUIRE(first == 0 || first == 1, "op_attn_probs: first is 0 or 1");
    DTTS_REQUIRE(nq_max >= 1 && nk_max >= 1 && nq_max <= T && nk_max <= T, "op_attn_probs: nq_max, nk_max in [1, T]");
    DTTS_REQUIRE(std::isfinite(scale), "op_attn_probs: scale");
    std::vector<int> l(B);
    for (int b = 0; b < B; ++b) {
        l[b] = lens_host ? lens_host[b] : T;
        DTTS_REQUIRE(l[b] >= 0 && l[b] <= T, "op_attn_probs: lengths must lie in [0, T]");
        DTTS_REQUIRE(q0_host[b] >= 0 && nq_host[b] >= 0 && nq_host[b] <= nq_max && q0_host[b] + nq_host[b] <= T, "op_attn_probs: query window");
        DTTS_REQUIRE(k0_host[b] >= 0 && nk_host[b] >= 0 && nk_host[b] <= nk_max && k0_host[b] + nk_host[b] <= T, "op_attn_probs: key window");
    }
    std::vector<float> w;
    if (mode == ATTN_PROBS_MEAN) {
        DTTS_REQUIRE(w_host, "op_attn_probs: the mean mode needs head weights");
        w.assign(w_host, w_host + H);
        for (float v : w) DTTS_REQUIRE(std::isfinite(v), "op_attn_probs: head weights must be finite");
    }
    // ---- nothing has been launched or uploaded up to here
    AttnProbsParams a;
    a.qkv = qkv;
    a.bs = (long long)rows * cs;
    a.cs = cs;
    a.q_off = q_off;
    a.k_off = k_off;
    a.head_stride = head_stride;
    a.lens = upload_ints(l.data(), B, s);
    a.q0 = upload_ints(q0_host, B, s);
    a.nq = upload_ints(nq_host, B, s);
    a.k0 = upload_ints(k0_host, B, s);
    a.nk = upload_ints(nk_host, B, s);
    a.B = B; a.H = H; a.D = D;
    a.nq_max = nq_max;
    a.nk_max = nk_max;
    a.scale = scale;
    a.mode = mode;
    a.out = out;
    if (mode == ATTN_PROBS_MEAN) a.w = reinterpret_cast<const float*>(upload_ints(reinterpret_cast<const int*>(w.data()), H, s));
    a.first = first;
    launch_attn_probs(a, s);
}

// The monotone path of align_path.hip on the caller's scores: score DEVICE [B][n_max][m_max], n / m HOST, path DEVICE int32 [B][n_max].
// The int16 back-pointers live in the call workspace.
void Model::op_monotone_path(const float* score, const int* n_host, const int* m_host, int B, int n_max, int m_max, int* path, hipStream_t s) {
    DTTS_REQUIRE(score && n_host && m_host && path, "op_monotone_path: null argument");
    DTTS_REQUIRE(B >= 1 && B <= 65535 && n_max >= 1 && m_max >= 1, "op_monotone_path: B, n_max, m_max");
    DTTS_REQUIRE(n_max <= cfg.gpt_max_mel_pos, "op_monotone_path: more codes than mel positions (gpt_max_mel_pos)");
    DTTS_REQUIRE(m_max <= cfg.gpt_max_text_pos + 1 && m_max <= ALIGN_PATH_MAX_M, "op_monotone_path: more text columns than gpt_max_text_pos + 1");
    for (int b = 0; b < B; ++b) {
        DTTS_REQUIRE(n_host[b] >= 0 && n_host[b] <= n_max && m_host[b] >= 0 && m_host[b] <= m_max, "op_monotone_path: n / m outside [0, max]");
        DTTS_REQUIRE(n_host[b] == 0 || m_host[b] >= 1, "op_monotone_path: a row with codes needs at least one text column");
    }
    // ---- nothing has been launched or uploaded up to here
    ws().ensure(sizeof(short) * (size_t)B * n_max * m_max + 4096);
    short* back = static_cast<short*>(ws().raw(sizeof(short) * (size_t)B * n_max * m_max));
    launch_monotone_path(score, upload_ints(n_host, B, s), upload_ints(m_host, B, s), B, n_max, m_max, back, path, s);
}

}  // namespace dtts
