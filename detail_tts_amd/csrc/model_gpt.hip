// Stage A orchestration: conditioning encoder, GPT-2 prefill, KV-cache decode loop with on-device sampling,
// teacher-forced latents.  Reference: gpt/model.py:107-185 (GPT2InferenceModel.forward), :429-491 (forward /
// return_latent), :514-545 (inference_speech_tortoise); HF GPT2Model block structure and
// GenerationMixin._sample.  KV cache uses mel position k for the k-th code.
#include <algorithm>
#include <cmath>

#include "gpt_kernels.h"
#include "model.h"
#include "prof.h"

namespace dtts {

__global__ void copy_columns_kernel(const float* src, long long s_bs, int s_cs, const int* col0, const int* ncols, int C, float* dst,
                                    long long d_bs, int d_cs) {
    const int c = blockIdx.y, b = blockIdx.z;
    const int n = ncols[b], c0 = col0[b];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x)
        dst[(long long)b * d_bs + (long long)c * d_cs + t] = src[(long long)b * s_bs + (long long)c * s_cs + c0 + t];
}

void Model::build_gpt(hipStream_t s) {
    const int C = cfg.gpt_dim;
    gpt_cond_ = mel_style_w("gpt.conditioning_encoder", cfg.mel_channels, C / 2, C);
    gpt_layers_.clear();
    for (int l = 0; l < cfg.gpt_layers; ++l) {
        GptLayerW w;
        const std::string p = "gpt.gpt.h." + std::to_string(l);
        w.ln1_g = W(p + ".ln_1.weight", C);
        w.ln1_b = W(p + ".ln_1.bias", C);
        w.ln2_g = W(p + ".ln_2.weight", C);
        w.ln2_b = W(p + ".ln_2.bias", C);
        w.attn = conv(p + ".attn.c_attn", C, 3 * C, 1);
        w.proj = conv(p + ".attn.c_proj", C, C, 1);
        w.fc = conv(p + ".mlp.c_fc", C, 4 * C, 1);
        w.fc2 = conv(p + ".mlp.c_proj", 4 * C, C, 1);
        gpt_layers_.push_back(w);
    }
    lnf_g_ = W("gpt.gpt.ln_f.weight", C);
    lnf_b_ = W("gpt.gpt.ln_f.bias", C);
    fin_g_ = W("gpt.final_norm.weight", C);
    fin_b_ = W("gpt.final_norm.bias", C);
    mel_head_ = conv("gpt.mel_head", C, cfg.gpt_mel_codes, 1);
    // text_head (gpt/model.py:318): bound only when the checkpoint carries it; nothing on the inference path reads it
    has_text_head_ = weights_.count("gpt.text_head.wp") != 0;
    text_head_ = has_text_head_ ? conv("gpt.text_head", C, cfg.gpt_text_tokens, 1) : PackedConv();
    text_emb_ = W("gpt.text_embedding.weight", (size_t)cfg.gpt_text_tokens * C);
    mel_emb_ = W("gpt.mel_embedding.weight", (size_t)cfg.gpt_mel_codes * C);
    text_pos_ = W("gpt.text_pos_embedding.emb.weight", (size_t)cfg.gpt_max_text_pos * C);
    mel_pos_ = W("gpt.mel_pos_embedding.emb.weight", (size_t)cfg.gpt_max_mel_pos * C);
    // LayerNorm-algebra vectors of the two GEMVs of every layer that sit behind a LayerNorm (gpt_kernels.h): the decode step applies
    // ln_1 / ln_2 as two scalars per row in the CONSUMER of c_attn / c_fc
    size_t tot = 0;
    for (auto& w : gpt_layers_) tot += 2 * ((size_t)w.attn.CoutP + w.fc.CoutP) + 256;
    gpt_persist_.ensure(sizeof(float) * tot + 4096);
    for (auto& w : gpt_layers_) {
        float* ca = gpt_persist_.f32(w.attn.CoutP);
        float* da = gpt_persist_.f32(w.attn.CoutP);
        float* cf = gpt_persist_.f32(w.fc.CoutP);
        float* df = gpt_persist_.f32(w.fc.CoutP);
        launch_ln_fold_vectors(w.attn.w, C, w.attn.CoutP, w.ln1_g, w.ln1_b, w.attn.b, ca, da, s);
        launch_ln_fold_vectors(w.fc.w, C, w.fc.CoutP, w.ln2_g, w.ln2_b, w.fc.b, cf, df, s);
        w.attn_c = ca; w.attn_d = da; w.fc_c = cf; w.fc_d = df;
    }
    // the persistent token kernel's register-order weight copies (gpt_token.hip)
    tok_ok_ = gpt_token_supported(C, cfg.gpt_heads, gpt_layers_.empty() ? 0 : gpt_layers_[0].fc.Cout, (int)gpt_layers_.size(), cfg.gpt_mel_codes);
    for (auto& w : gpt_layers_) tok_ok_ = tok_ok_ && w.fc2.CoutP == C && w.fc.Cout == 4 * C;
    tok_ok_ = tok_ok_ && gpt_token_prepare();            // 128 co-resident workgroups + the opt-in LDS size on THIS device
    tok_failed_ = false;
    if (tok_ok_) {
        const size_t per_layer = gpt_token_pack_floats(0) + gpt_token_pack_floats(1) + gpt_token_pack_floats(2) + gpt_token_pack_floats(4);
        gpt_tokw_.ensure(sizeof(float) * (per_layer * gpt_layers_.size() + gpt_token_pack_floats(3) + GPT_TOKEN_VS) + 65536 +
                         sizeof(GptTokenLayer) * GPT_TOKEN_MAX_LAYERS);
        gpt_tokw_.reset();
        tokp_ = GptTokenParams();
        tokp_.NL = (int)gpt_layers_.size();
        tok_layers_.assign(gpt_layers_.size(), GptTokenLayer());
        for (size_t l = 0; l < gpt_layers_.size(); ++l) {
            const GptLayerW& w = gpt_layers_[l];
            GptTokenLayer& t = tok_layers_[l];
            float* q = gpt_tokw_.f32(gpt_token_pack_floats(0));
            float* pj = gpt_tokw_.f32(gpt_token_pack_floats(1));
            float* f = gpt_tokw_.f32(gpt_token_pack_floats(2));
            launch_gpt_token_pack(0, w.attn.w, 3 * C, w.attn.CoutP, q, s);
            launch_gpt_token_pack(1, w.proj.w, C, w.proj.CoutP, pj, s);
            launch_gpt_token_pack(2, w.fc.w, 4 * C, w.fc.CoutP, f, s);
            t.wq = reinterpret_cast<const float4*>(q);
            t.wp = reinterpret_cast<const float4*>(pj);
            t.wf = reinterpret_cast<const float4*>(f);
            t.w2 = w.fc2.w;
            float* f2 = gpt_tokw_.f32(gpt_token_pack_floats(4));
            launch_gpt_token_pack(4, w.fc2.w, w.fc2.Cout, w.fc2.CoutP, f2, s);
            t.w2p = reinterpret_cast<const float4*>(f2);
            t.bq = w.attn.b; t.bp = w.proj.b; t.bf = w.fc.b; t.b2 = w.fc2.b;
            t.g1 = w.ln1_g; t.be1 = w.ln1_b; t.g2 = w.ln2_g; t.be2 = w.ln2_b;
        }
        GptTokenLayer* dl = static_cast<GptTokenLayer*>(gpt_tokw_.raw(sizeof(GptTokenLayer) * tok_layers_.size()));
        DTTS_CHECK_HIP(hipMemcpyAsync(dl, tok_layers_.data(), sizeof(GptTokenLayer) * tok_layers_.size(), hipMemcpyHostToDevice, s));
        tokp_.L = dl;
        float* hw = gpt_tokw_.f32(gpt_token_pack_floats(3));
        float* hb = gpt_tokw_.f32(GPT_TOKEN_VS);
        launch_gpt_token_pack(3, mel_head_.w, cfg.gpt_mel_codes, mel_head_.CoutP, hw, s);
        DTTS_CHECK_HIP(hipMemsetAsync(hb, 0, sizeof(float) * GPT_TOKEN_VS, s));
        DTTS_CHECK_HIP(hipMemcpyAsync(hb, mel_head_.b, sizeof(float) * cfg.gpt_mel_codes, hipMemcpyDeviceToDevice, s));
        tokp_.wh = reinterpret_cast<const float4*>(hw);
        tokp_.bh = hb;
        tokp_.Vs = GPT_TOKEN_VS;
        tokp_.lnf_g = lnf_g_; tokp_.lnf_b = lnf_b_; tokp_.fin_g = fin_g_; tokp_.fin_b = fin_b_;
    }
    // gpt_score's partials for a full group (16 rows x every mel position): no allocation in its launch path
    gpt_score_ws_.ensure(sizeof(float) * gpt_score_part_floats(GEMV_MAXB, cfg.gpt_max_mel_pos, mel_head_.CoutP) + 4096);
    gpt_drop_graphs();      // captured graphs hold the old weight pointers
    gs_ = GptSession();
}

// sessions of <= 8 rows decode a token with ONE persistent kernel (DTTS_GPT_TOKEN_KERNEL=0: the launch-per-GEMV chain)
bool Model::gpt_use_token_kernel() const {
    static const bool on = env_on("DTTS_GPT_TOKEN_KERNEL");
    static const int env_rows = env_int("DTTS_GPT_TOKEN_ROWS", GPT_TOKEN_ROWS);
    return on && opt_gpt_token_ && tok_ok_ && !tok_failed_ && gs_.B <= std::min(env_rows, GPT_TOKEN_ROWS) && gs_.xch != nullptr;
}

// HF GPT-2 stack (without ln_f) over x [B, C, L] in place; optionally fills the KV cache.
void Model::gpt_prefill_layers(float* x, const int* lens, int B, int L, float* kv_cache, long long kv_layer_stride,
                               long long kv_bs, int kv_cs, hipStream_t s, const GptAttnCapture* capture) {
    const int C = cfg.gpt_dim, H = cfg.gpt_heads, D = C / H;
    const size_t act = (size_t)B * C * L;
    const size_t mark = ws().mark();
    float* h = ws().f32(act);
    float* qkv = ws().f32(3 * act);
    float* att = ws().f32(act);
    float* mlp = ws().f32(4 * act);
    const long long bs = (long long)C * L;
    for (size_t l = 0; l < gpt_layers_.size(); ++l) {
        const GptLayerW& w = gpt_layers_[l];
        launch_ln_channels(x, nullptr, bs, L, lens, L, B, C, w.ln1_g, w.ln1_b, 1e-5f, h, bs, L, s);
        ConvParams p = cp(h, C, qkv, 3 * C, B, L, L, lens);
        run_conv(w.attn, p, s);
        if (kv_cache) launch_kv_to_cache(qkv, 3 * bs, L, lens, L, B, C, kv_cache + l * kv_layer_stride, kv_bs, kv_cs, s);
        if (capture) gpt_capture_probs(*capture, (int)l, qkv, lens, B, L, s);
        AttnParams a;
        a.qkv = qkv;
        a.bs = 3 * bs;
        a.cs = L;
        a.q_off = 0;
        a.k_off = C;
        a.v_off = 2 * C;
        a.head_stride = D;
        a.out = att;
        a.o_bs = bs;
        a.o_cs = L;
        a.lens = lens;
        a.T = L;
        a.B = B;
        a.H = H;
        a.D = D;
        a.scale = 1.f / std::sqrt((float)D);
        a.causal = 1;
        launch_flash_attention(a, s);
        p = cp(att, C, x, C, B, L, L, lens);
        p.res = x;
        p.res_bs = bs;
        p.res_cs = L;
        run_conv(w.proj, p, s);
        launch_ln_channels(x, nullptr, bs, L, lens, L, B, C, w.ln2_g, w.ln2_b, 1e-5f, h, bs, L, s);
        p = cp(h, C, mlp, 4 * C, B, L, L, lens);
        p.epi_act = ACT_GELU_NEW;
        run_conv(w.fc, p, s);
        p = cp(mlp, 4 * C, x, C, B, L, L, lens);
        p.res = x;
        p.res_bs = bs;
        p.res_cs = L;
        run_conv(w.fc2, p, s);
    }
    ws().rewind(mark);
}

// The read-out of a selected layer's attention probabilities (attn_probs.hip) from the qkv rows the flash launch is about to consume.
// HEADS: slot k of the layer list gets its own [B][H][nq_max][nk_max]; MEAN: the layers accumulate into one buffer in list order.
void Model::gpt_capture_probs(const GptAttnCapture& c, int layer, const float* qkv, const int* lens, int B, int L, hipStream_t s) {
    const int C = cfg.gpt_dim, H = cfg.gpt_heads, D = C / H;
    for (int k = 0; k < c.req.n_layers; ++k) {
        if (c.req.layers[k] != layer) continue;
        AttnProbsParams a;
        a.qkv = qkv;
        a.bs = (long long)3 * C * L;
        a.cs = L;
        a.q_off = 0;
        a.k_off = C;
        a.head_stride = D;
        a.lens = lens;
        a.q0 = c.q0; a.nq = c.nq; a.k0 = c.k0; a.nk = c.nk;
        a.B = B; a.H = H; a.D = D;
        a.nq_max = c.req.nq_max;
        a.nk_max = c.req.nk_max;
        a.scale = 1.f / std::sqrt((float)D);
        a.mode = c.req.mode;
        if (c.req.mode == ATTN_PROBS_HEADS) {
            a.out = c.req.out + (size_t)k * B * H * a.nq_max * a.nk_max;
        } else {
            a.out = c.req.out;
            a.w = c.w + (size_t)k * H;
            a.first = k == 0;
        }
        launch_attn_probs(a, s);
    }
}

static size_t prefill_ws(int B, int C, int L) { return sizeof(float) * (size_t)9 * B * C * L + 16 * 256; }

// text [B][Lt_max] as api.py passes it (trailing 0 included) -> ids [255, text..., 0]  (gpt/model.py:517-518)
// Ids index device embedding tables: they are range-checked here, on the host where they live (nn.Embedding raises on these).
static void text_prefix_ids(const int* text, const int* text_lens, int B, int Lt_max, int n_text_tokens, std::vector<int>& ids,
                            std::vector<int>& tl, int& tl_max) {
    DTTS_REQUIRE(text && B >= 1 && Lt_max >= 0, "text ids");
    tl.resize(B);
    tl_max = 0;
    for (int b = 0; b < B; ++b) {
        const int n = text_lens ? text_lens[b] : Lt_max;
        DTTS_REQUIRE(n >= 0 && n <= Lt_max, "text length outside [0, Lt_max]");
        for (int j = 0; j < n; ++j) {
            const int id = text[(size_t)b * Lt_max + j];
            DTTS_REQUIRE(id >= 0 && id < n_text_tokens, "text id outside the text_embedding table");
        }
        tl[b] = n + 2;
        tl_max = std::max(tl_max, tl[b]);
    }
    ids.assign((size_t)B * tl_max, 0);
    for (int b = 0; b < B; ++b) {
        int* r = ids.data() + (size_t)b * tl_max;
        r[0] = 255;
        for (int j = 0; j < tl[b] - 2; ++j) r[1 + j] = text[(size_t)b * Lt_max + j];
        r[tl[b] - 1] = 0;
    }
}

// The mel stream a session's prefill embeds behind the text (gpt/model.py:528-530 and :561-564 with :132-136), per row:
//   no prompt : [8192]                          n_p = 1
//   prompt    : [1, 8192, c_1 .. c_m]           n_p = m + 2: inference_speech_valle's fake_inputs hold 1 + (Lt + 3) + (m + 1) ids - the
//               first value of build_aligned_inputs_and_targets is [8192, codes], the stop token belongs to its unused targets - and
//               the cached embedding covers Lt + 3 columns, so ONE fill id 1 is embedded with mel_embedding at mel position 0
//   raw       : [8192, c_1 .. c_m]              n_p = m + 1 (option gpt_prompt_raw, tests: a tortoise session after m forced steps)
// mel[b][0 .. np[b]) with row stride np_max; seen[b] = [1, mel[b]...] (row stride np_max + 1): HF's repetition penalty sees every id of
// input_ids, the fill id 1 of the prefix columns included.  Codes are range-checked here, on the host where they live.
static void prompt_prefix_ids(const dtts_gpt_options& o, int B, int G, int max_mel_pos, bool raw, std::vector<int>& np, int& np_max,
                              std::vector<int>& mel, std::vector<int>& seen, std::vector<int>& nseen) {
    np.assign(B, 1);
    np_max = 1;
    DTTS_REQUIRE(o.prompt_codes || !o.prompt_lens, "prompt_lens without prompt_codes");
    if (o.prompt_codes) {
        DTTS_REQUIRE(o.prompt_lens && o.prompt_stride >= 0, "prompt_codes needs prompt_lens and prompt_stride");
        for (int b = 0; b < B; ++b) {
            const int m = o.prompt_lens[b];
            DTTS_REQUIRE(m >= 0 && m <= o.prompt_stride, "prompt_lens outside [0, prompt_stride]");
            // (the sampler reads position row n_p + G - 1 for the input of a token that is never fed: m + 2 + G rows are touched; the
            // limit keeps one more row spare)
            DTTS_REQUIRE((long long)m + 3 + G <= max_mel_pos, "prompt_lens: m + 3 + max_generate_length exceeds the mel position table (gpt_max_mel_pos)");
            for (int k = 0; k < m; ++k) {
                const int c = o.prompt_codes[(size_t)b * o.prompt_stride + k];
                DTTS_REQUIRE(c >= 0 && c < 8192, "prompt_codes: code outside [0, 8192)");
            }
            np[b] = raw ? m + 1 : m + 2;
            np_max = std::max(np_max, np[b]);
        }
    }
    mel.assign((size_t)B * np_max, 0);
    seen.assign((size_t)B * (np_max + 1), 0);
    nseen.assign(B, 0);
    for (int b = 0; b < B; ++b) {
        int* r = mel.data() + (size_t)b * np_max;
        int n = 0;
        if (o.prompt_codes) {
            const int m = o.prompt_lens[b];
            if (!raw) r[n++] = 1;
            r[n++] = 8192;
            for (int k = 0; k < m; ++k) r[n++] = o.prompt_codes[(size_t)b * o.prompt_stride + k];
        } else {
            r[n++] = 8192;
        }
        int* q = seen.data() + (size_t)b * (np_max + 1);
        q[0] = 1;
        std::copy(r, r + n, q + 1);
        nseen[b] = n + 1;
    }
}

// ---- HF's remaining logits processors: what the host prepares for the sampler's control block -----------------------------------
// [V] bit 0 = suppress_tokens, bit 1 = begin_suppress_tokens (ids were range-checked by check_gpt_options against 8194; here against V)
static std::vector<unsigned char> processor_token_mask(const dtts_gpt_options& o, int V) {
    std::vector<unsigned char> m(V, 0);
    for (int i = 0; i < o.n_suppress_tokens; ++i) {
        DTTS_REQUIRE(o.suppress_tokens[i] >= 0 && o.suppress_tokens[i] < V, "suppress_tokens: id outside [0, V)");
        m[o.suppress_tokens[i]] |= 1;
    }
    for (int i = 0; i < o.n_begin_suppress_tokens; ++i) {
        DTTS_REQUIRE(o.begin_suppress_tokens[i] >= 0 && o.begin_suppress_tokens[i] < V, "begin_suppress_tokens: id outside [0, V)");
        m[o.begin_suppress_tokens[i]] |= 2;
    }
    return m;
}
// ExponentialDecayLengthPenalty's multipliers: t[i] = float(pow(factor, i) - 1), the power and the difference in double as Python
// evaluates them (float.__pow__ is the C library's pow), rounded once to the float32 torch multiplies |score| by.  Saturated at
// DECAY_MUL_MAX: far behind `start` HF's multiplier leaves float32 (inf: |score| * inf, then inf - inf = NaN in its softmax) or Python's
// pow raises OverflowError; here the stop score stays finite and so large that the stop token is the only one left - what the
// penalty is for.  No factor is refused for the length of the call.
constexpr double DECAY_MUL_MAX = 1e30;
void gpt_decay_multipliers(double factor, int n, float* out) {
    for (int i = 0; i < n; ++i) {
        const double m = i == 0 ? 0.0 : std::pow(factor, (double)i) - 1.0;
        out[i] = (float)(m < DECAY_MUL_MAX ? m : DECAY_MUL_MAX);
    }
}
// MinLength and MinNewTokensLength folded: the first decode step at which the stop token may be drawn.  At step j HF sees
// input_len + j ids, j - forced_prefix of them behind its prompt: the stop is -inf while input_len + j < min_length or
// j - forced_prefix < min_new_tokens.  (forced_prefix < 0: the unit entry's rows, which are already some tokens behind the prompt.)
int gpt_first_stop_step(int input_len, int forced_prefix, int min_length, int min_new_tokens) {
    return std::max(0, std::max(min_length - input_len, min_new_tokens > 0 ? forced_prefix + min_new_tokens : 0));
}
static bool processors_mask_on(const dtts_gpt_options& o) { return o.n_suppress_tokens > 0 || o.n_begin_suppress_tokens > 0; }

// ---- per-row sampling settings: ONE way into the control block.  Row b's settings are its own record (dtts_gpt_options.row_options) or
// the session's scalar fields; a uniform session writes its one value into every slot and the sampler reads slot blockIdx.x either way.
static dtts_gpt_row_options gpt_row_settings(const dtts_gpt_options& o, int b) {
    if (o.row_options) return o.row_options[b];
    dtts_gpt_row_options r{};
    r.temperature = o.temperature; r.top_p = o.top_p; r.repetition_penalty = o.repetition_penalty; r.typical_mass = o.typical_mass;
    r.min_p = o.min_p; r.epsilon_cutoff = o.epsilon_cutoff; r.top_k = o.top_k; r.max_generate_length = o.max_generate_length;
    r.no_repeat_ngram_size = o.no_repeat_ngram_size; r.min_length = o.min_length; r.min_new_tokens = o.min_new_tokens;
    r.exp_decay_start = o.exp_decay_start; r.exp_decay_factor = o.exp_decay_factor;
    r.suppress_tokens = o.suppress_tokens; r.n_suppress_tokens = o.n_suppress_tokens;
    r.begin_suppress_tokens = o.begin_suppress_tokens; r.n_begin_suppress_tokens = o.n_begin_suppress_tokens;
    return r;
}
static dtts_gpt_options gpt_row_as_options(const dtts_gpt_options& o, const dtts_gpt_row_options& r) {
    dtts_gpt_options t = o;
    t.suppress_tokens = r.suppress_tokens; t.n_suppress_tokens = r.n_suppress_tokens;
    t.begin_suppress_tokens = r.begin_suppress_tokens; t.n_begin_suppress_tokens = r.n_begin_suppress_tokens;
    return t;
}
// What the host hands the sampler besides the scalars: the token masks ([V] for a uniform session, [B][V] under row_options) and ONE
// decay table in which rows of the same factor share a slice of decay_n entries.  Fills the control block's slots of rows 0 .. B-1
// (max_steps = G is the caller's); the caller uploads the two tables and points tok_mask / decay_mul at them when they are not empty.
struct GptRowTables {
    std::vector<unsigned char> mask;
    std::vector<float> decay;
    int ngram_max = 0;
};
static GptRowTables gpt_ctl_rows(GptCtl& c, const dtts_gpt_options& o, int B, int V, int G, int decay_n) {
    GptRowTables t;
    std::vector<double> factors;
    bool any_mask = false;
    for (int b = 0; b < B; ++b) {
        const dtts_gpt_row_options r = gpt_row_settings(o, b);
        DTTS_REQUIRE(r.no_repeat_ngram_size >= 0 && r.no_repeat_ngram_size <= SAMP_NGRAM_MAX, "no_repeat_ngram_size outside 0 .. 16");
        c.repetition_penalty[b] = r.repetition_penalty;
        c.temperature[b] = r.temperature;
        c.top_p[b] = r.top_p;
        c.top_k[b] = r.top_k;
        c.typical_mass[b] = r.typical_mass;
        c.row_max_steps[b] = o.row_options ? std::min(std::max(r.max_generate_length, 1), G) : G;
        c.ngram[b] = r.no_repeat_ngram_size;
        c.min_p[b] = r.min_p;
        c.eps_cutoff[b] = r.epsilon_cutoff;
        t.ngram_max = std::max(t.ngram_max, r.no_repeat_ngram_size);
        any_mask = any_mask || r.n_suppress_tokens > 0 || r.n_begin_suppress_tokens > 0;
        c.decay_tab[b] = 0;
        c.decay_n[b] = 0;
        if (r.exp_decay_factor > 0.0) {
            size_t k = 0;
            while (k < factors.size() && factors[k] != r.exp_decay_factor) ++k;
            if (k == factors.size()) {
                factors.push_back(r.exp_decay_factor);
                t.decay.resize((k + 1) * (size_t)decay_n);
                gpt_decay_multipliers(r.exp_decay_factor, decay_n, t.decay.data() + k * (size_t)decay_n);
            }
            c.decay_tab[b] = (int)k * decay_n;
            c.decay_n[b] = decay_n;
        }
    }
    c.mask_stride = 0;
    if (any_mask) {
        if (!o.row_options) t.mask = processor_token_mask(o, V);
        else {
            c.mask_stride = V;
            t.mask.reserve((size_t)B * V);
            for (int b = 0; b < B; ++b) {
                const std::vector<unsigned char> m = processor_token_mask(gpt_row_as_options(o, o.row_options[b]), V);
                t.mask.insert(t.mask.end(), m.begin(), m.end());
            }
        }
    }
    return t;
}

// ---- decode session ------------------------------------------------------------------------------------------------------------
// dtts_gpt_prefill: conditioning encoder + [cond | text | start_mel] prefill (KV cache filled) + the first sampled token; with
// dtts_gpt_options.prompt_codes the prefix is [cond | text | 1, 8192, prompt] (inference_speech_valle, gpt/model.py:546-579): the
// whole prompt runs through the parallel prefill, no prompt token takes a decode step, and the KV cache, the repetition-penalty history
// and the mel position counter start behind it.  The latents written while decoding are then the hidden states WITH THE PROMPT IN
// CONTEXT - not what forward(return_latent=True) on the generated codes alone returns (gpt_teacher_forced computes those).  The session
// (KV cache, residual rows, sampler state, device control block) lives in the handle's own arena, whose addresses stay fixed from call
// to call, so the captured decode graphs stay valid.
void Model::gpt_prefill(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host,
                        int Lt_max, int B, const dtts_gpt_options& o, float* latents_cm, int lat_stride, hipStream_t s,
                        const float* cond_in) {
    DTTS_REQUIRE(bound_ && has_gpt_, "gpt weights not bound");
    DTTS_REQUIRE(cond_in || (refer && Tr >= 1), "gpt_prefill: neither a prompt mel nor its conditioning latent");
    if (cond_in) Tr = 0;                             // (sizes the encoder's scratch below: none)
    DTTS_REQUIRE(B >= 1 && B <= GEMV_MAXB, "a GPT decode session holds 1..16 sequences (dtts_gpt_generate groups larger batches)");
    DTTS_REQUIRE(o.max_generate_length >= 1 && o.max_generate_length + 1 <= cfg.gpt_max_mel_pos, "max_generate_length");
    DTTS_REQUIRE(!latents_cm || lat_stride >= o.max_generate_length, "latent buffer too small");
    DTTS_REQUIRE(o.sample_ids, "sample_ids");
    const int beamK = o.num_beams > 1 ? o.num_beams : 0;
    if (beamK) {
        DTTS_REQUIRE(beamK <= BEAM_MAXK && B % beamK == 0, "a beam session's rows are whole utterances: B has to be a multiple of num_beams");
        DTTS_REQUIRE(!o.forced_codes && !o.forced_uniforms, "num_beams with forced_codes / forced_uniforms");
        DTTS_REQUIRE(cfg.gpt_mel_codes <= BEAM_V_MAX, "num_beams: vocabulary too large for the beam step");
        latents_cm = nullptr;                        // rows change lineage: no decode-time latents (dtts_gpt_latents on the chosen codes)
    }
    if (!replaying_) {                               // keep the call's inputs: a timed-out token kernel is replayed on the chain (gpt_finish)
        GptReplay& r = replay_;
        r.valid = false;
        if (tok_ok_ && !tok_failed_ && B <= GPT_TOKEN_ROWS) {
            const size_t nref = cond_in ? (size_t)B * cfg.gpt_dim : (size_t)B * cfg.mel_channels * Tr;
            gpt_replay_.ensure(sizeof(float) * nref + 256);
            DTTS_CHECK_HIP(hipMemcpyAsync(gpt_replay_.f32(nref), cond_in ? cond_in : refer, sizeof(float) * nref, hipMemcpyDeviceToDevice, s));
            r.has_cond = cond_in != nullptr;
            r.Tr = Tr; r.Lt_max = Lt_max; r.B = B; r.lat_stride = lat_stride; r.latents_cm = latents_cm;
            r.has_refer_lens = refer_lens_host != nullptr;
            r.has_text_lens = text_lens_host != nullptr;
            r.refer_lens.clear(); r.text_lens.clear(); r.forced_codes.clear(); r.row_seeds.clear();      // nothing of an earlier session survives
            r.prompt_codes.clear(); r.prompt_lens.clear(); r.suppress.clear(); r.begin_suppress.clear();
            r.rows.clear(); r.row_ids.clear();
            if (o.row_options) {                     // the rows' settings and their id lists are the session's: kept with it
                r.rows.assign(o.row_options, o.row_options + B);
                r.row_ids.resize((size_t)2 * B);
                for (int b = 0; b < B; ++b) {
                    const dtts_gpt_row_options& q = o.row_options[b];
                    if (q.n_suppress_tokens > 0) r.row_ids[2 * b].assign(q.suppress_tokens, q.suppress_tokens + q.n_suppress_tokens);
                    if (q.n_begin_suppress_tokens > 0) r.row_ids[2 * b + 1].assign(q.begin_suppress_tokens, q.begin_suppress_tokens + q.n_begin_suppress_tokens);
                }
            }
            if (o.n_suppress_tokens > 0) r.suppress.assign(o.suppress_tokens, o.suppress_tokens + o.n_suppress_tokens);
            if (o.n_begin_suppress_tokens > 0) r.begin_suppress.assign(o.begin_suppress_tokens, o.begin_suppress_tokens + o.n_begin_suppress_tokens);
            if (refer_lens_host) r.refer_lens.assign(refer_lens_host, refer_lens_host + B);
            r.text.assign(text_host, text_host + (size_t)B * Lt_max);
            if (text_lens_host) r.text_lens.assign(text_lens_host, text_lens_host + B);
            r.sample_ids.assign(o.sample_ids, o.sample_ids + B);
            r.o = o;
            if (o.forced_codes) r.forced_codes.assign(o.forced_codes, o.forced_codes + (size_t)B * o.max_generate_length);
            if (o.row_seeds) r.row_seeds.assign(o.row_seeds, o.row_seeds + B);
            if (o.prompt_codes && o.prompt_lens && o.prompt_stride >= 0) {
                r.prompt_codes.assign(o.prompt_codes, o.prompt_codes + (size_t)B * o.prompt_stride);
                r.prompt_lens.assign(o.prompt_lens, o.prompt_lens + B);
                if (r.prompt_codes.empty()) r.prompt_codes.push_back(0);      // (stride 0: the replayed options still need a pointer)
            }
            r.valid = true;
        }
    }
    ArenaUse use_stage_a_arena(ws_gpt_);             // decode steps use only gpt_state_; the prefill's scratch is stage A's own
    const int C = cfg.gpt_dim, V = cfg.gpt_mel_codes, G = o.max_generate_length;
    const int NL = (int)gpt_layers_.size();
    std::vector<int> ids, tl;
    int tl_max;
    text_prefix_ids(text_host, text_lens_host, B, Lt_max, cfg.gpt_text_tokens, ids, tl, tl_max);
    DTTS_REQUIRE(tl_max <= cfg.gpt_max_text_pos, "text too long");
    std::vector<int> lp(B), ml, mel0, seen0, nseen;
    int Lp = 0, np_max;
    prompt_prefix_ids(o, B, G, cfg.gpt_max_mel_pos, opt_prompt_raw_, ml, np_max, mel0, seen0, nseen);
    for (int b = 0; b < B; ++b) {
        lp[b] = 1 + tl[b] + ml[b];
        Lp = std::max(Lp, lp[b]);
    }
    if (o.forced_codes)
        for (size_t i = 0; i < (size_t)B * G; ++i)
            DTTS_REQUIRE(o.forced_codes[i] >= -1 && o.forced_codes[i] < V, "forced code outside the mel_embedding table (-1 = sample at this step)");
    // ---- session storage.  The KV capacity is rounded up so that sessions of similar lengths share one arena layout (and graph).
    const int cap = round_up(Lp + G, 128);
    const long long kv_bs = (long long)2 * C * cap, kv_layer = kv_bs * B;
    const size_t need = sizeof(float) * ((size_t)NL * kv_layer + (size_t)B * (4 * C + cfg.gpt_heads * 8 * ATT_REC) + (size_t)2 * B * GEMV_PART_FLOATS + 2 * 64 * GEMV_MAXB * 2) +
                        (size_t)B * V + sizeof(int) * ((size_t)2 * B * G + 64) + sizeof(GptCtl) + 64 * 256 +
                        sizeof(int) * (size_t)B * cap + (size_t)B * V + sizeof(float) * (size_t)B * ((size_t)G + 1) + 4 * 256 +
                        sizeof(int) * ((size_t)2 * B * G + 8 * GEMV_MAXB) + sizeof(float) * ((size_t)G + 1 + 2 * GEMV_MAXB) + 16 * 256 +
                        (tok_ok_ && B <= GPT_TOKEN_ROWS ? sizeof(unsigned long long) * GPT_TOKEN_XCH_WORDS + sizeof(float) * GPT_TOKEN_ROWS * GPT_TOKEN_VS + 1024 : 0);
    if (need > gpt_state_.capacity() || gs_.B != B || gs_.cap != cap || gs_.G != G) {
        gpt_drop_graphs();
        gpt_state_.ensure(need);
        gpt_state_.reset();
        GptSession n;
        n.B = B; n.cap = cap; n.G = G;
        n.kv = gpt_state_.f32((size_t)NL * kv_layer);
        n.x = gpt_state_.f32((size_t)B * C);
        n.y = gpt_state_.f32((size_t)B * C);
        n.ab = gpt_state_.f32((size_t)B * cfg.gpt_heads * 8 * ATT_REC);
        n.lat = gpt_state_.f32((size_t)B * C);
        n.xa = gpt_state_.f32((size_t)B * C);
        n.part = gpt_state_.f32((size_t)B * GEMV_PART_FLOATS);
        n.part2 = gpt_state_.f32((size_t)B * GEMV_PART_FLOATS);
        n.st1 = gpt_state_.f32((size_t)64 * GEMV_MAXB * 2);
        n.st2 = gpt_state_.f32((size_t)64 * GEMV_MAXB * 2);
        n.seen = static_cast<unsigned char*>(gpt_state_.raw((size_t)B * V));
        n.finished = gpt_state_.i32(B);
        n.codes = gpt_state_.i32((size_t)B * G);
        n.forced = gpt_state_.i32((size_t)B * G);
        n.hist = gpt_state_.i32((size_t)B * cap);
        n.tok_mask = static_cast<unsigned char*>(gpt_state_.raw((size_t)B * V));      // a mask and a decay slice per row at the most
        n.decay_mul = gpt_state_.f32((size_t)B * ((size_t)G + 1));
        n.ctl = static_cast<GptCtl*>(gpt_state_.raw(sizeof(GptCtl)));
        if (tok_ok_ && B <= GPT_TOKEN_ROWS) {
            n.xch = static_cast<unsigned long long*>(gpt_state_.raw(sizeof(unsigned long long) * GPT_TOKEN_XCH_WORDS));
            n.logits = gpt_state_.f32((size_t)GPT_TOKEN_ROWS * GPT_TOKEN_VS);
            n.tok_err = gpt_state_.i32(2);
            n.tok_epoch = reinterpret_cast<unsigned*>(n.tok_err + 1);
            // tags of a previous layout of this arena must not survive: all words 0 (no valid tag is 0), the launch counter restarts at 1
            DTTS_CHECK_HIP(hipMemsetAsync(n.xch, 0, sizeof(unsigned long long) * GPT_TOKEN_XCH_WORDS, s));
            const int init[2] = {0, 1};
            DTTS_CHECK_HIP(hipMemcpyAsync(n.tok_err, init, sizeof(init), hipMemcpyHostToDevice, s));
            DTTS_CHECK_HIP(hipStreamSynchronize(s));
        }
        // the beam state comes LAST: every buffer the sampled decode uses keeps the offset it had without it
        n.b_run_seq = gpt_state_.i32((size_t)B * G);
        n.b_fin_seq = gpt_state_.i32((size_t)B * G);
        n.b_fin_flag = gpt_state_.i32(GEMV_MAXB); n.b_fin_len = gpt_state_.i32(GEMV_MAXB); n.b_unsat = gpt_state_.i32(GEMV_MAXB);
        n.b_done = gpt_state_.i32(GEMV_MAXB); n.b_parents = gpt_state_.i32(GEMV_MAXB); n.b_tokens = gpt_state_.i32(GEMV_MAXB);
        n.b_last_step = gpt_state_.i32(GEMV_MAXB); n.b_ident = gpt_state_.i32(GEMV_MAXB);
        n.b_run_score = gpt_state_.f32(GEMV_MAXB); n.b_fin_score = gpt_state_.f32(GEMV_MAXB);
        n.b_len_div = gpt_state_.f32((size_t)G + 1);
        gs_ = n;
    }
    if (gs_.beam_K != beamK) gpt_drop_graphs();      // (the captured steps hold the sampler or the beam kernels)
    gs_.beam_K = beamK;
    gs_.beam_lp = o.length_penalty;
    gs_.beam_es = o.early_stopping;
    gs_.kv_bs = kv_bs;
    gs_.kv_layer = kv_layer;
    gs_.steps = 0;
    gs_.active = false;
    // (the encoder's scratch sits ON TOP of emb: a 6-row beam group with a 64-frame prompt and a 10-column prefix overflowed the arena
    // while the two were sized side by side)
    ws().ensure(sizeof(float) * (size_t)B * C * Lp +
                std::max(prefill_ws(B, C, Lp), sizeof(float) * ((size_t)5 * B * (C / 2) * Tr + (size_t)B * C * Tr + (size_t)B * C)) + 65536);
    float* emb = ws().f32((size_t)B * C * Lp);
    const float* cond = cond_in;                     // UnifiedVoice.compute_embeddings' cond_latents (gpt/model.py:492-513)
    if (!cond_in) {
        float* enc = ws().f32((size_t)B * C);
        std::vector<int> rl(B);
        for (int b = 0; b < B; ++b) rl[b] = refer_lens_host ? refer_lens_host[b] : Tr;
        const int* d_rl = upload_ints(rl.data(), B, s);
        const size_t m = ws().mark();
        mel_style(gpt_cond_, refer, d_rl, rl.data(), B, Tr, enc, s);         // gpt/model.py:521-524
        ws().rewind(m);
        cond = enc;
    }
    const int* d_ids = upload_ints(ids.data(), B * tl_max, s);
    const int* d_tl = upload_ints(tl.data(), B, s);
    const int* d_ml = upload_ints(ml.data(), B, s);
    const int* d_mel0 = upload_ints(mel0.data(), B * np_max, s);
    const int* d_lp = upload_ints(lp.data(), B, s);
    const int* d_seen0 = upload_ints(seen0.data(), B * (np_max + 1), s);
    const int* d_nseen = upload_ints(nseen.data(), B, s);
    // control block (host copy kept in the handle: the asynchronous upload reads it)
    GptCtl& c = ctl_host_;
    std::memset(&c, 0, sizeof(c));
    for (int b = 0; b < B; ++b) { c.lp[b] = lp[b]; c.pos_off[b] = ml[b]; c.sample_id[b] = o.sample_ids[b]; c.seed[b] = o.row_seeds ? o.row_seeds[b] : o.seed; }
    {
        const int wgs = o.token_wgs ? o.token_wgs : opt_tok_wgs_;      // latched: a later set_option does not change a running session's kernel
        if (wgs != gs_.tok_wgs) gpt_drop_graphs();                      // (captured decode graphs hold the previous session's kernel choice)
        gs_.tok_wgs = wgs;
        static const int env_fuse = env_tri("DTTS_GPT_FUSE_PROJ");       // the env value wins when set, as the token kernel's switches do
        const bool fuse = env_fuse >= 0 ? env_fuse != 0 : opt_gpt_fuse_proj_;
        if (fuse != gs_.fuse_proj) gpt_drop_graphs();                   // (the captured chain holds K2 + K3 in one form or the other)
        gs_.fuse_proj = fuse;
    }
    c.suppress_eos = o.suppress_eos;
    c.max_steps = G;
    c.forced_u = o.forced_uniforms;
    c.u_stride = G;
    c.forced_tokens = o.forced_codes ? gs_.forced : nullptr;
    c.f_stride = G;
    c.latents = latents_cm;
    c.lat_bs = (long long)C * lat_stride;
    c.lat_cs = lat_stride;
    // ---- HF's remaining processors.  A row's input_ids at step j are fills + nn ids: fills = lp - nn fill ids (1) in front of the nn
    // ordered ids [8192, prompt codes] (the prompt's own leading 1 is a fill id), then j tokens.  HF's prompt ends behind the forced
    // prefix (input_tokens): k = the leading forced codes >= 0.
    std::vector<int> hist0;
    DTTS_REQUIRE(!o.row_options || !beamK, "row_options with num_beams > 1 (a beam session is uniform)");
    const GptRowTables tabs = gpt_ctl_rows(c, o, B, V, G, G + 1);
    {
        const int n = tabs.ngram_max;                  // (the history is kept when ANY row bans n-grams)
        c.hist = n > 0 ? gs_.hist : nullptr;
        c.hist_stride = cap;
        if (n > 0) hist0.assign((size_t)B * cap, 0);
        for (int b = 0; b < B; ++b) {
            const int lead = o.prompt_codes && !opt_prompt_raw_ ? 1 : 0, nn = ml[b] - lead;
            int k = 0;
            if (o.forced_codes)
                while (k < G && o.forced_codes[(size_t)b * G + k] >= 0) ++k;
            const dtts_gpt_row_options rw = gpt_row_settings(o, b);
            c.hist_n0[b] = nn;
            c.nfill[b] = std::min(c.ngram[b], lp[b] - nn);
            if (n > 0) std::copy(mel0.data() + (size_t)b * np_max + lead, mel0.data() + (size_t)b * np_max + ml[b], hist0.data() + (size_t)b * cap);
            c.stop_from[b] = gpt_first_stop_step(lp[b], k, rw.min_length, rw.min_new_tokens);
            c.decay_off[b] = k + rw.exp_decay_start;
            c.begin_step[b] = k;
        }
        if (!tabs.mask.empty()) {
            c.tok_mask = gs_.tok_mask;
            DTTS_CHECK_HIP(hipMemcpyAsync(gs_.tok_mask, tabs.mask.data(), tabs.mask.size(), hipMemcpyHostToDevice, s));
        }
        if (!tabs.decay.empty()) {
            c.decay_mul = gs_.decay_mul;
            DTTS_CHECK_HIP(hipMemcpyAsync(gs_.decay_mul, tabs.decay.data(), sizeof(float) * tabs.decay.size(), hipMemcpyHostToDevice, s));
        }
        if (n > 0) DTTS_CHECK_HIP(hipMemcpyAsync(gs_.hist, hist0.data(), sizeof(int) * hist0.size(), hipMemcpyHostToDevice, s));
    }
    DTTS_CHECK_HIP(hipMemcpyAsync(gs_.ctl, &c, sizeof(c), hipMemcpyHostToDevice, s));
    if (o.forced_codes) DTTS_CHECK_HIP(hipMemcpyAsync(gs_.forced, o.forced_codes, sizeof(int) * (size_t)B * G, hipMemcpyHostToDevice, s));
    // seen = ids of the fake prefix: 1 (all prefix slots) and start_mel 8192  (gpt/model.py:528-530); behind a prompt also its codes
    // (:561-564)
    DTTS_CHECK_HIP(hipMemsetAsync(gs_.seen, 0, (size_t)B * V, s));
    DTTS_CHECK_HIP(hipMemsetAsync(gs_.finished, 0, sizeof(int) * B, s));
    launch_mark_seen(d_seen0, np_max + 1, d_nseen, B, V, gs_.seen, s);
    {   // rows that finish early are padded with 8193 (HF pad_token_id)
        std::vector<int> pad((size_t)B * G, 8193);
        DTTS_CHECK_HIP(hipMemcpyAsync(gs_.codes, pad.data(), sizeof(int) * pad.size(), hipMemcpyHostToDevice, s));
        std::vector<float> rs0(GEMV_MAXB, -1.0e9f), fs0(GEMV_MAXB, -1.0e9f), ld0((size_t)G + 1, 1.f);
        std::vector<int> zero(GEMV_MAXB, 0), one(GEMV_MAXB, 1), minus(GEMV_MAXB, -1);
        if (beamK) {                                 // HF's initial beam state: running scores [0, -1e9, ...], an empty finished set
            for (int b = 0; b < B; b += beamK) rs0[b] = 0.f;
            for (int i = 0; i <= G; ++i) ld0[i] = (float)std::pow((double)i, (double)o.length_penalty);     // Python's int ** float, rounded once
            DTTS_CHECK_HIP(hipMemcpyAsync(gs_.b_run_seq, pad.data(), sizeof(int) * pad.size(), hipMemcpyHostToDevice, s));
            DTTS_CHECK_HIP(hipMemcpyAsync(gs_.b_fin_seq, pad.data(), sizeof(int) * pad.size(), hipMemcpyHostToDevice, s));
            DTTS_CHECK_HIP(hipMemcpyAsync(gs_.b_run_score, rs0.data(), sizeof(float) * GEMV_MAXB, hipMemcpyHostToDevice, s));
            DTTS_CHECK_HIP(hipMemcpyAsync(gs_.b_fin_score, fs0.data(), sizeof(float) * GEMV_MAXB, hipMemcpyHostToDevice, s));
            DTTS_CHECK_HIP(hipMemcpyAsync(gs_.b_len_div, ld0.data(), sizeof(float) * ld0.size(), hipMemcpyHostToDevice, s));
            for (int* z : {gs_.b_fin_flag, gs_.b_fin_len, gs_.b_done, gs_.b_parents, gs_.b_tokens, gs_.b_ident})
                DTTS_CHECK_HIP(hipMemcpyAsync(z, zero.data(), sizeof(int) * GEMV_MAXB, hipMemcpyHostToDevice, s));
            DTTS_CHECK_HIP(hipMemcpyAsync(gs_.b_unsat, one.data(), sizeof(int) * GEMV_MAXB, hipMemcpyHostToDevice, s));
            DTTS_CHECK_HIP(hipMemcpyAsync(gs_.b_last_step, minus.data(), sizeof(int) * GEMV_MAXB, hipMemcpyHostToDevice, s));
        }
        DTTS_CHECK_HIP(hipStreamSynchronize(s));          // host temporaries (ids, pad, forced codes) are consumed
    }
    // ---- prefill over [cond | text | start_mel] or [cond | text | 1, start_mel, prompt]
    DTTS_CHECK_HIP(hipMemsetAsync(emb, 0, sizeof(float) * (size_t)B * C * Lp, s));
    launch_build_prefix(cond, d_ids, tl_max, d_tl, text_emb_, text_pos_, mel_emb_, mel_pos_, d_mel0, np_max, d_ml, B, C, Lp, emb, s);
    gpt_prefill_layers(emb, d_lp, B, Lp, gs_.kv, kv_layer, kv_bs, cap, s);
    launch_gather_last(emb, (long long)C * Lp, Lp, d_lp, 0, B, C, gs_.xa, s);
    // first token: lm_head = (final_norm, mel_head) applied to ln_f(h)   (gpt/model.py:41, 173)
    launch_gpt_final_ln(gs_.xa, nullptr, nullptr, 0, 0, B, lnf_g_, lnf_b_, fin_g_, fin_b_, gs_.lat, C, gs_.ctl, s);
    gpt_head_and_sample(s);
    gs_.steps = 1;
    gs_.active = true;
}

// mel_head GEMV on `lat` + sampler (the GEMV's finish is the sampler's prologue); the sampler leaves the next input embedding in y
void Model::gpt_head_and_sample(hipStream_t s) {
    const int C = cfg.gpt_dim, V = cfg.gpt_mel_codes, VP = mel_head_.CoutP, B = gs_.B;
    GemvIn in;
    in.x = gs_.lat;
    in.x_stride = C;
    launch_gemv_block(GP_PLAIN, mel_head_.w, C, VP, in, B, gs_.part, s);
    if (gs_.beam_K) {
        gpt_beam_launches(gs_.part, gemv_block_slices(C, VP), mel_head_.b, VP, s);
        return;
    }
    SamplerParams sp;
    sp.parts = gs_.part;
    sp.slices = gemv_block_slices(C, VP);
    sp.bias = mel_head_.b;
    sp.Vs = VP;
    sp.V = V;
    sp.B = B;
    sp.seen = gs_.seen;
    sp.finished = gs_.finished;
    sp.codes = gs_.codes;
    sp.codes_stride = gs_.G;
    sp.eos = 8193;
    sp.ctl = gs_.ctl;
    sp.mel_emb = mel_emb_;
    sp.mel_pos = mel_pos_;
    sp.x_next = gs_.y;
    sp.C = C;
    launch_sampler(sp, s);
}

// Beam session: beam_step_kernel in the sampler's place (same logits, same control block), then beam_reorder_kernel.  Fixed arguments:
// capturable like the sampler.
void Model::gpt_beam_launches(const float* parts, int slices, const float* bias, int Vs, hipStream_t s) {
    const int K = gs_.beam_K, U = gs_.B / K;
    BeamParams p{};
    p.parts = parts; p.slices = slices; p.bias = bias; p.Vs = Vs;
    p.V = cfg.gpt_mel_codes; p.U = U; p.K = K;
    p.seen = gs_.seen; p.finished = gs_.finished; p.eos = 8193; p.ctl = gs_.ctl;
    p.mel_emb = mel_emb_; p.mel_pos = mel_pos_; p.x_next = gs_.y; p.C = cfg.gpt_dim;
    p.run_seq = gs_.b_run_seq; p.fin_seq = gs_.b_fin_seq; p.seq_stride = gs_.G;
    p.run_score = gs_.b_run_score; p.fin_score = gs_.b_fin_score; p.fin_flag = gs_.b_fin_flag; p.fin_len = gs_.b_fin_len;
    p.unsat = gs_.b_unsat; p.done = gs_.b_done; p.parents = gs_.b_parents; p.tokens = gs_.b_tokens;
    p.last_step = gs_.b_last_step; p.ident = gs_.b_ident; p.len_div = gs_.b_len_div;
    p.length_penalty = gs_.beam_lp; p.early_stopping = gs_.beam_es;
    {
        ProfScope ps("beam_step", 0.0, 0.0, s);
        launch_beam_step(p, s);
    }
    BeamReorderParams r{};
    r.kv = gs_.kv; r.kv_layer = gs_.kv_layer; r.kv_bs = gs_.kv_bs; r.cap = gs_.cap; r.NL = (int)gpt_layers_.size(); r.C = cfg.gpt_dim;
    r.seen = gs_.seen; r.V = cfg.gpt_mel_codes; r.U = U; r.K = K; r.ctl = gs_.ctl;
    r.parents = gs_.b_parents; r.tokens = gs_.b_tokens; r.last_step = gs_.b_last_step; r.ident = gs_.b_ident;
    r.skip_kv = opt_beam_skip_reorder_ ? 1 : 0;
    ProfScope ps("beam_reorder", 0.0, 0.0, s);
    launch_beam_reorder(r, s);
}

// One token for every row of the session: 5 launches per layer + final LayerNorms + mel_head + sampler, all with fixed arguments
// (the step index, positions and sampling state are read from the device control block) -> safe to capture in a hipGraph.
void Model::gpt_step_launches(hipStream_t s) {
    const int C = cfg.gpt_dim, H = cfg.gpt_heads, D = C / H, B = gs_.B, NL = (int)gpt_layers_.size();
    if (gpt_use_token_kernel()) {                       // 2 launches per token: the persistent token kernel + the sampler
        GptTokenParams p = tokp_;
        p.x_in = gs_.y;
        p.kv = gs_.kv;
        p.kv_layer = gs_.kv_layer;
        p.kv_bs = gs_.kv_bs;
        p.cap = gs_.cap;
        p.ctl = gs_.ctl;
        p.B = B;
        p.xch = gs_.xch;
        p.lat = gs_.lat;
        p.logits = gs_.logits;
        p.err = gs_.tok_err;
        p.epoch = gs_.tok_epoch;
        static const int env_excl = env_tri("DTTS_GPT_TOKEN_EXCLUSIVE_CU");
        p.exclusive_cu = env_excl >= 0 ? env_excl : (opt_tok_exclusive_ ? 1 : 0);
        static const int env_prio = env_int("DTTS_GPT_TOKEN_PRIO", 1);
        static const int env_nap = env_int("DTTS_GPT_TOKEN_NAP", 0);
        static const int env_ablate = env_int("DTTS_GPT_TOKEN_ABLATE", 0);
        p.prio = env_prio;
        p.poll_nap = env_nap;
        p.ablate = env_ablate;
        static const int env_min_rows = env_int("DTTS_GPT_TOKEN_MIN_ROWS", 0);
        p.min_rows = env_min_rows ? env_min_rows : opt_tok_min_rows_;
        static const int env_wgs = env_int("DTTS_GPT_TOKEN_WGS", 0);
        p.wgs = env_wgs ? env_wgs : gs_.tok_wgs;
        if (opt_tok_fault_ > 0 && --opt_tok_fault_ == 0) {      // test hook: what a timed-out exchange leaves behind (flag up, token dead)
            const int one = 1;
            DTTS_CHECK_HIP(hipMemcpyAsync(gs_.tok_err, &one, sizeof(int), hipMemcpyHostToDevice, s));
            if (opt_tok_fault_eos_) {        // ... and the sampler, drawing from the dead kernel's stale logits, "finishes" every row
                const std::vector<int> fin(B, 1);
                DTTS_CHECK_HIP(hipMemcpyAsync(gs_.finished, fin.data(), sizeof(int) * B, hipMemcpyHostToDevice, s));
            }
            DTTS_CHECK_HIP(hipStreamSynchronize(s));
        }
        {
            ProfScope ps("gpt_token", 0.0, 0.0, s);
            launch_gpt_token(p, s);
        }
        if (gs_.beam_K) {
            gpt_beam_launches(gs_.logits, 1, nullptr, GPT_TOKEN_VS, s);
            return;
        }
        SamplerParams sp;
        sp.parts = gs_.logits;
        sp.slices = 1;
        sp.bias = nullptr;
        sp.Vs = GPT_TOKEN_VS;
        sp.V = cfg.gpt_mel_codes;
        sp.B = B;
        sp.seen = gs_.seen;
        sp.finished = gs_.finished;
        sp.codes = gs_.codes;
        sp.codes_stride = gs_.G;
        sp.eos = 8193;
        sp.ctl = gs_.ctl;
        sp.mel_emb = mel_emb_;
        sp.mel_pos = mel_pos_;
        sp.x_next = gs_.y;
        sp.C = C;
        launch_sampler(sp, s);
        return;
    }
    const int st_sl = gemv_block_slices(C, gpt_layers_[0].attn.CoutP);      // statistics slices of a K = C RESSUM GEMV
    for (int l = 0; l < NL; ++l) {
        const GptLayerW& w = gpt_layers_[l];
        float* cache = gs_.kv + (size_t)l * gs_.kv_layer;
        const int sq = gemv_block_slices(C, w.attn.CoutP), spj = gemv_block_slices(C, w.proj.CoutP);
        const int sf = gemv_block_slices(C, w.fc.CoutP), s4 = gemv_block_slices(4 * C, w.fc2.CoutP);
        DTTS_REQUIRE(gemv_block_slices(C, w.fc.CoutP) == st_sl && st_sl <= 64, "statistics slices");
        GemvIn a;                                        // K1: X = Y + (previous layer's mlp projection) ; c_attn(gamma1 . X)
        a.x = gs_.y;
        a.x_stride = C;
        if (l > 0) {
            a.parts = gs_.part2;
            a.in_slices = s4;
            a.in_stride = gpt_layers_[l - 1].fc2.CoutP;
            a.in_bias = gpt_layers_[l - 1].fc2.b;
        }
        a.gamma = w.ln1_g;
        a.y_out = gs_.x;
        a.stats_out = gs_.st1;
        launch_gemv_block(GP_RESSUM, w.attn.w, C, w.attn.CoutP, a, B, gs_.part, s);
        const bool fp = gs_.fuse_proj && w.proj.CoutP == 768 && H == 16;
        if (fp) {                                        // K2 + K3: attention and its output projection, per-head partials in part2
            launch_decode_attention_qkv(gs_.part, sq, w.attn.CoutP, gs_.st1, st_sl, w.attn_c, w.attn_d, cache, gs_.kv_bs, gs_.cap, gs_.ctl, B, H,
                                        D, gs_.part2, s, w.proj.w, w.proj.CoutP);
        } else {
            launch_decode_attention_qkv(gs_.part, sq, w.attn.CoutP, gs_.st1, st_sl, w.attn_c, w.attn_d, cache, gs_.kv_bs, gs_.cap, gs_.ctl, B, H,
                                        D, gs_.ab, s);
            GemvIn p;                                    // K3: attention projection (combines the key splits)
            p.parts = gs_.ab;
            p.in_slices = decode_attention_splits();
            p.in_stride = D;
            launch_gemv_block(GP_ATTN, w.proj.w, C, w.proj.CoutP, p, B, gs_.part2, s);
        }
        GemvIn f;                                        // K4: Y = X + proj ; c_fc(gamma2 . Y)
        f.x = gs_.x;
        f.x_stride = C;
        f.parts = gs_.part2;
        f.in_slices = fp ? H : spj;
        f.in_stride = w.proj.CoutP;
        f.in_bias = w.proj.b;
        f.gamma = w.ln2_g;
        f.y_out = gs_.y;
        f.stats_out = gs_.st2;
        launch_gemv_block(GP_RESSUM, w.fc.w, C, w.fc.CoutP, f, B, gs_.part, s);
        GemvIn m;                                        // K5: c_proj(gelu(ln_2 finish of c_fc))
        m.parts = gs_.part;
        m.in_slices = sf;
        m.in_stride = w.fc.CoutP;
        m.in_act = ACT_GELU_NEW;
        m.stats_in = gs_.st2;
        m.stats_slices = st_sl;
        m.K_ln = C;
        m.fold_c = w.fc_c;
        m.fold_d = w.fc_d;
        launch_gemv_block(GP_LNPARTS, w.fc2.w, 4 * C, w.fc2.CoutP, m, B, gs_.part2, s);
    }
    const GptLayerW& wl = gpt_layers_[NL - 1];
    launch_gpt_final_ln(gs_.y, wl.fc2.b, gs_.part2, gemv_block_slices(4 * C, wl.fc2.CoutP), wl.fc2.CoutP, B, lnf_g_, lnf_b_, fin_g_, fin_b_,
                        gs_.lat, C, gs_.ctl, s);
    gpt_head_and_sample(s);
}

void Model::gpt_decode_step(hipStream_t s) {
    DTTS_REQUIRE(gs_.active, "dtts_gpt_decode_step: no session (call dtts_gpt_prefill first)");
    gpt_step_launches(s);                 // beyond max_generate_length the kernels are device-side no-ops (GptCtl::max_steps)
    gs_.steps = std::min(gs_.steps + 1, gs_.G);
}

void Model::gpt_drop_graphs() {
    for (auto& g : gpt_graph_)
        if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
}

static int gpt_graph_chunk() {
    static const int n = []() { const int k = env_int("DTTS_GPT_GRAPH_CHUNK", 16); return k < 1 ? 1 : (k > 64 ? 64 : k); }();
    return n;
}

// captures `n` decode steps on the internal stream (kernel nodes only; the stream is not the legacy default stream, which cannot be
// captured) and instantiates them
hipGraphExec_t Model::gpt_capture(int n) {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    DTTS_CHECK_HIP(hipStreamBeginCapture(sg_, hipStreamCaptureModeRelaxed));
    try {
        for (int i = 0; i < n; ++i) gpt_step_launches(sg_);
    } catch (...) {
        (void)hipStreamEndCapture(sg_, &graph);
        if (graph) (void)hipGraphDestroy(graph);
        throw;
    }
    DTTS_CHECK_HIP(hipStreamEndCapture(sg_, &graph));
    const hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    DTTS_CHECK_HIP(e);
    return exec;
}

// n more tokens (clamped to the session's max_generate_length) through the captured graphs: chunks of 16 steps + single steps, on the
// handle's internal stream, ordered after / before `s` by events.  Asynchronous; no host work per token.
int Model::gpt_decode(int n_steps, hipStream_t s) {
    DTTS_REQUIRE(gs_.active, "dtts_gpt_decode: no session (call dtts_gpt_prefill first)");
    int n = std::min(n_steps, gs_.G - gs_.steps);
    if (n <= 0) return 0;
    static const int env_graph = env_tri("DTTS_GPT_GRAPH");
    if (!(env_graph >= 0 ? env_graph != 0 : opt_gpt_graph_)) {
        for (int i = 0; i < n; ++i) gpt_step_launches(s);
        gs_.steps += n;
        return n;
    }
    if (!sg_) {
        DTTS_CHECK_HIP(hipStreamCreateWithFlags(&sg_, hipStreamNonBlocking));
        DTTS_CHECK_HIP(hipEventCreateWithFlags(&ev_g0_, hipEventDisableTiming));
        DTTS_CHECK_HIP(hipEventCreateWithFlags(&ev_g1_, hipEventDisableTiming));
    }
    const int chunk = gpt_graph_chunk();
    DTTS_CHECK_HIP(hipEventRecord(ev_g0_, s));
    DTTS_CHECK_HIP(hipStreamWaitEvent(sg_, ev_g0_, 0));
    int left = n;
    if (left >= chunk && chunk > 1) {
        if (!gpt_graph_[0]) gpt_graph_[0] = gpt_capture(chunk);
        for (; left >= chunk; left -= chunk) DTTS_CHECK_HIP(hipGraphLaunch(gpt_graph_[0], sg_));
    }
    if (left > 0) {
        if (!gpt_graph_[1]) gpt_graph_[1] = gpt_capture(1);
        for (; left > 0; --left) DTTS_CHECK_HIP(hipGraphLaunch(gpt_graph_[1], sg_));
    }
    DTTS_CHECK_HIP(hipEventRecord(ev_g1_, sg_));
    DTTS_CHECK_HIP(hipStreamWaitEvent(s, ev_g1_, 0));
    gs_.steps += n;
    return n;
}

// != 0 when every row has drawn the stop token (synchronises the stream)
int Model::gpt_all_finished(hipStream_t s) {
    DTTS_REQUIRE(gs_.active, "no GPT session");
    int fin[GEMV_MAXB];
    DTTS_CHECK_HIP(hipMemcpyAsync(fin, gs_.finished, sizeof(int) * gs_.B, hipMemcpyDeviceToHost, s));
    DTTS_CHECK_HIP(hipStreamSynchronize(s));
    return std::all_of(fin, fin + gs_.B, [](int f) { return f != 0; }) ? 1 : 0;
}

// A session whose persistent token kernel raised its error flag is replayed from its prefill on the launch-per-GEMV chain; the caller
// then reads the results again.  hctl: the failed session's control block.
bool Model::gpt_replay_failed(const GptCtl& hctl, hipStream_t s) {
    const int B = gs_.B, G = gs_.G;
    // An exchange poll of the persistent token kernel gave up (its 128 workgroups were not all resident: CU mask, partition mode,
    // another process holding CUs).  The handle leaves the token kernel for good and THIS session is replayed from its prefill on
    // the launch-per-GEMV chain - same sampler, same Philox draws, so the codes are the ones the chain would have produced.
    // Did the FAILED session look finished?  Once the kernel is dead the sampler draws from stale logits, so rows may have drawn the
    // stop token spuriously and the caller's decode loop (gpt_all_finished) stopped on that: the replay must then go on past the
    // failed session's step count until the chain's own rows have finished (silently truncated audio otherwise).
    int fin[GEMV_MAXB];
    DTTS_CHECK_HIP(hipMemcpyAsync(fin, gs_.finished, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    DTTS_CHECK_HIP(hipMemsetAsync(gs_.tok_err, 0, sizeof(int), s));
    DTTS_CHECK_HIP(hipStreamSynchronize(s));
    const bool failed_looked_finished = std::all_of(fin, fin + B, [](int f) { return f != 0; });
    gs_.active = false;
    tok_failed_ = true;
    gpt_drop_graphs();
    int steps = gs_.steps;
    for (int b = 0; b < B; ++b) steps = std::max(steps, std::min(hctl.step[b], G));
    fprintf(stderr, "[detail_hip] persistent decode kernel: an activation exchange timed out; replaying %d tokens on the launch-per-GEMV chain "
                    "(this handle stays on the chain)\n", steps);
    DTTS_REQUIRE(replay_.valid && !replaying_, "persistent decode kernel: an activation exchange timed out and the session cannot be replayed; "
                                               "set DTTS_GPT_TOKEN_KERNEL=0");
    GptReplay& r = replay_;
    dtts_gpt_options o = r.o;
    o.sample_ids = r.sample_ids.data();
    o.forced_codes = r.forced_codes.empty() ? nullptr : r.forced_codes.data();
    o.row_seeds = r.row_seeds.empty() ? nullptr : r.row_seeds.data();
    if (!r.rows.empty()) {
        for (size_t b = 0; b < r.rows.size(); ++b) {
            r.rows[b].suppress_tokens = r.row_ids[2 * b].empty() ? nullptr : r.row_ids[2 * b].data();
            r.rows[b].begin_suppress_tokens = r.row_ids[2 * b + 1].empty() ? nullptr : r.row_ids[2 * b + 1].data();
        }
        o.row_options = r.rows.data();
    } else o.row_options = nullptr;
    if (o.prompt_codes) { o.prompt_codes = r.prompt_codes.data(); o.prompt_lens = r.prompt_lens.data(); }
    o.suppress_tokens = r.suppress.empty() ? nullptr : r.suppress.data();
    o.begin_suppress_tokens = r.begin_suppress.empty() ? nullptr : r.begin_suppress.data();
    replaying_ = true;
    try {
        gpt_replay_.reset();
        const float* kept = gpt_replay_.f32(r.has_cond ? (size_t)r.B * cfg.gpt_dim : (size_t)r.B * cfg.mel_channels * r.Tr);
        gpt_prefill(r.has_cond ? nullptr : kept, r.has_refer_lens ? r.refer_lens.data() : nullptr, r.Tr, r.text.data(),
                    r.has_text_lens ? r.text_lens.data() : nullptr, r.Lt_max, r.B, o, r.latents_cm, r.lat_stride, s, r.has_cond ? kept : nullptr);
        for (int i = 1; i < steps; ++i) gpt_step_launches(s);
        gs_.steps = steps;
        if (!o.suppress_eos && failed_looked_finished)
            while (gs_.steps < G && !gpt_all_finished(s)) {
                const int n = std::min(16, G - gs_.steps);
                for (int i = 0; i < n; ++i) gpt_step_launches(s);
                gs_.steps += n;
            }
    } catch (...) {
        replaying_ = false;
        throw;
    }
    replaying_ = false;
    return true;
}

// results: codes include the stop token; rows that finished early are padded with 8193 (HF pad_token_id).  Synchronises.
void Model::gpt_finish(int* codes_host, int* ncodes_host, hipStream_t s) {
    DTTS_REQUIRE(gs_.active, "dtts_gpt_finish: no session");
    DTTS_REQUIRE(!gs_.beam_K, "dtts_gpt_finish: a beam session's results are hypotheses and scores: call dtts_gpt_beam_finish");
    const int B = gs_.B, G = gs_.G, Ga = gs_.G;
    std::vector<int> hc((size_t)B * Ga, 8193);
    GptCtl hctl;
    DTTS_CHECK_HIP(hipMemcpyAsync(hc.data(), gs_.codes, sizeof(int) * hc.size(), hipMemcpyDeviceToHost, s));
    // the DEVICE step counters are the truth: the sampler advances them, also when the steps were replayed from a caller-owned graph
    // (dtts_gpt_decode_step captured once, replayed n times: the host counter gs_.steps saw one call); steps >= G were device no-ops
    DTTS_CHECK_HIP(hipMemcpyAsync(&hctl, gs_.ctl, sizeof(GptCtl), hipMemcpyDeviceToHost, s));
    int tok_err = 0;
    if (gs_.tok_err) DTTS_CHECK_HIP(hipMemcpyAsync(&tok_err, gs_.tok_err, sizeof(int), hipMemcpyDeviceToHost, s));
    DTTS_CHECK_HIP(hipStreamSynchronize(s));
    if (tok_err && gpt_replay_failed(hctl, s)) {
        DTTS_CHECK_HIP(hipMemcpyAsync(hc.data(), gs_.codes, sizeof(int) * hc.size(), hipMemcpyDeviceToHost, s));
        DTTS_CHECK_HIP(hipMemcpyAsync(&hctl, gs_.ctl, sizeof(GptCtl), hipMemcpyDeviceToHost, s));
        DTTS_CHECK_HIP(hipStreamSynchronize(s));
    }
    for (int b = 0; b < B; ++b) {
        // (a row's own cap: what lies behind it is the latched row's padding; row_max_steps = G in a uniform session)
        const int done = std::max(0, std::min(std::min(hctl.step[b], G), hctl.row_max_steps[b]));
        int n = done;
        for (int t = 0; t < done; ++t)
            if (hc[(size_t)b * Ga + t] == 8193) { n = t + 1; break; }
        if (ncodes_host) ncodes_host[b] = n;
        if (codes_host)
            for (int t = 0; t < G; ++t) codes_host[(size_t)b * G + t] = t < done ? hc[(size_t)b * Ga + t] : 8193;
    }
    gs_.active = false;
}

// UnifiedVoice.inference_speech_tortoise (gpt/model.py:514-545) or, with prompt_codes, inference_speech_valle (:546-579): prefill +
// decode loop + results.  Batches larger than one session
// (8 rows) run group after group; the finish flags are polled once per 16-token graph (never per token).
void Model::gpt_generate(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host,
                         int Lt_max, int B, const dtts_gpt_options& o, int* codes_host, int* ncodes_host, float* latents_cm,
                         int lat_stride, hipStream_t s, const float* cond_in) {
    DTTS_REQUIRE(B >= 1, "gpt batch");
    DTTS_REQUIRE(o.sample_ids, "sample_ids");
    DTTS_REQUIRE(o.num_beams <= 1, "dtts_gpt_generate: num_beams > 1 returns hypotheses and scores: call dtts_gpt_beam_generate");
    const int C = cfg.gpt_dim, G = o.max_generate_length, chunk = gpt_graph_chunk();
    for (int g0 = 0; g0 < B; g0 += GEMV_MAXB) {
        const int nb = std::min(GEMV_MAXB, B - g0);
        dtts_gpt_options og = o;
        og.sample_ids = o.sample_ids + g0;
        if (o.forced_uniforms) og.forced_uniforms = o.forced_uniforms + (size_t)g0 * G;
        if (o.forced_codes) og.forced_codes = o.forced_codes + (size_t)g0 * G;
        if (o.row_seeds) og.row_seeds = o.row_seeds + g0;
        if (o.row_options) og.row_options = o.row_options + g0;
        if (o.prompt_codes) og.prompt_codes = o.prompt_codes + (size_t)g0 * o.prompt_stride;
        if (o.prompt_lens) og.prompt_lens = o.prompt_lens + g0;
        gpt_prefill(cond_in ? nullptr : refer + (size_t)g0 * cfg.mel_channels * Tr, refer_lens_host ? refer_lens_host + g0 : nullptr, Tr,
                    text_host + (size_t)g0 * Lt_max, text_lens_host ? text_lens_host + g0 : nullptr, Lt_max, nb, og,
                    latents_cm ? latents_cm + (size_t)g0 * C * lat_stride : nullptr, lat_stride, s, cond_in ? cond_in + (size_t)g0 * C : nullptr);
        while (gs_.steps < G) {
            if (!o.suppress_eos && gpt_all_finished(s)) break;
            gpt_decode(chunk, s);
        }
        gpt_finish(codes_host + (size_t)g0 * G, ncodes_host + g0, s);
    }
}

// results of a beam session: per utterance the best nrs finished hypotheses in score order (HF: sequences[:, :num_return_sequences]),
// their generated lengths and sequences_scores.  Synchronises; ends the session.
void Model::gpt_beam_finish(int nrs, int* seqs_host, int* lens_host, float* scores_host, hipStream_t s) {
    DTTS_REQUIRE(gs_.active && gs_.beam_K > 1, "dtts_gpt_beam_finish: no beam session");
    const int B = gs_.B, G = gs_.G, K = gs_.beam_K, U = B / K;
    DTTS_REQUIRE(nrs >= 1 && nrs <= K, "dtts_gpt_beam_finish: num_return_sequences outside 1 .. num_beams");
    std::vector<int> hseq((size_t)B * G), hlen(GEMV_MAXB);
    std::vector<float> hsc(GEMV_MAXB);
    GptCtl hctl;
    int tok_err = 0;
    auto fetch = [&]() {
        DTTS_CHECK_HIP(hipMemcpyAsync(hseq.data(), gs_.b_fin_seq, sizeof(int) * hseq.size(), hipMemcpyDeviceToHost, s));
        DTTS_CHECK_HIP(hipMemcpyAsync(hlen.data(), gs_.b_fin_len, sizeof(int) * GEMV_MAXB, hipMemcpyDeviceToHost, s));
        DTTS_CHECK_HIP(hipMemcpyAsync(hsc.data(), gs_.b_fin_score, sizeof(float) * GEMV_MAXB, hipMemcpyDeviceToHost, s));
        DTTS_CHECK_HIP(hipMemcpyAsync(&hctl, gs_.ctl, sizeof(GptCtl), hipMemcpyDeviceToHost, s));
        DTTS_CHECK_HIP(hipStreamSynchronize(s));
    };
    if (gs_.tok_err) DTTS_CHECK_HIP(hipMemcpyAsync(&tok_err, gs_.tok_err, sizeof(int), hipMemcpyDeviceToHost, s));
    fetch();
    if (tok_err && gpt_replay_failed(hctl, s)) fetch();      // (the replay record carries the beam fields: still a beam session)
    for (int u = 0; u < U; ++u)
        for (int j = 0; j < nrs; ++j) {
            const int row = u * K + j;
            const size_t o = (size_t)u * nrs + j;
            lens_host[o] = hlen[row];
            scores_host[o] = hsc[row];
            for (int t = 0; t < G; ++t) seqs_host[o * G + t] = t < hlen[row] ? hseq[(size_t)row * G + t] : 8193;
        }
    gs_.active = false;
}

// dtts_gpt_generate under num_beams = K: every utterance becomes K replica rows (HF's repeat_interleave); a group is floor(16 / K) whole
// utterances.  The K prefills of an utterance are computed K times (sharing them is a follow-up).
void Model::gpt_beam_generate(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host,
                              int Lt_max, int B, const dtts_gpt_options& o, int nrs, int* seqs_host, int* lens_host, float* scores_host,
                              hipStream_t s, const float* cond_in) {
    DTTS_REQUIRE(B >= 1, "gpt batch");
    const int K = o.num_beams, G = o.max_generate_length, chunk = gpt_graph_chunk();
    DTTS_REQUIRE(K > 1 && K <= BEAM_MAXK && nrs >= 1 && nrs <= K, "gpt_beam_generate: num_beams 2 .. 16, num_return_sequences 1 .. num_beams");
    DTTS_REQUIRE((cond_in || (refer && Tr >= 1)) && text_host && Lt_max >= 0, "gpt_beam_generate: operands");
    const int per = GEMV_MAXB / K;
    const float* src = cond_in ? cond_in : refer;    // what a beam row repeats: the utterance's cond vector, or its prompt mel
    const size_t mel = cond_in ? (size_t)cfg.gpt_dim : (size_t)cfg.mel_channels * Tr;
    gpt_beam_in_.ensure(sizeof(float) * mel * GEMV_MAXB + 4096);
    for (int g0 = 0; g0 < B; g0 += per) {
        const int nu = std::min(per, B - g0), R = nu * K;
        gpt_beam_in_.reset();
        float* rf = gpt_beam_in_.f32(mel * R);
        std::vector<int> rl(R), tx((size_t)R * std::max(Lt_max, 1), 0), tl(R), sid(R), pc, pl;
        if (o.prompt_codes) { pc.assign((size_t)R * std::max(o.prompt_stride, 1), 0); pl.assign(R, 0); }
        for (int r = 0; r < R; ++r) {
            const int b = g0 + r / K;
            DTTS_CHECK_HIP(hipMemcpyAsync(rf + mel * r, src + mel * b, sizeof(float) * mel, hipMemcpyDeviceToDevice, s));
            rl[r] = !cond_in && refer_lens_host ? refer_lens_host[b] : Tr;
            tl[r] = text_lens_host ? text_lens_host[b] : Lt_max;
            std::copy(text_host + (size_t)b * Lt_max, text_host + (size_t)(b + 1) * Lt_max, tx.begin() + (size_t)r * Lt_max);
            sid[r] = o.sample_ids ? o.sample_ids[b] : 0;
            if (o.prompt_codes) {
                pl[r] = o.prompt_lens[b];
                std::copy(o.prompt_codes + (size_t)b * o.prompt_stride, o.prompt_codes + (size_t)(b + 1) * o.prompt_stride,
                          pc.begin() + (size_t)r * o.prompt_stride);
            }
        }
        dtts_gpt_options og = o;
        og.sample_ids = sid.data();
        og.row_seeds = nullptr;
        DTTS_REQUIRE(!o.row_options, "gpt_beam_generate: row_options (a beam session is uniform)");
        if (o.prompt_codes) { og.prompt_codes = pc.data(); og.prompt_lens = pl.data(); }
        gpt_prefill(cond_in ? nullptr : rf, rl.data(), Tr, tx.data(), tl.data(), Lt_max, R, og, nullptr, 0, s, cond_in ? rf : nullptr);
        while (gs_.steps < G) {
            if (gpt_all_finished(s)) break;
            gpt_decode(chunk, s);
        }
        gpt_beam_finish(nrs, seqs_host + (size_t)g0 * nrs * G, lens_host + (size_t)g0 * nrs, scores_host + (size_t)g0 * nrs, s);
    }
}

// unit entry: ONE beam step on given logits, the state handed in and out on the host (tests/test_gpu_beam.py)
void Model::op_beam_step(const float* logits, int U, int V, const dtts_gpt_options& o, int step, const int* prompt_host, int prompt_len,
                         int* run_seq, float* run_score, int* fin_seq, float* fin_score, int* fin_flag, int* fin_len, int* unsat, int* done,
                         int* parents, int* tokens, float* cand_score, int* cand_beam, int* cand_tok, hipStream_t s) {
    const int K = o.num_beams, G = o.max_generate_length, R = U * K, n = o.no_repeat_ngram_size;
    DTTS_REQUIRE(K >= 1 && K <= BEAM_MAXK && U >= 1 && R <= GEMV_MAXB, "op_beam_step: 1 .. 16 beams, at most 16 rows");
    DTTS_REQUIRE(V >= 2 && V <= BEAM_V_MAX && G >= 1 && step >= 0 && step < G && prompt_len >= 0, "op_beam_step: V, max_generate_length, step");
    DTTS_REQUIRE(logits && run_seq && run_score && fin_seq && fin_score && fin_flag && fin_len && unsat && done && parents && tokens &&
                     cand_score && cand_beam && cand_tok && (prompt_host || prompt_len == 0), "op_beam_step: null argument");
    DTTS_REQUIRE(n >= 0 && n <= SAMP_NGRAM_MAX, "no_repeat_ngram_size outside 0 .. 16");
    const int hs = prompt_len + G;
    std::vector<unsigned char> seen((size_t)R * V, 0);
    std::vector<int> hist((size_t)R * hs, 0);
    GptCtl c;
    std::memset(&c, 0, sizeof(c));
    for (int r = 0; r < R; ++r) {
        int* h = hist.data() + (size_t)r * hs;
        for (int j = 0; j < prompt_len; ++j) h[j] = prompt_host[(size_t)(r / K) * prompt_len + j];
        for (int j = 0; j < step; ++j) h[prompt_len + j] = run_seq[(size_t)r * G + j];
        for (int j = 0; j < prompt_len + step; ++j) {
            DTTS_REQUIRE(h[j] >= 0 && h[j] < V, "op_beam_step: id outside the vocabulary");
            seen[(size_t)r * V + h[j]] = 1;
        }
        c.step[r] = step;
        c.hist_n0[r] = prompt_len;
        c.stop_from[r] = gpt_first_stop_step(prompt_len, 0, o.min_length, o.min_new_tokens);
        c.decay_off[r] = o.exp_decay_start;
    }
    std::vector<float> ld((size_t)G + 1);
    for (int i = 0; i <= G; ++i) ld[i] = (float)std::pow((double)i, (double)o.length_penalty);
    const GptRowTables tabs = gpt_ctl_rows(c, o, R, V, G, G + 1);
    const size_t ni = (size_t)2 * R * G + (size_t)R * hs + 8 * GEMV_MAXB + 2 * GEMV_MAXB * 2, nf = (size_t)G + 1 + 2 * GEMV_MAXB + 2 * GEMV_MAXB + G + 1;
    ws().ensure((size_t)R * V + (size_t)V + sizeof(int) * ni + sizeof(float) * nf + sizeof(GptCtl) + 40 * 256);
    unsigned char* d_seen = static_cast<unsigned char*>(ws().raw((size_t)R * V));
    unsigned char* d_mask = static_cast<unsigned char*>(ws().raw((size_t)V));
    int* d_hist = ws().i32((size_t)R * hs);
    int *d_rs = ws().i32((size_t)R * G), *d_fs = ws().i32((size_t)R * G);
    int *d_flag = ws().i32(GEMV_MAXB), *d_len = ws().i32(GEMV_MAXB), *d_unsat = ws().i32(GEMV_MAXB), *d_done = ws().i32(GEMV_MAXB);
    int *d_par = ws().i32(GEMV_MAXB), *d_tok = ws().i32(GEMV_MAXB), *d_last = ws().i32(GEMV_MAXB), *d_ident = ws().i32(GEMV_MAXB);
    int *d_cb = ws().i32(2 * GEMV_MAXB), *d_ct = ws().i32(2 * GEMV_MAXB);
    float *d_rsc = ws().f32(GEMV_MAXB), *d_fsc = ws().f32(GEMV_MAXB), *d_ld = ws().f32((size_t)G + 1), *d_cs = ws().f32(2 * GEMV_MAXB);
    float* d_decay = ws().f32((size_t)G + 1);
    GptCtl* dctl = static_cast<GptCtl*>(ws().raw(sizeof(GptCtl)));
    c.suppress_eos = o.suppress_eos;
    c.max_steps = G;
    c.hist = n > 0 ? d_hist : nullptr;
    c.hist_stride = hs;
    if (!tabs.mask.empty()) {
        c.tok_mask = d_mask;
        DTTS_CHECK_HIP(hipMemcpyAsync(d_mask, tabs.mask.data(), tabs.mask.size(), hipMemcpyHostToDevice, s));
    }
    if (!tabs.decay.empty()) {
        c.decay_mul = d_decay;
        DTTS_CHECK_HIP(hipMemcpyAsync(d_decay, tabs.decay.data(), sizeof(float) * tabs.decay.size(), hipMemcpyHostToDevice, s));
    }
    auto up = [&](void* d, const void* h, size_t bytes) { DTTS_CHECK_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s)); };
    auto down = [&](void* h, const void* d, size_t bytes) { DTTS_CHECK_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s)); };
    up(dctl, &c, sizeof(c));
    up(d_seen, seen.data(), seen.size());
    up(d_hist, hist.data(), sizeof(int) * hist.size());
    up(d_rs, run_seq, sizeof(int) * (size_t)R * G);
    up(d_fs, fin_seq, sizeof(int) * (size_t)R * G);
    up(d_flag, fin_flag, sizeof(int) * R);
    up(d_len, fin_len, sizeof(int) * R);
    up(d_unsat, unsat, sizeof(int) * U);
    up(d_done, done, sizeof(int) * U);
    up(d_rsc, run_score, sizeof(float) * R);
    up(d_fsc, fin_score, sizeof(float) * R);
    up(d_ld, ld.data(), sizeof(float) * ld.size());
    DTTS_CHECK_HIP(hipMemsetAsync(d_par, 0, sizeof(int) * GEMV_MAXB, s));
    DTTS_CHECK_HIP(hipMemsetAsync(d_tok, 0, sizeof(int) * GEMV_MAXB, s));
    DTTS_CHECK_HIP(hipMemsetAsync(d_cs, 0, sizeof(float) * 2 * GEMV_MAXB, s));
    DTTS_CHECK_HIP(hipMemsetAsync(d_cb, 0, sizeof(int) * 2 * GEMV_MAXB, s));
    DTTS_CHECK_HIP(hipMemsetAsync(d_ct, 0, sizeof(int) * 2 * GEMV_MAXB, s));
    BeamParams p{};
    p.parts = logits; p.slices = 1; p.bias = nullptr; p.Vs = V; p.V = V; p.U = U; p.K = K;
    p.seen = d_seen; p.finished = nullptr; p.eos = V - 1; p.ctl = dctl;
    p.run_seq = d_rs; p.fin_seq = d_fs; p.seq_stride = G; p.run_score = d_rsc; p.fin_score = d_fsc; p.fin_flag = d_flag; p.fin_len = d_len;
    p.unsat = d_unsat; p.done = d_done; p.parents = d_par; p.tokens = d_tok; p.last_step = d_last; p.ident = d_ident; p.len_div = d_ld;
    p.length_penalty = o.length_penalty; p.early_stopping = o.early_stopping;
    p.cand_score = d_cs; p.cand_beam = d_cb; p.cand_tok = d_ct;
    launch_beam_step(p, s);
    down(run_seq, d_rs, sizeof(int) * (size_t)R * G);
    down(fin_seq, d_fs, sizeof(int) * (size_t)R * G);
    down(fin_flag, d_flag, sizeof(int) * R);
    down(fin_len, d_len, sizeof(int) * R);
    down(unsat, d_unsat, sizeof(int) * U);
    down(done, d_done, sizeof(int) * U);
    down(run_score, d_rsc, sizeof(float) * R);
    down(fin_score, d_fsc, sizeof(float) * R);
    down(parents, d_par, sizeof(int) * R);
    down(tokens, d_tok, sizeof(int) * R);
    down(cand_score, d_cs, sizeof(float) * (size_t)U * 2 * K);
    down(cand_beam, d_cb, sizeof(int) * (size_t)U * 2 * K);
    down(cand_tok, d_ct, sizeof(int) * (size_t)U * 2 * K);
    DTTS_CHECK_HIP(hipStreamSynchronize(s));
}

// unit entry: the device sampler on given logits rows (HF logits processors + inverse-CDF draw), one token per row
void Model::op_sample_logits(const float* logits, int R, int V, const int* history_host, int hist_len, const float* uniforms, int top_k,
                             float top_p, float temperature, float repetition_penalty, float typical_mass, int suppress_eos,
                             int* tokens_host, hipStream_t s) {
    DTTS_REQUIRE(R >= 1 && R <= GEMV_MAXB, "op_sample_logits: rows 1..16");
    DTTS_REQUIRE(V >= 2 && V <= sampler_max_vocab(), "op_sample_logits: vocabulary outside 2 .. the LDS sampler's maximum");
    ws().ensure((size_t)R * V + sizeof(int) * 4 * R + sizeof(GptCtl) + 16 * 256);
    unsigned char* seen = static_cast<unsigned char*>(ws().raw((size_t)R * V));
    int* finished = ws().i32(R);
    int* codes = ws().i32(R);
    GptCtl* dctl = static_cast<GptCtl*>(ws().raw(sizeof(GptCtl)));
    std::vector<unsigned char> hs((size_t)R * V, 0);
    for (int r = 0; r < R; ++r)
        for (int j = 0; j < hist_len; ++j) {
            const int id = history_host[(size_t)r * hist_len + j];
            DTTS_REQUIRE(id >= 0 && id < V, "history id");
            hs[(size_t)r * V + id] = 1;
        }
    GptCtl c;
    std::memset(&c, 0, sizeof(c));
    for (int r = 0; r < R; ++r) {
        c.repetition_penalty[r] = repetition_penalty;
        c.temperature[r] = temperature;
        c.top_p[r] = top_p;
        c.top_k[r] = top_k;
        c.typical_mass[r] = typical_mass;
        c.row_max_steps[r] = 1;
    }
    c.suppress_eos = suppress_eos;
    c.max_steps = 1;
    c.forced_u = uniforms;
    c.u_stride = 1;
    DTTS_CHECK_HIP(hipMemcpyAsync(dctl, &c, sizeof(c), hipMemcpyHostToDevice, s));
    DTTS_CHECK_HIP(hipMemcpyAsync(seen, hs.data(), hs.size(), hipMemcpyHostToDevice, s));
    DTTS_CHECK_HIP(hipMemsetAsync(finished, 0, sizeof(int) * R, s));
    SamplerParams sp;
    sp.parts = logits;
    sp.slices = 1;
    sp.bias = nullptr;
    sp.Vs = V;
    sp.V = V;
    sp.B = R;
    sp.seen = seen;
    sp.finished = finished;
    sp.codes = codes;
    sp.codes_stride = 1;
    sp.eos = V - 1;
    sp.ctl = dctl;
    sp.mel_emb = nullptr;
    sp.mel_pos = nullptr;
    sp.x_next = nullptr;
    sp.C = 0;
    launch_sampler(sp, s);
    DTTS_CHECK_HIP(hipMemcpyAsync(tokens_host, codes, sizeof(int) * R, hipMemcpyDeviceToHost, s));
    DTTS_CHECK_HIP(hipStreamSynchronize(s));
}

// unit entry: the sampler under a whole option block, on rows whose input_ids are `fills[r]` fill ids followed by an ordered history
void Model::op_sample_logits_opts(const float* logits, int R, int V, const dtts_gpt_options& o, const int* history_host, int hist_stride,
                                  const int* hist_lens, const int* fills, const int* prompt_lens, const float* uniforms, int* tokens_host,
                                  hipStream_t s) {
    DTTS_REQUIRE(R >= 1 && R <= GEMV_MAXB, "op_sample_logits_opts: rows 1..16");
    DTTS_REQUIRE(V >= 2 && V <= sampler_max_vocab(), "op_sample_logits_opts: vocabulary outside 2 .. the LDS sampler's maximum");
    DTTS_REQUIRE(logits && uniforms && tokens_host && hist_lens && fills && prompt_lens && hist_stride >= 0, "op_sample_logits_opts: operands");
    const int hs = hist_stride + 1;                       // the sampler appends the drawn token behind the row's history
    std::vector<unsigned char> seen((size_t)R * V, 0);
    std::vector<int> hist((size_t)R * hs, 0);
    GptCtl c;
    std::memset(&c, 0, sizeof(c));
    int decay_n = 2;
    for (int r = 0; r < R; ++r) {
        DTTS_REQUIRE(hist_lens[r] >= 0 && hist_lens[r] <= hist_stride && fills[r] >= 0, "op_sample_logits_opts: hist_lens / fills");
        DTTS_REQUIRE(hist_lens[r] == 0 || history_host, "op_sample_logits_opts: history");
        const int cur = fills[r] + hist_lens[r];          // len(input_ids)
        DTTS_REQUIRE(prompt_lens[r] >= 0 && prompt_lens[r] <= cur, "op_sample_logits_opts: prompt_lens outside [0, fills + hist_lens]");
        if (fills[r] > 0) seen[(size_t)r * V + 1] = 1;
        for (int j = 0; j < hist_lens[r]; ++j) {
            const int id = history_host[(size_t)r * hist_stride + j];
            DTTS_REQUIRE(id >= 0 && id < V, "history id");
            seen[(size_t)r * V + id] = 1;
            hist[(size_t)r * hs + j] = id;
        }
        const dtts_gpt_row_options rw = gpt_row_settings(o, r);      // (dtts_op_sample_logits_rows: the row's own record)
        c.hist_n0[r] = hist_lens[r];
        c.nfill[r] = std::min(rw.no_repeat_ngram_size, fills[r]);
        const int fresh = cur - prompt_lens[r];           // tokens behind HF's prompt
        c.stop_from[r] = gpt_first_stop_step(cur, -fresh, rw.min_length, rw.min_new_tokens);      // > 0: the sampler's step 0 is in front of it
        const int i = fresh - rw.exp_decay_start;         // the sampler's step is 0: i = step - decay_off
        c.decay_off[r] = -i;
        decay_n = std::max(decay_n, i + 1);
        c.begin_step[r] = fresh == 0 ? 0 : -1;
    }
    const GptRowTables tabs = gpt_ctl_rows(c, o, R, V, 1, decay_n);
    const int n = tabs.ngram_max;
    ws().ensure((size_t)R * V + sizeof(int) * ((size_t)R * hs + 4 * R) + sizeof(GptCtl) + (size_t)R * V + sizeof(float) * (size_t)R * decay_n + 16 * 256);
    unsigned char* d_seen = static_cast<unsigned char*>(ws().raw((size_t)R * V));
    int* finished = ws().i32(R);
    int* codes = ws().i32(R);
    int* d_hist = ws().i32((size_t)R * hs);
    unsigned char* d_mask = static_cast<unsigned char*>(ws().raw((size_t)R * V));
    float* d_decay = ws().f32((size_t)R * decay_n);
    GptCtl* dctl = static_cast<GptCtl*>(ws().raw(sizeof(GptCtl)));
    c.suppress_eos = o.suppress_eos;
    c.max_steps = 1;
    c.forced_u = uniforms;
    c.u_stride = 1;
    c.hist = n > 0 ? d_hist : nullptr;
    c.hist_stride = hs;
    if (!tabs.mask.empty()) {
        c.tok_mask = d_mask;
        DTTS_CHECK_HIP(hipMemcpyAsync(d_mask, tabs.mask.data(), tabs.mask.size(), hipMemcpyHostToDevice, s));
    }
    if (!tabs.decay.empty()) {
        c.decay_mul = d_decay;
        DTTS_CHECK_HIP(hipMemcpyAsync(d_decay, tabs.decay.data(), sizeof(float) * tabs.decay.size(), hipMemcpyHostToDevice, s));
    }
    DTTS_CHECK_HIP(hipMemcpyAsync(dctl, &c, sizeof(c), hipMemcpyHostToDevice, s));
    DTTS_CHECK_HIP(hipMemcpyAsync(d_seen, seen.data(), seen.size(), hipMemcpyHostToDevice, s));
    DTTS_CHECK_HIP(hipMemcpyAsync(d_hist, hist.data(), sizeof(int) * hist.size(), hipMemcpyHostToDevice, s));
    DTTS_CHECK_HIP(hipMemsetAsync(finished, 0, sizeof(int) * R, s));
    SamplerParams sp;
    sp.parts = logits;
    sp.slices = 1;
    sp.bias = nullptr;
    sp.Vs = V;
    sp.V = V;
    sp.B = R;
    sp.seen = d_seen;
    sp.finished = finished;
    sp.codes = codes;
    sp.codes_stride = 1;
    sp.eos = V - 1;
    sp.ctl = dctl;
    sp.mel_emb = nullptr;
    sp.mel_pos = nullptr;
    sp.x_next = nullptr;
    sp.C = 0;
    launch_sampler(sp, s);
    DTTS_CHECK_HIP(hipMemcpyAsync(tokens_host, codes, sizeof(int) * R, hipMemcpyDeviceToHost, s));
    DTTS_CHECK_HIP(hipStreamSynchronize(s));
}

// The teacher-forced pass over [cond | 255, text, 0 | 8192, codes, 8193] (gpt/model.py:463-476, 392-403): see model.h
Model::GptForced Model::gpt_teacher_forced(const float* refer, const int* refer_lens_host, int Tr, const int* text_host,
                                           const int* text_lens_host, int Lt_max, const int* codes_host, const int* ncodes_host, int n_max,
                                           int B, size_t extra_ws_bytes, hipStream_t s, const float* cond_in, const GptAttnRequest* attn) {
    DTTS_REQUIRE(bound_ && has_gpt_, "gpt weights not bound");
    DTTS_REQUIRE(cond_in || (refer && Tr >= 1), "neither a prompt mel nor its conditioning latent");
    if (cond_in) Tr = 0;
    const int C = cfg.gpt_dim;
    GptForced f;
    std::vector<int> ids;
    int tl_max;
    text_prefix_ids(text_host, text_lens_host, B, Lt_max, cfg.gpt_text_tokens, ids, f.tl, tl_max);
    DTTS_REQUIRE(tl_max <= cfg.gpt_max_text_pos, "text too long");
    const std::vector<int>& tl = f.tl;
    std::vector<int>& ml = f.ml;
    ml.resize(B);
    std::vector<int> lt(B), nn(B);
    int ml_max = 0, L = 0;
    for (int b = 0; b < B; ++b) {
        nn[b] = ncodes_host ? ncodes_host[b] : n_max;
        DTTS_REQUIRE(nn[b] >= 0 && nn[b] <= n_max, "ncodes outside [0, n_max]");
        ml[b] = nn[b] + 2;                                  // start + codes + stop  (gpt/model.py:464, 470)
        ml_max = std::max(ml_max, ml[b]);
        lt[b] = 1 + tl[b] + ml[b];
        L = std::max(L, lt[b]);
    }
    DTTS_REQUIRE(ml_max <= cfg.gpt_max_mel_pos, "too many mel codes");
    std::vector<int> mids((size_t)B * ml_max, 8193);
    for (int b = 0; b < B; ++b) {
        int* r = mids.data() + (size_t)b * ml_max;
        r[0] = 8192;
        for (int k = 0; k < nn[b]; ++k) {
            const int c = codes_host[(size_t)b * n_max + k];
            DTTS_REQUIRE(c >= 0 && c < cfg.gpt_mel_codes, "mel code outside the mel_embedding table");
            r[1 + k] = c;
        }
        r[nn[b] + 1] = 8193;
    }
    ws().ensure(sizeof(float) * ((size_t)2 * B * C * L + (size_t)B * C) + prefill_ws(B, C, L) + sizeof(int) * mids.size() +
               (size_t)sizeof(float) * ((size_t)5 * B * (C / 2) * Tr + (size_t)B * C * Tr) + 65536 + extra_ws_bytes);
    float* emb = ws().f32((size_t)B * C * L);
    float* enc = ws().f32((size_t)B * C * L);
    float* enc_cond = ws().f32((size_t)B * C);
    int* d_mids = ws().i32(mids.size());
    DTTS_CHECK_HIP(hipMemcpyAsync(d_mids, mids.data(), sizeof(int) * mids.size(), hipMemcpyHostToDevice, s));
    DTTS_CHECK_HIP(hipStreamSynchronize(s));
    const float* cond = cond_in;
    if (!cond_in) {
        std::vector<int> rl(B);
        for (int b = 0; b < B; ++b) rl[b] = refer_lens_host ? refer_lens_host[b] : Tr;
        const int* d_rl = upload_ints(rl.data(), B, s);
        const size_t m = ws().mark();
        mel_style(gpt_cond_, refer, d_rl, rl.data(), B, Tr, enc_cond, s);
        ws().rewind(m);
        cond = enc_cond;
    }
    const int* d_ids = upload_ints(ids.data(), B * tl_max, s);
    const int* d_tl = upload_ints(tl.data(), B, s);
    const int* d_ml = upload_ints(ml.data(), B, s);
    const int* d_lt = upload_ints(lt.data(), B, s);
    DTTS_CHECK_HIP(hipMemsetAsync(emb, 0, sizeof(float) * (size_t)B * C * L, s));
    launch_build_prefix(cond, d_ids, tl_max, d_tl, text_emb_, text_pos_, mel_emb_, mel_pos_, d_mids, ml_max, d_ml, B, C, L, emb, s);
    GptAttnCapture cap;
    if (attn) {
        // the windows (model.h): HEADS the row's whole [lt_b, lt_b]; MEAN queries c0_b + j = the columns predicting code j, keys 1 .. tl_b
        cap.req = *attn;
        std::vector<int> q0(B), nq(B), k0(B), nk(B);
        for (int b = 0; b < B; ++b) {
            const bool heads = attn->mode == ATTN_PROBS_HEADS;
            q0[b] = heads ? 0 : 1 + tl[b];
            nq[b] = heads ? lt[b] : nn[b];
            k0[b] = heads ? 0 : 1;
            nk[b] = heads ? lt[b] : tl[b];
        }
        if (attn->mode == ATTN_PROBS_HEADS) {
            DTTS_REQUIRE(attn->nq_max >= L && attn->nk_max == attn->nq_max, "attention maps: the output's L is smaller than the longest row");
        } else {
            DTTS_REQUIRE(attn->nq_max == n_max && attn->nk_max == tl_max, "text alignment: output shape");
        }
        cap.q0 = upload_ints(q0.data(), B, s);
        cap.nq = upload_ints(nq.data(), B, s);
        cap.k0 = upload_ints(k0.data(), B, s);
        cap.nk = upload_ints(nk.data(), B, s);
        static_assert(sizeof(float) == sizeof(int), "the head weights travel through the int upload ring");
        if (attn->w) cap.w = reinterpret_cast<const float*>(upload_ints(reinterpret_cast<const int*>(attn->w), attn->n_layers * cfg.gpt_heads, s));
    }
    gpt_prefill_layers(emb, d_lt, B, L, nullptr, 0, 0, 0, s, attn ? &cap : nullptr);
    const long long bs = (long long)C * L;
    launch_ln_channels(emb, nullptr, bs, L, d_lt, L, B, C, lnf_g_, lnf_b_, 1e-5f, enc, bs, L, s);       // GPT2Model.ln_f
    launch_ln_channels(enc, nullptr, bs, L, d_lt, L, B, C, fin_g_, fin_b_, 1e-5f, emb, bs, L, s);       // final_norm (:403)
    f.enc = emb;
    f.L = L;
    return f;
}

// UnifiedVoice.forward(..., return_latent=True) as called at vqvae/model_24k.py:796-799.
// codes [B][n_max] host, n[b] valid -> latents_cm [B, C, lat_stride] (columns 0..n[b]-1)
void Model::gpt_latents(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host,
                        int Lt_max, const int* codes_host, const int* ncodes_host, int n_max, int B, float* latents_cm, int lat_stride,
                        hipStream_t s, const float* cond_in) {
    const int C = cfg.gpt_dim;
    const GptForced f = gpt_teacher_forced(refer, refer_lens_host, Tr, text_host, text_lens_host, Lt_max, codes_host, ncodes_host, n_max, B, 0, s, cond_in);
    std::vector<int> c0(B), nn(B);
    for (int b = 0; b < B; ++b) {
        c0[b] = 1 + f.tl[b];                                // column of the start_mel input
        nn[b] = f.ml[b] - 2;
    }
    const int* d_c0 = upload_ints(c0.data(), B, s);
    const int* d_nn = upload_ints(nn.data(), B, s);
    // enc[:, -(n+2):][:, :-2]  (:406, :481)
    hipLaunchKernelGGL(copy_columns_kernel, dim3(cdiv(n_max, 128) > 0 ? cdiv(n_max, 128) : 1, C, B), dim3(128), 0, s, f.enc, (long long)C * f.L,
                       f.L, d_c0, d_nn, C, latents_cm, (long long)C * lat_stride, lat_stride);
    DTTS_CHECK_HIP(hipGetLastError());
}

// `head` (mel_head / text_head as bound) fused with log-softmax + gather over the columns of lat (gpt_score.hip).  Rows run in groups of
// 16 (one targets table per group); everything is enqueued on s, nothing is allocated unless a call asks for more partials than the
// workspace sized at bind time holds.
void Model::score_head(const PackedConv& head, const float* lat, long long lat_bs, int lat_cs, const int* targets_host, const int* ntargets_host,
                       int n_max, int B, float* logprob_out, float* logits_out, hipStream_t s) {
    const int V = head.Cout;
    for (int g0 = 0; g0 < B; g0 += GEMV_MAXB) {
        const int nb = std::min(GEMV_MAXB, B - g0);
        std::vector<int> tg((size_t)nb * n_max, 0), tiles;
        for (int b = 0; b < nb; ++b) {
            const int nt = ntargets_host[g0 + b];
            std::copy(targets_host + (size_t)(g0 + b) * n_max, targets_host + (size_t)(g0 + b) * n_max + nt, tg.begin() + (size_t)b * n_max);
            for (int n0 = 0; n0 < nt; n0 += 128) { tiles.push_back(b); tiles.push_back(n0); }
        }
        const size_t need = sizeof(float) * gpt_score_part_floats(nb, n_max, head.CoutP) + 4096;
        if (need > gpt_score_ws_.capacity()) gpt_score_ws_.ensure(need);
        gpt_score_ws_.reset();
        ScoreParams p;
        p.lat = lat + (size_t)g0 * lat_bs;
        p.lat_bs = lat_bs;
        p.lat_cs = lat_cs;
        p.w = head.w;
        p.bias = head.b;
        p.C = head.Cin; p.CinP = head.CinP; p.V = V; p.CoutP = head.CoutP;
        p.targets = upload_ints(tg.data(), (int)tg.size(), s);
        p.ntargets = upload_ints(ntargets_host + g0, nb, s);
        p.tiles = upload_ints(tiles.data(), (int)tiles.size(), s);
        p.B = nb; p.n_max = n_max;
        p.part = gpt_score_ws_.f32(gpt_score_part_floats(nb, n_max, head.CoutP));
        p.out = logprob_out + (size_t)g0 * n_max;
        p.logits_out = logits_out ? logits_out + (size_t)g0 * V * n_max : nullptr;
        launch_gpt_score(p, (int)tiles.size() / 2, s);
    }
}

// gpt/model.py:408-415 (mel_head on final_norm's output) + log_softmax + gather, on latents the decode / the teacher-forced pass left:
// column k of latents_cm is the hidden state token k was drawn from, so logprob[b][k] = log p(targets[b][k]) under the UNPROCESSED
// distribution.
void Model::gpt_score(const float* latents_cm, int lat_stride, const int* targets_host, const int* ntargets_host, int n_max, int B,
                      float* logprob_out, float* logits_out, hipStream_t s) {
    DTTS_REQUIRE(bound_ && has_gpt_, "gpt weights not bound");
    DTTS_REQUIRE(B >= 0 && n_max >= 0, "gpt_score: B, n_max");
    if (B == 0 || n_max == 0) return;
    DTTS_REQUIRE(latents_cm && targets_host && ntargets_host && logprob_out, "gpt_score: null argument");
    DTTS_REQUIRE(n_max <= lat_stride, "gpt_score: n_max exceeds the latents' column stride");
    DTTS_REQUIRE(n_max <= 4096, "gpt_score: at most 4096 positions per row");
    const int C = cfg.gpt_dim, V = cfg.gpt_mel_codes;
    for (int b = 0; b < B; ++b) {
        DTTS_REQUIRE(ntargets_host[b] >= 0 && ntargets_host[b] <= n_max, "gpt_score: ntargets outside [0, n_max]");
        for (int k = 0; k < ntargets_host[b]; ++k) {
            const int t = targets_host[(size_t)b * n_max + k];
            DTTS_REQUIRE(t >= 0 && t < V, "gpt_score: target outside the mel_head's rows");
        }
    }
    score_head(mel_head_, latents_cm, (long long)C * lat_stride, lat_stride, targets_host, ntargets_host, n_max, B, logprob_out, logits_out, s);
}

// UnifiedVoice.forward's loss mode (gpt/model.py:429-491).  The reference has no attention mask and takes both cross-entropies as plain
// means over every position, so a batch is a rectangle: every row has the full Lt text ids and n mel codes (clip_inputs and
// set_mel_padding are host preprocessing of the caller, detail_tts_amd/gpt/model.py).  Inputs [cond | 255, text, 0 | 8192, codes, 8193];
// targets (build_aligned_inputs_and_targets, :372-375) [text, 0, 0] and [codes, 8193, 8193]; text logits from columns 1 .. Lt + 2 of
// final_norm's output, mel logits from its last n + 2 columns (:402-415) - both heads read the teacher-forced pass's own buffer.
void Model::gpt_forward_losses(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, int Lt, const int* codes_host, int n,
                               int B, float* losses_out, float* text_logprob, float* mel_logprob, float* mel_logits, hipStream_t s,
                               const float* cond_in) {
    DTTS_REQUIRE(bound_ && has_gpt_, "gpt weights not bound");
    DTTS_REQUIRE(has_text_head_, "gpt_forward_losses: gpt.text_head.weight is not bound (the checkpoint carries no text_head)");
    DTTS_REQUIRE(B >= 1 && Lt >= 0 && n >= 0, "gpt_forward_losses: B, Lt, n");
    DTTS_REQUIRE((refer || cond_in) && losses_out && text_host && codes_host, "gpt_forward_losses: null argument");
    DTTS_REQUIRE(Lt + 2 <= 4096 && n + 2 <= 4096, "gpt_forward_losses: at most 4096 positions per span (gpt_score's limit)");
    DTTS_REQUIRE(text_head_.Cout == cfg.gpt_text_tokens && text_head_.Cout > text_head_.CoutP - 128, "gpt_forward_losses: packed text_head shape");
    const int C = cfg.gpt_dim, nt = Lt + 2, nm = n + 2;
    const size_t lp_floats = (size_t)B * nt + (size_t)B * nm;
    // ids and codes are range-checked in here, before any launch
    const GptForced f = gpt_teacher_forced(refer, refer_lens_host, Tr, text_host, nullptr, Lt, codes_host, nullptr, n, B,
                                           sizeof(float) * lp_floats + 4 * 256, s, cond_in);
    if (!text_logprob) text_logprob = ws().f32((size_t)B * nt);
    if (!mel_logprob) mel_logprob = ws().f32((size_t)B * nm);
    std::vector<int> tt((size_t)B * nt, 0), tm((size_t)B * nm, 8193), ntt(B, nt), ntm(B, nm);
    for (int b = 0; b < B; ++b) {
        std::copy(text_host + (size_t)b * Lt, text_host + (size_t)(b + 1) * Lt, tt.begin() + (size_t)b * nt);
        std::copy(codes_host + (size_t)b * n, codes_host + (size_t)(b + 1) * n, tm.begin() + (size_t)b * nm);
    }
    const long long bs = (long long)C * f.L;
    score_head(text_head_, f.enc + 1, bs, f.L, tt.data(), ntt.data(), nt, B, text_logprob, nullptr, s);
    score_head(mel_head_, f.enc + (f.L - nm), bs, f.L, tm.data(), ntm.data(), nm, B, mel_logprob, mel_logits, s);
    launch_gpt_loss_means(text_logprob, B * nt, mel_logprob, B * nm, losses_out, s);
}

// ------------------------------------------------------------------------------------------ unit entries of the decode chain
// One launch each of the kernels gpt_step_launches strings together, on the caller's buffers (tests/test_gpu_gpt_decode.py).  The sizes
// of the buffers are the caller's (Runtime checks the tensors); what is checked here is every relation the launcher and the kernel
// rely on.  Nothing is uploaded or launched before the last check.  The launches are bracketed for the profiler (level 2).
void Model::op_gemv_block(int pro, const float* W, int K, int CoutP, const GemvIn& in, int B, float* part, GemvShape* shape, int* slices,
                          hipStream_t s) {
    DTTS_REQUIRE(pro == GP_PLAIN || pro == GP_RESSUM || pro == GP_LNPARTS || pro == GP_ATTN, "op_gemv_block: prologue 0 .. 3");
    DTTS_REQUIRE(W && part, "op_gemv_block: null argument");
    DTTS_REQUIRE(B >= 1 && B <= GEMV_MAXB, "op_gemv_block: 1 .. 16 batch rows");
    DTTS_REQUIRE(K >= 128 && K <= (1 << 16) && K % 128 == 0, "op_gemv_block: K must be a multiple of 128");
    DTTS_REQUIRE(CoutP >= 4 && CoutP <= (1 << 20) && CoutP % 4 == 0, "op_gemv_block: CoutP must be a multiple of 4");
    DTTS_REQUIRE((long long)gemv_block_slices(K, CoutP) * CoutP <= (long long)GEMV_PART_FLOATS, "op_gemv_block: partials beyond the per-row scratch");
    if (pro == GP_PLAIN || pro == GP_RESSUM) DTTS_REQUIRE(in.x && in.x_stride >= K, "op_gemv_block: x rows [B][x_stride >= K]");
    if (pro == GP_RESSUM) {
        DTTS_REQUIRE(in.gamma && in.y_out && in.stats_out, "op_gemv_block: the residual prologue needs gamma, y_out and stats_out");
        DTTS_REQUIRE(in.in_slices >= 0 && in.in_slices <= 64, "op_gemv_block: in_slices 0 .. 64");
        DTTS_REQUIRE(in.in_slices == 0 || (in.parts && in.in_stride >= K), "op_gemv_block: partials [in_slices][B][in_stride >= K]");
    }
    if (pro == GP_LNPARTS) {
        DTTS_REQUIRE(in.parts && in.stats_in && in.fold_c && in.fold_d, "op_gemv_block: the LayerNorm prologue needs parts, stats_in, fold_c and fold_d");
        DTTS_REQUIRE(in.in_slices >= 1 && in.in_slices <= 64 && in.in_stride >= K, "op_gemv_block: partials [in_slices in 1 .. 64][B][in_stride >= K]");
        DTTS_REQUIRE(in.stats_slices >= 1 && in.stats_slices <= 64 && in.K_ln >= 1, "op_gemv_block: statistics [stats_slices in 1 .. 64][B][2] over K_ln >= 1 values");
        DTTS_REQUIRE(in.in_act == ACT_NONE || in.in_act == ACT_GELU_NEW, "op_gemv_block: in_act is 0 or gelu_new");
    }
    if (pro == GP_ATTN) {
        DTTS_REQUIRE(in.parts && in.in_stride >= 1 && in.in_stride <= ATT_REC - 2 && K % in.in_stride == 0, "op_gemv_block: records of head dim in_stride, K = H in_stride");
        DTTS_REQUIRE(in.in_slices >= 1 && in.in_slices <= 8, "op_gemv_block: 1 .. 8 key splits");
    }
    // ---- nothing has been launched up to here
    const GemvShape g = gemv_block_shape(K, CoutP, B);
    if (shape) *shape = g;
    if (slices) *slices = gemv_block_slices(K, CoutP);
    static const char* tags[3][2] = {{"gemv_block_kernel<1,8,8>", "gemv_block_kernel<1,8,16>"},
                                     {"gemv_block_kernel<1,16,8>", "gemv_block_kernel<1,16,16>"},
                                     {"gemv_block_kernel<4,16,8>", "gemv_block_kernel<4,16,16>"}};
    ProfScope ps(tags[g.vec == 4 ? 2 : (g.rpw == 16 ? 1 : 0)][g.nb == 16 ? 1 : 0], 0.0, 4.0 * K * CoutP, s);
    launch_gemv_block(pro, W, K, CoutP, in, B, part, s);
}

void Model::op_decode_attention(const float* part, int slices, int CoutP, const float* stats, int stats_slices, const float* fold_c,
                                const float* fold_d, float* cache, long long cache_bs, int cap, const int* lp_host, const int* step_host,
                                int B, int H, int D, int ksplit, const float* wproj, int wpCoutP, float* out, hipStream_t s) {
    DTTS_REQUIRE(part && stats && fold_c && fold_d && cache && lp_host && step_host && out, "op_decode_attention: null argument");
    DTTS_REQUIRE(D == 48, "op_decode_attention: head dim 48 is the only instantiation");
    DTTS_REQUIRE(B >= 1 && B <= GEMV_MAXB && H >= 1 && H <= 64, "op_decode_attention: 1 .. 16 rows, 1 .. 64 heads");
    DTTS_REQUIRE(slices >= 1 && slices <= 64 && stats_slices >= 1 && stats_slices <= 64, "op_decode_attention: slice counts 1 .. 64");
    DTTS_REQUIRE(CoutP >= 3 * H * D && CoutP <= (1 << 20), "op_decode_attention: the qkv partials need 3 H D columns");
    DTTS_REQUIRE(ksplit >= 0 && ksplit <= 8, "op_decode_attention: key splits 1 .. 8 (0: the process default)");
    DTTS_REQUIRE(cap >= 1 && decode_attention_fits(cap, wproj != nullptr), "op_decode_attention: cap beyond the LDS score buffer");
    DTTS_REQUIRE(cache_bs >= (long long)2 * H * D * cap, "op_decode_attention: a row's cache is K [C][cap] | V [cap][C]");
    if (wproj) DTTS_REQUIRE(wpCoutP == 768 && H * D <= 768 && ksplit == 0, "op_decode_attention: the fused projection is 768 columns wide and takes no key split");
    for (int b = 0; b < B; ++b)
        DTTS_REQUIRE(lp_host[b] >= 0 && step_host[b] >= 0 && lp_host[b] + step_host[b] >= 1 && (long long)lp_host[b] + step_host[b] <= cap,
                     "op_decode_attention: 1 <= lp + step <= cap for every row");
    // ---- nothing has been launched or uploaded up to here
    GptCtl c;
    std::memset(&c, 0, sizeof(c));
    for (int b = 0; b < B; ++b) { c.lp[b] = lp_host[b]; c.step[b] = step_host[b]; }
    static_assert(sizeof(GptCtl) % sizeof(int) == 0, "the control block travels through the int upload ring");
    const GptCtl* ctl = reinterpret_cast<const GptCtl*>(upload_ints(reinterpret_cast<const int*>(&c), (int)(sizeof(GptCtl) / sizeof(int)), s));
    ProfScope ps(wproj ? "decode_attention_qkv_kernel<48,proj>" : "decode_attention_qkv_kernel<48,split>", 0.0, 8.0 * B * H * D * cap, s);
    launch_decode_attention_qkv(part, slices, CoutP, stats, stats_slices, fold_c, fold_d, cache, cache_bs, cap, ctl, B, H, D, out, s, wproj,
                                wpCoutP, ksplit);
}

void Model::op_gpt_final_ln(const float* res, const float* bias, const float* parts, int in_slices, int in_stride, int B, const float* g1,
                            const float* b1, const float* g2, const float* b2, float* y, int C, const int* step_host, int max_steps,
                            float* latents, int lat_cs, hipStream_t s) {
    DTTS_REQUIRE(res && g1 && b1 && g2 && b2 && y && step_host, "op_gpt_final_ln: null argument");
    DTTS_REQUIRE(C >= 1 && C <= 1024, "op_gpt_final_ln: width 1 .. 1024");
    DTTS_REQUIRE(B >= 1 && B <= GEMV_MAXB, "op_gpt_final_ln: 1 .. 16 rows");
    DTTS_REQUIRE(in_slices >= 0 && in_slices <= 64, "op_gpt_final_ln: in_slices 0 .. 64");
    DTTS_REQUIRE(in_slices == 0 || (parts && in_stride >= C), "op_gpt_final_ln: partials [in_slices][B][in_stride >= C]");
    DTTS_REQUIRE(!latents || lat_cs >= 1, "op_gpt_final_ln: latents [B][C][lat_cs]");
    for (int b = 0; b < B; ++b)
        DTTS_REQUIRE(step_host[b] >= 0 && (!latents || step_host[b] >= max_steps || step_host[b] < lat_cs),
                     "op_gpt_final_ln: a step below max_steps must be a column of latents");
    // ---- nothing has been launched or uploaded up to here
    GptCtl c;
    std::memset(&c, 0, sizeof(c));
    for (int b = 0; b < B; ++b) c.step[b] = step_host[b];
    c.max_steps = max_steps;
    c.latents = latents;
    c.lat_bs = (long long)C * lat_cs;
    c.lat_cs = lat_cs;
    const GptCtl* ctl = reinterpret_cast<const GptCtl*>(upload_ints(reinterpret_cast<const int*>(&c), (int)(sizeof(GptCtl) / sizeof(int)), s));
    ProfScope ps("gpt_final_ln_kernel", 0.0, 8.0 * B * C, s);
    launch_gpt_final_ln(res, bias, parts, in_slices, in_stride, B, g1, b1, g2, b2, y, C, ctl, s);
}

void Model::op_ln_fold_vectors(const float* W, int K, int CoutP, const float* gamma, const float* beta, const float* bias, float* c, float* d,
                               hipStream_t s) {
    DTTS_REQUIRE(W && gamma && beta && c && d, "op_ln_fold_vectors: null argument");
    DTTS_REQUIRE(K >= 1 && K <= (1 << 16) && CoutP >= 1 && CoutP <= (1 << 20), "op_ln_fold_vectors: sizes");
    ProfScope ps("ln_fold_vectors_kernel", 0.0, 4.0 * K * CoutP, s);
    launch_ln_fold_vectors(W, K, CoutP, gamma, beta, bias, c, d, s);
}

void Model::op_kv_to_cache(const float* qkv, const int* lens_host, int B, int C, int L, float* cache, long long cache_bs, int cap,
                           hipStream_t s) {
    DTTS_REQUIRE(qkv && lens_host && cache, "op_kv_to_cache: null argument");
    DTTS_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && 2 * C <= 65535 && L >= 1 && L <= (1 << 20) && cap >= 1 && cap <= (1 << 20), "op_kv_to_cache: sizes");
    DTTS_REQUIRE(cache_bs >= (long long)2 * C * cap, "op_kv_to_cache: a row's cache is K [C][cap] | V [cap][C]");
    for (int b = 0; b < B; ++b) DTTS_REQUIRE(lens_host[b] >= 0 && lens_host[b] <= L && lens_host[b] <= cap, "op_kv_to_cache: lengths must lie in [0, min(L, cap)]");
    // ---- nothing has been launched or uploaded up to here
    const int* dl = upload_ints(lens_host, B, s);
    ProfScope ps("kv_to_cache_kernel", 0.0, 16.0 * B * C * L, s);
    launch_kv_to_cache(qkv, (long long)3 * C * L, L, dl, L, B, C, cache, cache_bs, cap, s);
}

}  // namespace dtts
