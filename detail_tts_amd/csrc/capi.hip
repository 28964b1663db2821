// extern "C" surface of libdetail_hip.so (see include/detail_hip.h).
#include <algorithm>
#include <mutex>

#include "model.h"
#include "prof.h"

using dtts::Model;

struct dtts_handle {
    std::unique_ptr<Model> m;
};

// last error of the CALLING thread (a handle may be driven by two threads: stage A of the next request beside stages B / C of this one)
static thread_local std::string t_err;

static std::string g_create_error;
static std::mutex g_create_mu;

#define DTTS_API_BEGIN try {
#define DTTS_API_END(h)                                   \
    }                                                     \
    catch (const dtts::Error& e) {                        \
        t_err = e.what();                                 \
        return e.code;                                    \
    }                                                     \
    catch (const std::exception& e) {                     \
        t_err = e.what();                                 \
        return -100;                                      \
    }                                                     \
    return 0;

extern "C" {

const char* dtts_version(void) { return "detail_hip 0.1 (gfx950)"; }

void dtts_default_config(dtts_config* c) {
    std::memset(c, 0, sizeof(*c));
    c->diff_channels = 768; c->diff_layers = 10; c->diff_heads = 16; c->mel_channels = 128; c->diff_out_channels = 256;
    c->diff_steps = 50; c->diff_trained_steps = 4000; c->cond_free_k = 2.0f;
    c->gpt_dim = 768; c->gpt_layers = 10; c->gpt_heads = 16; c->gpt_mel_codes = 8194; c->gpt_text_tokens = 257;
    c->gpt_max_mel_pos = 1603; c->gpt_max_text_pos = 802;
    c->inter_channels = 192; c->hidden_channels = 192; c->filter_channels = 512; c->enc_heads = 4; c->enc_layers = 3;
    c->gin_channels = 768; c->upsample_initial_channel = 400; c->n_upsamples = 5;
    const int rates[5] = {8, 4, 2, 2, 2}, kern[5] = {16, 8, 2, 2, 2};
    for (int i = 0; i < 5; ++i) { c->upsample_rates[i] = rates[i]; c->upsample_kernels[i] = kern[i]; }
    c->n_resblock_kernels = 3;
    const int rk[3] = {3, 7, 11}, rd[3] = {1, 3, 5};
    for (int i = 0; i < 3; ++i) { c->resblock_kernels[i] = rk[i]; c->resblock_dilations[i] = rd[i]; }
}

int dtts_op_resblock1(dtts_handle* h, int stage, int branch, const float* x, const int* lens, int B, int T, float* y, void* stream) {
    DTTS_API_BEGIN
    h->m->op_resblock1(stage, branch, x, lens, B, T, y, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_wn(dtts_handle* h, int flow, const float* hidden, const float* g, const int* lens, int B, int T, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->op_wn(flow, hidden, g, lens, B, T, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_enc_p(dtts_handle* h, const float* mel, const int* lens, int B, int T, float* m_p, float* logs_p, void* stream) {
    DTTS_API_BEGIN
    h->m->op_enc_p(mel, lens, B, T, m_p, logs_p, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_posterior_encode(dtts_handle* h, const float* spec, int spec_channels, const int* lens, const float* g, int B, int T,
                          const float* noise, unsigned long long seed, const int* sample_ids, float* z, float* m_q, float* logs_q, void* stream) {
    DTTS_API_BEGIN
    h->m->posterior_encode(spec, spec_channels, lens, g, B, T, noise, seed, sample_ids, z, m_q, logs_q, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_flow_forward(dtts_handle* h, const float* z, const float* g, const int* lens, int B, int T, float* z_p, void* stream) {
    DTTS_API_BEGIN
    h->m->flow_forward(z, g, lens, B, T, z_p, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_slice_segments(dtts_handle* h, const float* x, const int* ids, int B, int C, int T, int seg, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->slice_segments(x, ids, B, C, T, seg, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_kl_loss(dtts_handle* h, const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, const int* lens, int B, int C,
                 int T, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->kl_loss(z_p, logs_q, m_p, logs_p, lens, B, C, T, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_flowvae_forward(dtts_handle* h, const float* mel, const float* spec, int spec_channels, const int* lens, int B, int T,
                         const float* noise, unsigned long long seed, const int* sample_ids, const int* ids_slice, int seg, float* o,
                         float* z, float* z_p, float* m_p, float* logs_p, float* m_q, float* logs_q, float* quantized, void* stream) {
    DTTS_API_BEGIN
    h->m->flowvae_forward(mel, spec, spec_channels, lens, B, T, noise, seed, sample_ids, ids_slice, seg, o, z, z_p, m_p, logs_p, m_q, logs_q,
                          quantized, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_bind_discriminator(dtts_handle* h, const void* blob, size_t nbytes, const char* const* names, const unsigned long long* offsets,
                            const unsigned long long* numels, int n, void* stream) {
    DTTS_API_BEGIN
    h->m->bind_discriminator(blob, nbytes, names, offsets, numels, n, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_disc_layout(int N, int t, long long* offsets, int* dims) {
    DTTS_API_BEGIN
    if (!offsets || !dims || N < 1 || t < 12) throw dtts::Error(-1, "dtts_disc_layout: N >= 1, t >= 12 and two output arrays");
    const dtts::DiscLayout L = dtts::disc_layout(N, t);
    for (int m = 0; m < DTTS_DISC_MAPS; ++m) {
        offsets[m] = L.off[m];
        dims[4 * m] = L.C[m]; dims[4 * m + 1] = L.H[m]; dims[4 * m + 2] = L.p[m]; dims[4 * m + 3] = N;
    }
    offsets[DTTS_DISC_MAPS] = L.off[DTTS_DISC_MAPS];
    DTTS_API_END(nullptr)
}

int dtts_disc_forward(dtts_handle* h, const float* y, const float* y_hat, int B, int t, float* maps, void* stream) {
    DTTS_API_BEGIN
    h->m->disc_forward(y, y_hat, B, t, maps, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_disc_losses(dtts_handle* h, int n_maps, const float* const* r, const float* const* g, const long long* map_numel, int n_scores,
                     const float* const* dr, const float* const* dg, const long long* score_numel, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->disc_losses(n_maps, r, g, map_numel, n_scores, dr, dg, score_numel, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_spec_to_mel(dtts_handle* h, const float* spec, int B, int spec_channels, int T, float* mel_out, void* stream) {
    DTTS_API_BEGIN
    h->m->spec_to_mel(spec, B, spec_channels, T, mel_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_conv1d_grouped(dtts_handle* h, const float* x, const float* w, const float* bias, int B, int Cin, int Tin, int Cout, int groups,
                           int K, int stride, int pad, float slope, float* y, void* stream) {
    DTTS_API_BEGIN
    h->m->op_conv1d_grouped(x, w, bias, B, Cin, Tin, Cout, groups, K, stride, pad, slope, y, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_period_split(dtts_handle* h, const float* wav, int B, int t, int p, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->op_period_split(wav, B, t, p, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

long long dtts_flowvae_stage_work(int B, int T, int seg, int hop) {
    if (B < 1 || T < 1 || seg < 1 || hop < 1 || (long long)seg * hop < 12) return -1;
    return dtts::flowvae_stage_work_floats(B, T, seg, hop);
}

int dtts_flowvae_stage_losses(dtts_handle* h, const float* mel, const float* spec, int spec_channels, const int* lens, int B, int T,
                              const float* noise, unsigned long long seed, const int* sample_ids, const int* ids_slice, int seg,
                              const float* wav, int L, float* o, float* z, float* z_p, float* m_p, float* logs_p, float* m_q, float* logs_q,
                              float* quantized, float* work, float* losses, void* stream) {
    DTTS_API_BEGIN
    h->m->flowvae_stage_losses(mel, spec, spec_channels, lens, B, T, noise, seed, sample_ids, ids_slice, seg, wav, L, o, z, z_p, m_p, logs_p,
                               m_q, logs_q, quantized, work, losses, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_vq_decode(dtts_handle* h, const int* codes, const int* ncodes, int nmax, const float* refer, const int* refer_lens, int Tr,
                   int B, float* mel_out, void* stream) {
    DTTS_API_BEGIN
    h->m->vq_decode(codes, ncodes, nmax, refer, refer_lens, Tr, B, mel_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_vq_encode(dtts_handle* h, const float* mel, const int* lens, int B, int T, int* codes, float* x_vq, void* stream) {
    DTTS_API_BEGIN
    h->m->vq_encode(mel, lens, B, T, codes, x_vq, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_resample(dtts_handle* h, const float* x, int B, int L, const float* kernel, int orig, int neu, int width, float* y, int Lout,
                  void* stream) {
    DTTS_API_BEGIN
    h->m->resample(x, B, L, kernel, orig, neu, width, y, Lout, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_mel_spectrogram(dtts_handle* h, const float* wav, const int* lens, int B, int L, int n_fft, int hop, float* mel_out, int Tmax,
                         void* stream) {
    DTTS_API_BEGIN
    h->m->mel_spectrogram(wav, lens, B, L, n_fft, hop, mel_out, Tmax, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_spectrogram(dtts_handle* h, const float* wav, const int* lens, int B, int L, int n_fft, int hop, float* spec_out, int Tmax,
                     void* stream) {
    DTTS_API_BEGIN
    if (!spec_out) throw dtts::Error(-2, "dtts_spectrogram: spec_out is null");
    h->m->mel_spectrogram(wav, lens, B, L, n_fft, hop, nullptr, Tmax, (hipStream_t)stream, spec_out);
    DTTS_API_END(h)
}

int dtts_set_option(dtts_handle* h, const char* key, int value) {
    DTTS_API_BEGIN
    h->m->set_option(key, value);
    DTTS_API_END(h)
}

int dtts_uncond_cache_stats(dtts_handle* h, unsigned long long* out) {
    DTTS_API_BEGIN
    if (!out) throw dtts::Error(-2, "dtts_uncond_cache_stats: out is null");
    const dtts::UncondCacheStats st = h->m->uncond_cache_stats();
    out[0] = st.entries; out[1] = st.bytes; out[2] = st.hits; out[3] = st.misses; out[4] = st.bypasses; out[5] = st.evictions;
    DTTS_API_END(h)
}

int dtts_get_option(dtts_handle* h, const char* key, int* value) {
    DTTS_API_BEGIN
    if (!value) throw dtts::Error(-2, "dtts_get_option: value is null");
    *value = h->m->get_option(key);
    DTTS_API_END(h)
}

long long dtts_vocoder_ticket(dtts_handle* h) { return h && h->m ? h->m->vocoder_ticket() : 0; }
int dtts_vocoder_check_active(dtts_handle* h) { return h && h->m && h->m->vocoder_check_active() ? 1 : 0; }

int dtts_vocoder_check(dtts_handle* h, long long ticket) {
    DTTS_API_BEGIN
    h->m->vocoder_check(ticket);
    DTTS_API_END(h)
}

int dtts_profile_enable(int on) {
    dtts::Profiler::get().reset();
    dtts::Profiler::get().on = on != 0;
    dtts::Profiler::get().all = on >= 2;
    if (on) dtts::Profiler::get().reserve(1 << 16);
    return 0;
}

int dtts_profile_sampling(int every) {
    dtts::Profiler::get().step_every = every < 1 ? 1 : every;
    return 0;
}

int dtts_profile_report(dtts_kernel_stat* out, int max_entries) {
    auto v = dtts::Profiler::get().report();
    int n = 0;
    for (auto& st : v) {
        if (n >= max_entries) break;
        std::memset(&out[n], 0, sizeof(out[n]));
        std::strncpy(out[n].name, st.name.c_str(), sizeof(out[n].name) - 1);
        out[n].launches = st.launches;
        out[n].total_ms = st.ms;
        out[n].union_ms = st.union_ms;
        out[n].flops = st.flops;
        out[n].bytes = st.bytes;
        ++n;
    }
    return n;
}

int dtts_create(dtts_handle** out, const dtts_config* cfg, int device) {
    if (!out || !cfg) return -1;
    *out = nullptr;
    try {
        auto* h = new dtts_handle();
        h->m.reset(new Model(*cfg, device));
        *out = h;
    } catch (const std::exception& e) {
        std::lock_guard<std::mutex> lk(g_create_mu);
        g_create_error = e.what();
        return -2;
    }
    return 0;
}

int dtts_destroy(dtts_handle* h) {
    delete h;
    return 0;
}

const char* dtts_last_error(dtts_handle* h) { return h ? t_err.c_str() : g_create_error.c_str(); }

int dtts_bind_weights(dtts_handle* h, const void* blob, size_t nbytes, const char* const* names, const unsigned long long* offsets,
                      const unsigned long long* numels, int n, void* stream) {
    DTTS_API_BEGIN
    h->m->bind_weights(blob, nbytes, names, offsets, numels, n, (hipStream_t)stream);
    DTTS_API_END(h)
}

void dtts_gpt_options_init(dtts_gpt_options* o) {
    if (!o) return;
    *o = dtts_gpt_options{};
    o->struct_size = sizeof(dtts_gpt_options);
    o->max_generate_length = 600;
    o->top_k = 50;
    o->top_p = 0.8f;
    o->temperature = 0.8f;
    o->repetition_penalty = 2.0f;
    o->length_penalty = 1.0f;
}

// HF's remaining logits processors: the ranges their constructors accept (0 / NULL = off); NaN fails every range
static void check_gpt_processors(const dtts_gpt_options* o, int V) {
    DTTS_REQUIRE(o->no_repeat_ngram_size >= 0 && o->no_repeat_ngram_size <= dtts::SAMP_NGRAM_MAX, "options: no_repeat_ngram_size outside 0 .. 16 (0 = off)");
    DTTS_REQUIRE(o->min_length >= 0 && o->min_new_tokens >= 0, "options: min_length / min_new_tokens negative");
    DTTS_REQUIRE(o->exp_decay_factor == 0.0 || (o->exp_decay_factor > 1.0 && o->exp_decay_factor < (double)INFINITY && o->exp_decay_start >= 0),
                 "options: exp_decay_factor is 0 (off) or > 1 with exp_decay_start >= 0");
    DTTS_REQUIRE(o->n_suppress_tokens >= 0 && o->n_begin_suppress_tokens >= 0 && (o->n_suppress_tokens == 0 || o->suppress_tokens) &&
                     (o->n_begin_suppress_tokens == 0 || o->begin_suppress_tokens), "options: suppress_tokens / begin_suppress_tokens list without ids");
    for (int i = 0; i < o->n_suppress_tokens; ++i)
        DTTS_REQUIRE(o->suppress_tokens[i] >= 0 && o->suppress_tokens[i] < V, "options: suppress_tokens id outside the vocabulary");
    for (int i = 0; i < o->n_begin_suppress_tokens; ++i)
        DTTS_REQUIRE(o->begin_suppress_tokens[i] >= 0 && o->begin_suppress_tokens[i] < V, "options: begin_suppress_tokens id outside the vocabulary");
    DTTS_REQUIRE(o->min_p >= 0.f && o->min_p <= 1.f, "options: min_p outside [0, 1] (0 = off)");
    DTTS_REQUIRE(o->epsilon_cutoff >= 0.f && o->epsilon_cutoff < 1.f, "options: epsilon_cutoff outside [0, 1) (0 = off)");
}

// beam search (num_beams 0 / 1 = off): what may not be combined with it is refused here, before any launch
static void check_gpt_beams(const dtts_gpt_options* o) {
    DTTS_REQUIRE(o->num_beams >= 0 && o->num_beams <= dtts::BEAM_MAXK, "options: num_beams outside 0 .. 16 (a session holds 16 rows)");
    DTTS_REQUIRE(o->early_stopping >= 0 && o->early_stopping <= 2, "options: early_stopping is 0 (False), 1 (True) or 2 (\"never\")");
    DTTS_REQUIRE(o->length_penalty > -INFINITY && o->length_penalty < INFINITY, "options: length_penalty is not finite");
    if (o->num_beams > 1) {
        DTTS_REQUIRE(!o->forced_codes, "options: num_beams with forced_codes (input_tokens under beams is not served)");
        DTTS_REQUIRE(!o->forced_uniforms, "options: num_beams with forced_uniforms (beam search draws nothing)");
        DTTS_REQUIRE(!(o->typical_mass > 0.f && o->typical_mass < 1.f), "options: num_beams with typical sampling (beam-sample is not served)");
    }
}

// the sampling fields every row of a session has: the scalar fields of a uniform session, or one row's record written into them
static void check_gpt_sampling(const dtts_gpt_options* o, int V) {
    DTTS_REQUIRE(o->typical_mass >= 0.f && o->typical_mass <= 1.f, "options: typical_mass outside [0, 1] (0 = off)");      // NaN fails both
    DTTS_REQUIRE(o->temperature > 0.f && o->temperature < INFINITY && o->top_p >= 0.f && o->top_p <= 1.f && o->repetition_penalty > 0.f &&
                     o->repetition_penalty < INFINITY, "options: temperature / top_p / repetition_penalty out of range");
    check_gpt_processors(o, V);
}

// dtts_gpt_options.row_options: every row passes the checks the scalar fields get, before any launch; the error names the row
static void check_gpt_rows(const dtts_gpt_options* o, int B, int V, bool caps) {
    DTTS_REQUIRE(B >= 1, "options: row_options needs the row count");
    DTTS_REQUIRE(o->num_beams <= 1, "options: row_options with num_beams > 1 (a beam session is uniform)");
    int cap_max = 0;
    for (int b = 0; b < B; ++b) {
        const dtts_gpt_row_options& r = o->row_options[b];
        dtts_gpt_options t = *o;
        t.temperature = r.temperature; t.top_p = r.top_p; t.repetition_penalty = r.repetition_penalty; t.typical_mass = r.typical_mass;
        t.min_p = r.min_p; t.epsilon_cutoff = r.epsilon_cutoff; t.top_k = r.top_k;
        t.no_repeat_ngram_size = r.no_repeat_ngram_size; t.min_length = r.min_length; t.min_new_tokens = r.min_new_tokens;
        t.exp_decay_start = r.exp_decay_start; t.exp_decay_factor = r.exp_decay_factor;
        t.suppress_tokens = r.suppress_tokens; t.n_suppress_tokens = r.n_suppress_tokens;
        t.begin_suppress_tokens = r.begin_suppress_tokens; t.n_begin_suppress_tokens = r.n_begin_suppress_tokens;
        try {
            check_gpt_sampling(&t, V);
            if (caps)
                DTTS_REQUIRE(r.max_generate_length >= 1 && r.max_generate_length <= o->max_generate_length,
                             "row_options: max_generate_length outside 1 .. the call's max_generate_length");
        } catch (const dtts::Error& e) {
            throw dtts::Error(e.code, "row_options[" + std::to_string(b) + "]: " + e.what());
        }
        cap_max = std::max(cap_max, r.max_generate_length);
    }
    if (caps) DTTS_REQUIRE(cap_max == o->max_generate_length, "options: max_generate_length has to equal the largest row_options[].max_generate_length");
}

static void check_gpt_options(const dtts_gpt_options* o, int B) {
    DTTS_REQUIRE(o, "options");
    DTTS_REQUIRE(o->struct_size == sizeof(dtts_gpt_options),
                 "dtts_gpt_options.struct_size does not match this library's layout: start from dtts_gpt_options_init() (built against another include/detail_hip.h?)");
    DTTS_REQUIRE(o->sample_ids, "options: sample_ids");
    DTTS_REQUIRE(o->token_wgs == 0 || o->token_wgs == 128 || o->token_wgs == 64 || o->token_wgs == 32, "options: token_wgs is 0 (the handle's option), 128, 64 or 32");
    DTTS_REQUIRE(o->prompt_codes || !o->prompt_lens, "options: prompt_lens without prompt_codes");
    DTTS_REQUIRE(!o->prompt_codes || (o->prompt_lens && o->prompt_stride >= 0), "options: prompt_codes needs prompt_lens and prompt_stride >= 0");
    if (o->row_options) check_gpt_rows(o, B, 8194, true);
    else check_gpt_sampling(o, 8194);
    check_gpt_beams(o);
}

int dtts_gpt_generate(dtts_handle* h, const float* refer, const int* refer_lens, int Tr, const int* text, const int* text_lens,
                      int Lt_max, int B, const dtts_gpt_options* opts, int* codes_out, int* ncodes_out, float* latents_cm,
                      int lat_stride, void* stream) {
    DTTS_API_BEGIN
    check_gpt_options(opts, B);
    h->m->gpt_generate(refer, refer_lens, Tr, text, text_lens, Lt_max, B, *opts, codes_out, ncodes_out, latents_cm, lat_stride,
                       (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_prefill(dtts_handle* h, const float* refer, const int* refer_lens, int Tr, const int* text, const int* text_lens,
                     int Lt_max, int B, const dtts_gpt_options* opts, float* latents_cm, int lat_stride, void* stream) {
    DTTS_API_BEGIN
    check_gpt_options(opts, B);
    h->m->gpt_prefill(refer, refer_lens, Tr, text, text_lens, Lt_max, B, *opts, latents_cm, lat_stride, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_beam_generate(dtts_handle* h, const float* refer, const int* refer_lens, int Tr, const int* text, const int* text_lens,
                           int Lt_max, int B, const dtts_gpt_options* opts, int nrs, int* seqs_out, int* lens_out, float* scores_out,
                           void* stream) {
    DTTS_API_BEGIN
    check_gpt_options(opts, B);
    DTTS_REQUIRE(opts->num_beams > 1, "dtts_gpt_beam_generate: options.num_beams has to be 2 .. 16");
    DTTS_REQUIRE(nrs >= 1 && nrs <= opts->num_beams, "dtts_gpt_beam_generate: num_return_sequences outside 1 .. num_beams");
    DTTS_REQUIRE(seqs_out && lens_out && scores_out, "dtts_gpt_beam_generate: null output");
    h->m->gpt_beam_generate(refer, refer_lens, Tr, text, text_lens, Lt_max, B, *opts, nrs, seqs_out, lens_out, scores_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_beam_finish(dtts_handle* h, int nrs, int* seqs_out, int* lens_out, float* scores_out, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(seqs_out && lens_out && scores_out, "dtts_gpt_beam_finish: null output");
    h->m->gpt_beam_finish(nrs, seqs_out, lens_out, scores_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_beam_step(dtts_handle* h, const float* logits, int U, int V, const dtts_gpt_options* opts, int step, const int* prompt,
                      int prompt_len, int* run_seq, float* run_score, int* fin_seq, float* fin_score, int* fin_flag, int* fin_len,
                      int* unsat, int* done, int* parents, int* tokens, float* cand_score, int* cand_beam, int* cand_tok, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(opts, "options");
    DTTS_REQUIRE(opts->struct_size == sizeof(dtts_gpt_options),
                 "dtts_gpt_options.struct_size does not match this library's layout: start from dtts_gpt_options_init()");
    DTTS_REQUIRE(opts->repetition_penalty > 0.f && opts->repetition_penalty < INFINITY, "options: repetition_penalty out of range");
    DTTS_REQUIRE(V >= 2 && V <= dtts::BEAM_V_MAX, "op_beam_step: vocabulary outside 2 .. 12288");
    check_gpt_processors(opts, V);
    check_gpt_beams(opts);
    DTTS_REQUIRE(opts->num_beams >= 1, "op_beam_step: options.num_beams has to be 1 .. 16");
    DTTS_REQUIRE(!opts->row_options, "op_beam_step: row_options (a beam session is uniform)");
    h->m->op_beam_step(logits, U, V, *opts, step, prompt, prompt_len, run_seq, run_score, fin_seq, fin_score, fin_flag, fin_len, unsat, done,
                       parents, tokens, cand_score, cand_beam, cand_tok, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_decode_step(dtts_handle* h, void* stream) {
    DTTS_API_BEGIN
    h->m->gpt_decode_step((hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_decode(dtts_handle* h, int n_steps, int* n_done, void* stream) {
    DTTS_API_BEGIN
    const int n = h->m->gpt_decode(n_steps, (hipStream_t)stream);
    if (n_done) *n_done = n;
    DTTS_API_END(h)
}

int dtts_gpt_steps(dtts_handle* h) { return h ? h->m->gpt_steps() : 0; }

int dtts_gpt_all_finished(dtts_handle* h, int* all_finished, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(all_finished, "all_finished");
    *all_finished = h->m->gpt_all_finished((hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_finish(dtts_handle* h, int* codes_out, int* ncodes_out, void* stream) {
    DTTS_API_BEGIN
    h->m->gpt_finish(codes_out, ncodes_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_sample_logits(dtts_handle* h, const float* logits, int R, int V, const int* history, int hist_len, const float* uniforms,
                          int top_k, float top_p, float temperature, float repetition_penalty, int* tokens_out, void* stream) {
    return dtts_op_sample_logits_ex(h, logits, R, V, history, hist_len, uniforms, top_k, top_p, temperature, repetition_penalty, 0.f, 0,
                                    tokens_out, stream);
}

int dtts_op_sample_logits_ex(dtts_handle* h, const float* logits, int R, int V, const int* history, int hist_len, const float* uniforms,
                             int top_k, float top_p, float temperature, float repetition_penalty, float typical_mass, int suppress_eos,
                             int* tokens_out, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(typical_mass >= 0.f && typical_mass <= 1.f, "op_sample_logits: typical_mass outside [0, 1] (0 = off)");      // NaN fails both
    h->m->op_sample_logits(logits, R, V, history, hist_len, uniforms, top_k, top_p, temperature, repetition_penalty, typical_mass,
                           suppress_eos, tokens_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_sample_logits_opts(dtts_handle* h, const float* logits, int R, int V, const dtts_gpt_options* opts, const int* history,
                               int hist_stride, const int* hist_lens, const int* fills, const int* prompt_lens, const float* uniforms,
                               int* tokens_out, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(opts, "options");
    DTTS_REQUIRE(opts->struct_size == sizeof(dtts_gpt_options),
                 "dtts_gpt_options.struct_size does not match this library's layout: start from dtts_gpt_options_init()");
    DTTS_REQUIRE(opts->typical_mass >= 0.f && opts->typical_mass <= 1.f, "op_sample_logits_opts: typical_mass outside [0, 1] (0 = off)");
    DTTS_REQUIRE(opts->temperature > 0.f && opts->temperature < INFINITY && opts->top_p >= 0.f && opts->top_p <= 1.f &&
                     opts->repetition_penalty > 0.f && opts->repetition_penalty < INFINITY, "options: temperature / top_p / repetition_penalty out of range");
    check_gpt_processors(opts, V);
    if (opts->row_options) {                         // (the scalar fields are then not read: every row gets the checks they get)
        DTTS_REQUIRE(R >= 1 && R <= dtts::GEMV_MAXB, "op_sample_logits_opts: rows 1..16");
        DTTS_REQUIRE(opts->num_beams <= 1, "op_sample_logits_opts: row_options with num_beams > 1");
        check_gpt_rows(opts, R, V, false);
    }
    h->m->op_sample_logits_opts(logits, R, V, *opts, history, hist_stride, hist_lens, fills, prompt_lens, uniforms, tokens_out,
                                (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_sample_logits_rows(dtts_handle* h, const float* logits, int R, int V, const dtts_gpt_options* opts,
                               const dtts_gpt_row_options* rows, const int* history, int hist_stride, const int* hist_lens, const int* fills,
                               const int* prompt_lens, const float* uniforms, int* tokens_out, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(opts && rows, "op_sample_logits_rows: options / rows");
    DTTS_REQUIRE(opts->struct_size == sizeof(dtts_gpt_options),
                 "dtts_gpt_options.struct_size does not match this library's layout: start from dtts_gpt_options_init()");
    DTTS_REQUIRE(R >= 1 && R <= dtts::GEMV_MAXB, "op_sample_logits_rows: rows 1..16");
    dtts_gpt_options o = *opts;
    o.row_options = rows;
    o.num_beams = 0;
    check_gpt_rows(&o, R, V, false);
    h->m->op_sample_logits_opts(logits, R, V, o, history, hist_stride, hist_lens, fills, prompt_lens, uniforms, tokens_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_first_stop_step(int input_len, int forced_prefix, int min_length, int min_new_tokens) {
    return dtts::gpt_first_stop_step(input_len, forced_prefix, min_length, min_new_tokens);
}

void dtts_gpt_decay_multipliers(double factor, int n, float* out) {
    if (out && n > 0) dtts::gpt_decay_multipliers(factor, n, out);
}

int dtts_sampler_max_vocab(void) { return dtts::sampler_max_vocab(); }

int dtts_diff_p_sample(dtts_handle* h, float* x, const float* code_emb, const int* lens, int B, int T, int step,
                       unsigned long long seed, const int* sample_ids, const float* noise, float* x0_out, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_p_sample(x, code_emb, lens, B, T, step, seed, sample_ids, noise, x0_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_latents(dtts_handle* h, const float* refer, const int* refer_lens, int Tr, const int* text, const int* text_lens,
                     int Lt_max, const int* codes, const int* ncodes, int n_max, int B, float* latents_cm, int lat_stride,
                     void* stream) {
    DTTS_API_BEGIN
    h->m->gpt_latents(refer, refer_lens, Tr, text, text_lens, Lt_max, codes, ncodes, n_max, B, latents_cm, lat_stride,
                      (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_score(dtts_handle* h, const float* latents_cm, int lat_stride, const int* targets, const int* ntargets, int n_max, int B,
                   float* logprob_out, float* logits_out, void* stream) {
    DTTS_API_BEGIN
    h->m->gpt_score(latents_cm, lat_stride, targets, ntargets, n_max, B, logprob_out, logits_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_forward_losses(dtts_handle* h, const float* refer, const int* refer_lens, int Tr, const int* text_ids, int Lt, const int* mel_codes,
                            int n, int B, float* losses_out, float* text_logprob, float* mel_logprob, float* mel_logits, void* stream) {
    DTTS_API_BEGIN
    h->m->gpt_forward_losses(refer, refer_lens, Tr, text_ids, Lt, mel_codes, n, B, losses_out, text_logprob, mel_logprob, mel_logits,
                             (hipStream_t)stream);
    DTTS_API_END(h)
}

// ---- latents in: the entries above with the conditioning encoder's output handed in (include/detail_hip.h, "voices")
int dtts_gpt_generate_cond(dtts_handle* h, const float* cond, const int* text, const int* text_lens, int Lt_max, int B,
                           const dtts_gpt_options* opts, int* codes_out, int* ncodes_out, float* latents_cm, int lat_stride, void* stream) {
    DTTS_API_BEGIN
    check_gpt_options(opts, B);
    DTTS_REQUIRE(cond, "dtts_gpt_generate_cond: cond");
    h->m->gpt_generate(nullptr, nullptr, 0, text, text_lens, Lt_max, B, *opts, codes_out, ncodes_out, latents_cm, lat_stride, (hipStream_t)stream, cond);
    DTTS_API_END(h)
}

int dtts_gpt_prefill_cond(dtts_handle* h, const float* cond, const int* text, const int* text_lens, int Lt_max, int B,
                          const dtts_gpt_options* opts, float* latents_cm, int lat_stride, void* stream) {
    DTTS_API_BEGIN
    check_gpt_options(opts, B);
    DTTS_REQUIRE(cond, "dtts_gpt_prefill_cond: cond");
    h->m->gpt_prefill(nullptr, nullptr, 0, text, text_lens, Lt_max, B, *opts, latents_cm, lat_stride, (hipStream_t)stream, cond);
    DTTS_API_END(h)
}

int dtts_gpt_beam_generate_cond(dtts_handle* h, const float* cond, const int* text, const int* text_lens, int Lt_max, int B,
                                const dtts_gpt_options* opts, int nrs, int* seqs_out, int* lens_out, float* scores_out, void* stream) {
    DTTS_API_BEGIN
    check_gpt_options(opts, B);
    DTTS_REQUIRE(cond, "dtts_gpt_beam_generate_cond: cond");
    DTTS_REQUIRE(opts->num_beams > 1, "dtts_gpt_beam_generate: options.num_beams has to be 2 .. 16");
    DTTS_REQUIRE(nrs >= 1 && nrs <= opts->num_beams, "dtts_gpt_beam_generate: num_return_sequences outside 1 .. num_beams");
    DTTS_REQUIRE(seqs_out && lens_out && scores_out, "dtts_gpt_beam_generate: null output");
    h->m->gpt_beam_generate(nullptr, nullptr, 0, text, text_lens, Lt_max, B, *opts, nrs, seqs_out, lens_out, scores_out, (hipStream_t)stream, cond);
    DTTS_API_END(h)
}

int dtts_gpt_latents_cond(dtts_handle* h, const float* cond, const int* text, const int* text_lens, int Lt_max, const int* codes,
                          const int* ncodes, int n_max, int B, float* latents_cm, int lat_stride, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(cond, "dtts_gpt_latents_cond: cond");
    h->m->gpt_latents(nullptr, nullptr, 0, text, text_lens, Lt_max, codes, ncodes, n_max, B, latents_cm, lat_stride, (hipStream_t)stream, cond);
    DTTS_API_END(h)
}

int dtts_gpt_forward_losses_cond(dtts_handle* h, const float* cond, const int* text_ids, int Lt, const int* mel_codes, int n, int B,
                                 float* losses_out, float* text_logprob, float* mel_logprob, float* mel_logits, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(cond, "dtts_gpt_forward_losses_cond: cond");
    h->m->gpt_forward_losses(nullptr, nullptr, 0, text_ids, Lt, mel_codes, n, B, losses_out, text_logprob, mel_logprob, mel_logits,
                             (hipStream_t)stream, cond);
    DTTS_API_END(h)
}

int dtts_vq_decode_cond(dtts_handle* h, const int* codes, const int* ncodes, int nmax, const float* g_vq, int B, float* mel_out, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(g_vq, "dtts_vq_decode_cond: g_vq");
    h->m->vq_decode(codes, ncodes, nmax, nullptr, nullptr, 0, B, mel_out, (hipStream_t)stream, g_vq);
    DTTS_API_END(h)
}

int dtts_voice_pool(dtts_handle* h, const float* v, const float* weights, int S, int n, int D, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->voice_pool(v, weights, S, n, D, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_wav_edges(dtts_handle* h, const float* wav, const int* lens, int B, int stride, int frame, float threshold, int keep, int* edges,
                   void* stream) {
    DTTS_API_BEGIN
    h->m->wav_edges(wav, lens, B, stride, frame, threshold, keep, edges, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_wav_join(dtts_handle* h, const float* wav, int B, int stride, const int* begins, const int* counts, const int* offsets,
                  long long total, int fade, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->wav_join(wav, B, stride, begins, counts, offsets, total, fade, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_conditioning(dtts_handle* h, const float* refer, const int* lens, int B, int Tmax, float* cond_out, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_conditioning(refer, lens, B, Tmax, cond_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_timestep_independent(dtts_handle* h, const float* latent_cm, const int* lens_n, int B, int nmax, const float* cond,
                                   float* code_emb, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_timestep_independent(latent_cm, lens_n, B, nmax, cond, code_emb, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_timestep_independent_ex(dtts_handle* h, const float* latent_cm, const int* lens_n, int B, int nmax, const float* cond,
                                      const int* frames, const int* durations, int Tmax, float* code_emb, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_timestep_independent_ex(latent_cm, lens_n, B, nmax, cond, frames, durations, Tmax, code_emb, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_frame_map(dtts_handle* h, const int* lens_n, const int* frames, const int* durations, int B, int nmax, int Tmax, int* map_out,
                      void* stream) {
    DTTS_API_BEGIN
    h->m->op_frame_map(lens_n, frames, durations, B, nmax, Tmax, map_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_forward(dtts_handle* h, const float* x, const float* code_emb, const int* lens, int B, int T, int step,
                      int cond_free, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_forward(x, code_emb, lens, B, T, step, cond_free, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_sample(dtts_handle* h, const float* code_emb, const int* lens, int B, int T, unsigned long long seed,
                     const int* sample_ids, int n_steps, const float* x_init, const float* step_noise, float* mel_out, int denorm,
                     void* stream) {
    DTTS_API_BEGIN
    h->m->diff_sample(code_emb, lens, B, T, seed, sample_ids, n_steps, x_init, step_noise, mel_out, denorm, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_schedule(dtts_handle* h, const int* timesteps, int n, int* id_out, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(id_out, "id_out");
    *id_out = h->m->diff_schedule(timesteps, n, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_schedule_coefs(dtts_handle* h, int id, int* tmap, float* coefs, int cap, int* n_out) {
    DTTS_API_BEGIN
    const int n = h->m->diff_schedule_info(id, tmap, coefs, cap);
    if (n_out) *n_out = n;
    DTTS_API_END(h)
}

int dtts_diff_sample_ex(dtts_handle* h, int id, int sampler, float eta, const float* code_emb, const int* lens, int B, int T,
                        unsigned long long seed, const int* sample_ids, int n_steps, const float* x_init, const float* step_noise,
                        float* mel_out, int denorm, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_sample_ex(id, sampler, eta, code_emb, lens, B, T, seed, sample_ids, n_steps, x_init, step_noise, mel_out, denorm,
                         (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_step(dtts_handle* h, int id, int sampler, float eta, float* x, const float* code_emb, const int* lens, int B, int T,
                   int step, unsigned long long seed, const int* sample_ids, const float* noise, float* x0_out, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_step(id, sampler, eta, x, code_emb, lens, B, T, step, seed, sample_ids, noise, x0_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_invert(dtts_handle* h, int id, const float* code_emb, const int* lens, int B, int T, const float* x_start, int depth,
                     float* x_out, float* x_traj, float* x0_traj, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_invert(id, code_emb, lens, B, T, x_start, depth, x_out, x_traj, x0_traj, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_sample_from(dtts_handle* h, int id, int sampler, float eta, int first_step, const float* code_emb, const int* lens, int B,
                          int T, unsigned long long seed, const int* sample_ids, const float* x_init, const float* step_noise,
                          float* mel_out, int denorm, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_sample_from(id, sampler, eta, first_step, code_emb, lens, B, T, seed, sample_ids, x_init, step_noise, mel_out, denorm,
                           (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_inpaint(dtts_handle* h, int id, int sampler, float eta, int first_step, int resample, const float* code_emb, const int* lens,
                      int B, int T, unsigned long long seed, const int* sample_ids, const float* x_init, const float* known,
                      const unsigned char* keep, const float* step_noise, const float* known_noise, const float* renoise, float* x_out,
                      float* x_traj, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_inpaint(id, sampler, eta, first_step, resample, code_emb, lens, B, T, seed, sample_ids, x_init, known, keep, step_noise,
                       known_noise, renoise, x_out, x_traj, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_inpaint_blend(dtts_handle* h, float* x, const float* known, const unsigned char* keep, const int* lens, int B, int C, int T,
                          const float* coefs, int step0, int renoise, unsigned long long seed, const int* sample_ids, int philox_step,
                          const float* known_noise, const float* renoise_noise, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(coefs, "coefs");
    const dtts::InpaintCoefs k = {coefs[0], coefs[1], coefs[2], coefs[3]};
    h->m->op_inpaint_blend(x, known, keep, lens, B, C, T, k, step0, renoise, seed, sample_ids, philox_step, known_noise, renoise_noise,
                           (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_inpaint_table(const int* timesteps, int n, int trained_steps, float* coefs, int cap, int* n_out) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(timesteps && n >= 1 && trained_steps >= 1, "timesteps, n >= 1, trained_steps >= 1");
    std::vector<int> tmap(timesteps, timesteps + n);
    for (int t : tmap) DTTS_REQUIRE(t >= 0 && t < trained_steps, "timestep out of [0, trained_steps)");
    std::sort(tmap.begin(), tmap.end());
    tmap.erase(std::unique(tmap.begin(), tmap.end()), tmap.end());
    dtts::ScheduleTables sc;
    dtts::make_schedule(trained_steps, tmap, 0.f, sc);
    if (n_out) *n_out = sc.n;
    DTTS_REQUIRE(!coefs || cap >= sc.n, "cap < n");
    if (coefs)
        for (int i = 0; i < sc.n; ++i) {
            const dtts::InpaintCoefs k = sc.inpaint(i);
            const float v[4] = {k.known_a, k.known_b, k.renoise_a, k.renoise_b};
            std::memcpy(coefs + (size_t)4 * i, v, sizeof(v));
        }
    DTTS_API_END(nullptr)
}

int dtts_diff_reverse_step(dtts_handle* h, int id, float* x, const float* code_emb, const int* lens, int B, int T, int step, float* x0_out,
                           void* stream) {
    DTTS_API_BEGIN
    h->m->diff_reverse_step(id, x, code_emb, lens, B, T, step, x0_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_mean_variance(dtts_handle* h, int id, const float* x, const float* code_emb, const int* lens, int B, int T, int step,
                            float* mean, float* variance, float* log_variance, float* pred_xstart, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_mean_variance(id, x, code_emb, lens, B, T, step, mean, variance, log_variance, pred_xstart, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_ddim_reverse_table(const int* timesteps, int n, int trained_steps, float cond_free_k, float* coefs, int cap, int* n_out) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(timesteps && n >= 1 && trained_steps >= 1, "timesteps, n >= 1, trained_steps >= 1");
    std::vector<int> tmap(timesteps, timesteps + n);
    for (int t : tmap) DTTS_REQUIRE(t >= 0 && t < trained_steps, "timestep out of [0, trained_steps)");
    std::sort(tmap.begin(), tmap.end());
    tmap.erase(std::unique(tmap.begin(), tmap.end()), tmap.end());
    dtts::ScheduleTables sc;
    dtts::make_schedule(trained_steps, tmap, cond_free_k, sc);
    if (n_out) *n_out = sc.n;
    DTTS_REQUIRE(!coefs || cap >= sc.n, "cap < n");
    if (coefs)
        for (int i = 0; i < sc.n; ++i) {
            const dtts::DdimReverseCoefs k = sc.ddim_reverse(i);
            const float v[6] = {sc.ac_next[i], k.sqrt_recip_ac, k.sqrt_recipm1_ac, k.sqrt_ac_next, k.sqrt_1m_ac_next, k.cfk};
            std::memcpy(coefs + (size_t)6 * i, v, sizeof(v));
        }
    DTTS_API_END(nullptr)
}

int dtts_diff_forward_t(dtts_handle* h, const float* x, const float* code_emb, const int* lens, int B, int T, int timestep,
                        int cond_free, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_forward_t(x, code_emb, lens, B, T, timestep, cond_free, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_dpm_schedule_table(int n, float* times, float* model_times, float* coefs, int cap, int* n_out) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(n >= 2, "n must be >= 2");
    std::vector<float> t, mt, lam;
    std::vector<dtts::DpmStepCoefs> st;
    dtts::dpm_schedule_table(n, 0.f, t, mt, st, &lam);              // the guidance scale is not part of the table
    if (n_out) *n_out = n;
    DTTS_REQUIRE(!(times || model_times || coefs) || cap >= n, "cap < n");
    if (times) std::memcpy(times, t.data(), sizeof(float) * (n + 1));
    if (model_times) std::memcpy(model_times, mt.data(), sizeof(float) * n);
    if (coefs)
        for (int k = 0; k < n; ++k) {
            const dtts::DpmStepCoefs& c = st[k];
            const float v[7] = {c.alpha_s, c.sigma_s, lam[k], c.ratio, c.c1, c.inv_r0, (float)c.order};
            std::memcpy(coefs + (size_t)7 * k, v, sizeof(v));
        }
    DTTS_API_END(nullptr)
}

int dtts_diff_schedule_dpm(dtts_handle* h, int n, int* id_out, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(id_out, "id_out");
    *id_out = h->m->diff_schedule_dpm(n, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_step_dpm(dtts_handle* h, int id, float* x, float* x0_hist, const float* code_emb, const int* lens, int B, int T, int step,
                       float* x0_out, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_step_dpm(id, x, x0_hist, code_emb, lens, B, T, step, x0_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_forward_tf(dtts_handle* h, const float* x, const float* code_emb, const int* lens, int B, int T, float timestep,
                         int cond_free, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_forward_tf(x, code_emb, lens, B, T, timestep, cond_free, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_forward_rows(dtts_handle* h, int id, const float* x, const float* code_emb, const int* lens, int B, int T, const int* steps,
                           float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_forward_rows(id, x, code_emb, lens, B, T, steps, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_schedule_qtable(dtts_handle* h, int id, float* table, int cap, int* n_out) {
    DTTS_API_BEGIN
    const int n = h->m->diff_schedule_qtable(id, table, cap);
    if (n_out) *n_out = n;
    DTTS_API_END(h)
}

int dtts_diff_q_sample(dtts_handle* h, int id, const float* mel, int normalize, const int* t, const float* noise, unsigned long long seed,
                       const int* sample_ids, int B, int T, float* x_start_out, float* x_t_out, float* noise_out, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_q_sample(id, mel, normalize, t, noise, seed, sample_ids, B, T, x_start_out, x_t_out, noise_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_loss_terms(dtts_handle* h, int id, const float* model_out, const float* x_start, const float* x_t, const float* noise,
                         const int* t, int B, int T, float* terms_out, float* pred_xstart, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_loss_terms(id, model_out, x_start, x_t, noise, t, B, T, terms_out, pred_xstart, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_training_losses(dtts_handle* h, int id, const float* x_start, const int* t, const float* noise, unsigned long long seed,
                              const int* sample_ids, const float* code_emb, const int* lens, int B, int T, float* terms_out,
                              float* pred_xstart, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_training_losses(id, x_start, t, noise, seed, sample_ids, code_emb, lens, B, T, terms_out, pred_xstart, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_bpd_terms(dtts_handle* h, int id, const float* model_out, const float* x_start, const float* x_t, const float* noise, const int* t,
                        int R, int T, float* terms_out, float* pred_xstart, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_bpd_terms(id, model_out, x_start, x_t, noise, t, R, T, terms_out, pred_xstart, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_prior_bpd(dtts_handle* h, int id, const float* x_start, int B, int T, float* prior_out, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_prior_bpd(id, x_start, B, T, prior_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_diff_calc_bpd(dtts_handle* h, int id, const float* x_start, const float* code_emb, const int* lens, int B, int T, const float* noise,
                       unsigned long long seed, const int* sample_ids, int rows_per_pass, float* vb, float* xstart_mse, float* mse, float* prior,
                       float* total, void* stream) {
    DTTS_API_BEGIN
    h->m->diff_calc_bpd(id, x_start, code_emb, lens, B, T, noise, seed, sample_ids, rows_per_pass, vb, xstart_mse, mse, prior, total,
                        (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_l1_mean(dtts_handle* h, const float* a, const float* b, int B, int C, int T, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->l1_mean(a, b, B, C, T, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_vocoder(dtts_handle* h, const float* mel, const int* lens, int B, int T, unsigned long long seed, const int* sample_ids,
                 float noise_scale, const float* noise_override, float* wav, float* trace_z, void* stream) {
    DTTS_API_BEGIN
    h->m->vocoder(mel, lens, B, T, seed, sample_ids, noise_scale, noise_override, wav, trace_z, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_vocoder_stream(dtts_handle* h, const float* mel, const int* lens, int B, int T, unsigned long long seed, const int* sample_ids,
                        float noise_scale, const float* noise_override, int chunk_frames, float* wav, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(chunk_frames >= 16, "chunk_frames must be >= 16");
    h->m->vocoder(mel, lens, B, T, seed, sample_ids, noise_scale, noise_override, wav, nullptr, (hipStream_t)stream, chunk_frames);
    DTTS_API_END(h)
}

int dtts_generator(dtts_handle* h, const float* z, const float* g, const int* lens, int B, int T, float* wav, void* stream) {
    DTTS_API_BEGIN
    h->m->op_generator(z, g, lens, B, T, wav, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_mel_style(dtts_handle* h, const char* which, const float* mel, const int* lens, int B, int T, float* g_out, void* stream) {
    DTTS_API_BEGIN
    h->m->op_mel_style(which, mel, lens, B, T, g_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_attention_block(dtts_handle* h, const char* prefix, const float* x, const int* lens, int B, int C, int T, float* y,
                            void* stream) {
    DTTS_API_BEGIN
    h->m->op_attention_block(prefix, x, lens, B, C, T, y, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_resblock(dtts_handle* h, const char* prefix, const float* x, const int* lens, int B, int T, int step, float* y,
                     void* stream) {
    DTTS_API_BEGIN
    h->m->op_resblock(prefix, x, lens, B, T, step, y, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_conv1d(dtts_handle* h, const char* name, const float* x, const int* lens_in, int B, int Cin, int Tin, int Cout, int KW,
                   int stride, int dil, int pad, int pro_act, int epi_act, int gate, int phases, const float* res, float* y,
                   int Tout_alloc, void* stream) {
    DTTS_API_BEGIN
    h->m->op_conv1d(name, x, lens_in, B, Cin, Tin, Cout, KW, stride, dil, pad, pro_act, epi_act, gate, phases, res, y, Tout_alloc,
                    (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_conv1d_x3(dtts_handle* h, const char* name, const float* x, const int* lens, int B, int Cin, int T, int Cout, int KW,
                      int epi_act, float out_scale, int gate, const float* badd, const float* res, int p1, int ksplit_max, float* y,
                      dtts_conv_x3_info* info, void* stream) {
    DTTS_API_BEGIN
    dtts::ConvX3Launch c;
    h->m->op_conv1d_x3(name, x, lens, B, Cin, T, Cout, KW, epi_act, out_scale, gate, badd, res, p1, ksplit_max, y, &c, (hipStream_t)stream);
    if (info) {
        info->epi = c.epi; info->kw3 = c.kw3; info->stages = c.stages; info->ksplit = c.ksplit;
        info->p1 = c.p1; info->epi_vec = c.epi_vec; info->cols = c.cols; info->workgroups = c.workgroups;
    }
    DTTS_API_END(h)
}

size_t dtts_attn_x3_image_bytes(int B, int H, int T) {
    return (B > 0 && H > 0 && T > 0) ? dtts::AttnPlanes::bytes(B, H, T) : 0;
}

int dtts_op_attention_x3(dtts_handle* h, const char* name, const float* x, const int* lens, int B, int Cin, int T, int H,
                         const float* bias_tab, int p1, int out_f32, void* y, void* img_out, dtts_attn_x3_info* info, void* stream) {
    DTTS_API_BEGIN
    dtts::ConvX3Launch c;
    dtts::AttnX3Launch a;
    h->m->op_attention_x3(name, x, lens, B, Cin, T, H, bias_tab, p1, out_f32, y, img_out, &c, &a, (hipStream_t)stream);
    if (info) {
        info->conv.epi = c.epi; info->conv.kw3 = c.kw3; info->conv.stages = c.stages; info->conv.ksplit = c.ksplit;
        info->conv.p1 = c.p1; info->conv.epi_vec = c.epi_vec; info->conv.cols = c.cols; info->conv.workgroups = c.workgroups;
        info->attn_ksplit = a.ksplit; info->attn_p1 = a.p1; info->attn_workgroups = a.workgroups;
    }
    DTTS_API_END(h)
}

int dtts_op_attention(dtts_handle* h, const float* qkv, const int* lens, int B, int rows, int cs, int T, int H, int D, int q_off,
                      int k_off, int v_off, int head_stride, float scale, const float* bias_tab, int causal, const float* band,
                      int band_w, float* y, float* ml, void* stream) {
    DTTS_API_BEGIN
    h->m->op_attention(qkv, lens, B, rows, cs, T, H, D, q_off, k_off, v_off, head_stride, scale, bias_tab, causal, band, band_w, y, ml,
                       (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_attention_rel(dtts_handle* h, const float* qkv, const int* lens, int B, int T, int H, int D, const float* ek,
                          const float* ev, int window, float scale, float* y, float* relk, float* ml, void* stream) {
    DTTS_API_BEGIN
    h->m->op_attention_rel(qkv, lens, B, T, H, D, ek, ev, window, scale, y, relk, ml, (hipStream_t)stream);
    DTTS_API_END(h)
}

// ---- text-to-audio alignment (include/detail_hip.h, "alignment")
int dtts_gpt_attentions(dtts_handle* h, const float* refer, const int* refer_lens, int Tr, const int* text, const int* text_lens, int Lt_max,
                        const int* codes, const int* ncodes, int n_max, int B, const int* layers, int n_layers, float* out, int L_out,
                        void* stream) {
    DTTS_API_BEGIN
    h->m->gpt_attentions(refer, refer_lens, Tr, text, text_lens, Lt_max, codes, ncodes, n_max, B, layers, n_layers, out, L_out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_attentions_cond(dtts_handle* h, const float* cond, const int* text, const int* text_lens, int Lt_max, const int* codes,
                             const int* ncodes, int n_max, int B, const int* layers, int n_layers, float* out, int L_out, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(cond, "dtts_gpt_attentions_cond: cond");
    h->m->gpt_attentions(nullptr, nullptr, 0, text, text_lens, Lt_max, codes, ncodes, n_max, B, layers, n_layers, out, L_out, (hipStream_t)stream, cond);
    DTTS_API_END(h)
}

int dtts_gpt_text_alignment(dtts_handle* h, const float* refer, const int* refer_lens, int Tr, const int* text, const int* text_lens, int Lt_max,
                            const int* codes, const int* ncodes, int n_max, int B, const int* layers, int n_layers, const float* head_weights,
                            float* attn, float* text_mass, void* stream) {
    DTTS_API_BEGIN
    h->m->gpt_text_alignment(refer, refer_lens, Tr, text, text_lens, Lt_max, codes, ncodes, n_max, B, layers, n_layers, head_weights, attn,
                             text_mass, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_gpt_text_alignment_cond(dtts_handle* h, const float* cond, const int* text, const int* text_lens, int Lt_max, const int* codes,
                                 const int* ncodes, int n_max, int B, const int* layers, int n_layers, const float* head_weights, float* attn,
                                 float* text_mass, void* stream) {
    DTTS_API_BEGIN
    DTTS_REQUIRE(cond, "dtts_gpt_text_alignment_cond: cond");
    h->m->gpt_text_alignment(nullptr, nullptr, 0, text, text_lens, Lt_max, codes, ncodes, n_max, B, layers, n_layers, head_weights, attn,
                             text_mass, (hipStream_t)stream, cond);
    DTTS_API_END(h)
}

int dtts_op_attn_probs(dtts_handle* h, const float* qkv, const int* lens, int B, int rows, int cs, int T, int H, int D, int q_off, int k_off,
                       int head_stride, float scale, const int* q0, const int* nq, const int* k0, const int* nk, int nq_max, int nk_max,
                       int mode, const float* head_weights, int first, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->op_attn_probs(qkv, lens, B, rows, cs, T, H, D, q_off, k_off, head_stride, scale, q0, nq, k0, nk, nq_max, nk_max, mode, head_weights,
                        first, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_monotone_path(dtts_handle* h, const float* score, const int* n, const int* m, int B, int n_max, int m_max, int* path,
                          void* stream) {
    DTTS_API_BEGIN
    h->m->op_monotone_path(score, n, m, B, n_max, m_max, path, (hipStream_t)stream);
    DTTS_API_END(h)
}

// ---- the decode chain's kernels, one launch each (include/detail_hip.h)
int dtts_op_gemv_block(dtts_handle* h, int pro, const float* W, int K, int CoutP, int B, const float* x, int x_stride, const float* parts,
                       int in_slices, int in_stride, int in_act, const float* in_bias, const float* gamma, float* y_out, float* stats_out,
                       const float* stats_in, int stats_slices, int K_ln, const float* fold_c, const float* fold_d, float* part,
                       dtts_gemv_info* info, void* stream) {
    DTTS_API_BEGIN
    dtts::GemvIn in;
    in.x = x; in.x_stride = x_stride; in.parts = parts; in.in_slices = in_slices; in.in_stride = in_stride; in.in_act = in_act;
    in.in_bias = in_bias; in.gamma = gamma; in.y_out = y_out; in.stats_out = stats_out; in.stats_in = stats_in;
    in.stats_slices = stats_slices; in.K_ln = K_ln; in.fold_c = fold_c; in.fold_d = fold_d;
    dtts::GemvShape g{0, 0, 0};
    int slices = 0;
    h->m->op_gemv_block(pro, W, K, CoutP, in, B, part, &g, &slices, (hipStream_t)stream);
    if (info) { info->slices = slices; info->vec = g.vec; info->rpw = g.rpw; info->nb = g.nb; }
    DTTS_API_END(h)
}

int dtts_op_decode_attention(dtts_handle* h, const float* part, int slices, int CoutP, const float* stats, int stats_slices,
                             const float* fold_c, const float* fold_d, float* cache, long long cache_bs, int cap, const int* lp,
                             const int* step, int B, int H, int D, int ksplit, const float* wproj, int wpCoutP, float* out, void* stream) {
    DTTS_API_BEGIN
    h->m->op_decode_attention(part, slices, CoutP, stats, stats_slices, fold_c, fold_d, cache, cache_bs, cap, lp, step, B, H, D, ksplit, wproj,
                              wpCoutP, out, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_gpt_final_ln(dtts_handle* h, const float* res, const float* bias, const float* parts, int in_slices, int in_stride, int B,
                         const float* g1, const float* b1, const float* g2, const float* b2, float* y, int C, const int* step,
                         int max_steps, float* latents, int lat_cs, void* stream) {
    DTTS_API_BEGIN
    h->m->op_gpt_final_ln(res, bias, parts, in_slices, in_stride, B, g1, b1, g2, b2, y, C, step, max_steps, latents, lat_cs, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_ln_fold_vectors(dtts_handle* h, const float* W, int K, int CoutP, const float* gamma, const float* beta, const float* bias,
                            float* c, float* d, void* stream) {
    DTTS_API_BEGIN
    h->m->op_ln_fold_vectors(W, K, CoutP, gamma, beta, bias, c, d, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_kv_to_cache(dtts_handle* h, const float* qkv, const int* lens, int B, int C, int L, float* cache, long long cache_bs, int cap,
                        void* stream) {
    DTTS_API_BEGIN
    h->m->op_kv_to_cache(qkv, lens, B, C, L, cache, cache_bs, cap, (hipStream_t)stream);
    DTTS_API_END(h)
}

int dtts_op_philox_normal(dtts_handle* h, float* out, int n, int B, unsigned long long seed, const int* sample_ids, int stage,
                          int step, void* stream) {
    DTTS_API_BEGIN
    h->m->op_philox_normal(out, n, B, seed, sample_ids, stage, step, (hipStream_t)stream);
    DTTS_API_END(h)
}

}  // extern "C"
