// Host-side runtime of libdetail_hip.so: weight binding, workspace, stage orchestration.
// Everything here enqueues work on the caller's HIP stream; no hidden synchronisation except
// workspace growth (hipMalloc) which only happens when a call needs more memory than any before it, and the schedule cache
// (diff_schedule: hipMalloc of a new schedule's tables; an eviction waits for the last launch that read the evicted tables).
// The unconditional code-path cache (option uncond_cache_mb) allocates its one block at the first sampling call that can use it.
#pragma once
#include <map>
#include <memory>
#include <atomic>
#include <thread>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "attention.h"
#include "attn_probs.h"
#include "common.h"
#include "conv_gemm.h"
#include "conv_x3.h"
#include "diff_loss.h"
#include "diff_schedule.h"
#include "disc.h"
#include "flowvae_fwd.h"
#include "gpt_kernels.h"
#include "ops.h"
#include "uncond_cache.h"
#include "../../include/detail_hip.h"

namespace dtts {

struct PackedConv {
    const float* w = nullptr;
    const float* b = nullptr;   // padded to CoutP, packed row order (may be null)
    int Cin = 0, CinP = 0, Cout = 0, CoutP = 0, KW = 1;
    const void* w3 = nullptr;   // split-precision copy [KW][Cin/8][3][CoutP][8 bf16] (conv_x3.h), hot diffusion convs only
};

static inline int packed_cout(int cout) { return cout > 64 ? round_up(cout, 128) : (cout > 32 ? 64 : 32); }

// GroupNorm groups of a C-channel norm (normalization(), vqvae/utils/diff_util.py): 32, halved until it divides C
static inline int gn_groups(int C) {
    int groups = 32;
    while (C % groups) groups /= 2;
    return groups;
}

struct AttnBlockW {
    const float *gn_g = nullptr, *gn_b = nullptr, *bias_tab = nullptr;
    PackedConv qkv, proj;
    int C = 0, H = 0;
};

struct ResBlockW {
    const float *gn1_g = nullptr, *gn1_b = nullptr, *gn2_g = nullptr, *gn2_b = nullptr;
    PackedConv c1, c2, emb;
    int index = 0;   // row block in the scale/shift table
};

struct DiffLayerW {
    ResBlockW rb;
    AttnBlockW at;
};

struct MelStyleW {           // MelStyleEncoder (vqvae/modules/modules.py:642-720)
    PackedConv sp0, sp1, t0, t1, qkv, afc, fc;
    int n_mel = 0, hidden = 0, out = 0;
};

struct EncLayerW {           // attentions.Encoder layer (vqvae/modules/attentions.py:73-107)
    PackedConv qkv, o, f1, f2;
    const float *ek = nullptr, *ev = nullptr, *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
};

struct WnW {                 // modules.WN of n_layers gated layers (vqvae/modules/modules.py:152-229): the flows' have 4, enc_q's 16
    PackedConv cond;
    std::vector<PackedConv> in, res, skip;      // in / skip: n_layers; res: n_layers - 1 (the last layer has no residual half)
    int n_layers = 0;
};

struct CouplingW {           // ResidualCouplingLayer (vqvae/modules/modules.py:421-475)
    PackedConv pre, post;
    WnW enc;
};

struct PosteriorW {          // PosteriorEncoder / enc_q (vqvae/model_24k.py:172-218); optional, bound when the blob carries it
    PackedConv pre, proj;
    WnW enc;
    int spec_channels = 0;   // filter_length / 2 + 1, read from the bound blob (enc_q.pre.cin)
};

struct DiscPeriodW {         // DiscriminatorP (vqvae/model_24k.py:298-374): convs.0 direct, convs.1 .. 3 as de-interleaved 2-tap GEMMs, convs.4, conv_post
    const float *w0 = nullptr, *b0 = nullptr;
    PackedConv c[4], post;
};

struct DiscW {               // MultiPeriodDiscriminator (vqvae/model_24k.py:407-431); bound by bind_discriminator from a blob of its own
    const float *sw[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, *sb[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    PackedConv s5, s_post;   // DiscriminatorS convs.0 .. 4 above (direct / grouped kernels), convs.5 and conv_post as GEMMs
    DiscPeriodW per[5];
};

// where dtts_disc_forward puts its 37 maps (include/detail_hip.h dtts_disc_layout): map m is [N][p][C][H] at float offset off[m]
struct DiscLayout {
    long long off[DISC_MAPS + 1];
    int C[DISC_MAPS], H[DISC_MAPS], p[DISC_MAPS];
    long long numel(int m, int N) const { return (long long)N * p[m] * C[m] * H[m]; }
};
DiscLayout disc_layout(int N, int t);
long long flowvae_stage_work_floats(int B, int T, int seg, int hop);

struct GptLayerW {
    const float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
    PackedConv attn, proj, fc, fc2;
    // LayerNorm-algebra vectors of the decode step (gpt_kernels.h): c = W^T gamma, d = W^T beta + bias for c_attn / c_fc
    const float *attn_c = nullptr, *attn_d = nullptr, *fc_c = nullptr, *fc_d = nullptr;
};

// host arithmetic of HF's length processors and decay penalty (model_gpt.hip; also behind dtts_gpt_first_stop_step / dtts_gpt_decay_multipliers)
int gpt_first_stop_step(int input_len, int forced_prefix, int min_length, int min_new_tokens);
void gpt_decay_multipliers(double factor, int n, float* out);

// A GPT decode session (dtts_gpt_prefill .. dtts_gpt_finish): device state of <= 8 sequences in the handle's own arena
struct GptSession {
    int B = 0, cap = 0, G = 0, steps = 0;      // rows, KV capacity (columns), max_generate_length, tokens generated so far
    bool active = false;
    long long kv_bs = 0, kv_layer = 0;
    float *kv = nullptr, *x = nullptr, *y = nullptr, *ab = nullptr, *lat = nullptr, *xa = nullptr, *part = nullptr, *part2 = nullptr,
          *st1 = nullptr, *st2 = nullptr;
    unsigned char* seen = nullptr;
    int *finished = nullptr, *codes = nullptr, *forced = nullptr;
    int* hist = nullptr;               // [B][cap] ordered token history (no_repeat_ngram_size)
    unsigned char* tok_mask = nullptr; // [V] suppress_tokens / begin_suppress_tokens bits ([B][V] under row_options)
    float* decay_mul = nullptr;        // [<= B][G + 1] exponential_decay_length_penalty multipliers, one slice per distinct factor
    GptCtl* ctl = nullptr;
    // persistent token kernel (gpt_token.hip): exchange arena, logits rows, error flag, launch counter
    unsigned long long* xch = nullptr;
    float* logits = nullptr;
    int* tok_err = nullptr;
    unsigned* tok_epoch = nullptr;
    int tok_wgs = 128;                 // workgroups of the token kernel for this session (dtts_gpt_options.token_wgs, else option gpt_token_wgs)
    bool fuse_proj = true;             // the chain's attention applies its output projection itself (option gpt_fuse_proj, latched at prefill)
    // beam search (gpt_beam.hip): beam_K > 1 = the rows are B / beam_K utterances x beam_K beams and the beam kernels take the sampler's
    // place.  The buffers are laid out for every session (their addresses do not depend on K); graphs are dropped when K changes.
    int beam_K = 0, beam_es = 0;
    float beam_lp = 1.f;
    int *b_run_seq = nullptr, *b_fin_seq = nullptr, *b_fin_flag = nullptr, *b_fin_len = nullptr, *b_unsat = nullptr, *b_done = nullptr,
        *b_parents = nullptr, *b_tokens = nullptr, *b_last_step = nullptr, *b_ident = nullptr;
    float *b_run_score = nullptr, *b_fin_score = nullptr, *b_len_div = nullptr;
};

struct ResBlock1W {
    PackedConv c1[3], c2[3];
    int k = 3;
};

struct GenStageW {
    PackedConv up;
    int rate = 1, up_pad = 0, cout = 0;
    ResBlock1W rb[3];
};

class Arena {
public:
    ~Arena();
    void ensure(size_t bytes);            // grow (sync + realloc) if needed, then reset
    void reset() { off_ = 0; }
    size_t mark() const { return off_; }
    void rewind(size_t m) { off_ = m; }
    float* f32(size_t n) { return static_cast<float*>(raw(n * sizeof(float))); }
    int* i32(size_t n) { return static_cast<int*>(raw(n * sizeof(int))); }
    void* raw(size_t bytes);
    size_t capacity() const { return cap_; }
    void swap(Arena& o) { std::swap(base_, o.base_); std::swap(cap_, o.cap_); std::swap(off_, o.off_); }

private:
    char* base_ = nullptr;
    size_t cap_ = 0, off_ = 0;
};

// A stage-local arena stands in for the handle's main workspace for the duration of one entry point ON THE CALLING THREAD, so stages
// that run concurrently on different streams - and are issued from different host threads (stage A of the next request under stage B of
// this one, SynthesizerTrn.infer_stream) - never share scratch.
class ArenaUse {
public:
    explicit ArenaUse(Arena& a);
    ~ArenaUse();
    ArenaUse(const ArenaUse&) = delete;
    ArenaUse& operator=(const ArenaUse&) = delete;

private:
    Arena* prev_;
};
Arena* arena_override();     // the calling thread's stand-in (nullptr: none)

// While one lives ON THE CALLING THREAD, the trunk's launches make no choice by the number of samples they cover: Model::run_conv caps
// conv_x3's split-K at 1 and attention_block the attention's key split, the two places where the batch size picks a summation order.
// A sample's result is then the same bits whatever rows share its launch (diff_calc_bpd: any rows_per_pass gives the same bits).
class RowInvariantLaunches {
public:
    RowInvariantLaunches();
    ~RowInvariantLaunches();
    RowInvariantLaunches(const RowInvariantLaunches&) = delete;
    RowInvariantLaunches& operator=(const RowInvariantLaunches&) = delete;
    static bool on();

private:
    bool prev_;
};

class Model {
public:
    Model(const dtts_config& cfg, int device);
    ~Model();

    void bind_weights(const void* blob, size_t nbytes, const char* const* names, const unsigned long long* offsets,
                      const unsigned long long* numels, int n, hipStream_t stream);

    // ---- stage B
    void diff_conditioning(const float* refer, const int* lens_host, int B, int Tmax, float* cond_out, hipStream_t s);
    void diff_timestep_independent(const float* latent_cm, const int* lens_n_host, int B, int nmax, const float* cond,
                                   float* code_emb, hipStream_t s);
    // ... expanded to a frame plan (frame_map.hip): row b to frames_host[b] frames, uniformly (F.interpolate's nearest rule) or by
    // durations_host [B, nmax]; code_emb [B,768,Tmax].  frames_host == nullptr: the entry above, the same launches.
    void diff_timestep_independent_ex(const float* latent_cm, const int* lens_n_host, int B, int nmax, const float* cond,
                                      const int* frames_host, const int* durations_host, int Tmax, float* code_emb, hipStream_t s);
    void op_frame_map(const int* lens_n_host, const int* frames_host, const int* durations_host, int B, int nmax, int Tmax, int* map_out,
                      hipStream_t s);
    void check_frames(const int* lens_n_host, const int* frames_host, const int* durations_host, int B, int nmax, int Tmax);
    void frame_map_device(const int* d_lens_n, const int* d_frames, const int* durations_host, int B, int nmax, int Tmax, int* map,
                          hipStream_t s);
    void affine_gather(const float* x, long long x_bs, int x_cs, const float* ab, const int* d_frames, const int* map, int Tmax, int B, int C,
                       float* y, hipStream_t s);
    void diff_forward(const float* x, const float* code_emb, const int* lens_host, int B, int T, int step, int cond_free,
                      float* out, hipStream_t s);
    void diff_sample(const float* code_emb, const int* lens_host, int B, int T, unsigned long long seed, const int* sample_ids_host,
                     int n_steps, const float* x_init, const float* step_noise, float* mel_out, int denorm, hipStream_t s);
    // any schedule (id from diff_schedule) and sampler (0 = ancestral p_sample, 1 = DDIM with `eta`); diff_sample == diff_sample_ex(0, 0, 0)
    void diff_sample_ex(int sched_id, int sampler, float eta, const float* code_emb, const int* lens_host, int B, int T,
                        unsigned long long seed, const int* sample_ids_host, int n_steps, const float* x_init, const float* step_noise,
                        float* mel_out, int denorm, hipStream_t s);
    // one sampler step of schedule `sched_id` on x in place (unit entry of the sampler parity tests)
    void diff_step(int sched_id, int sampler, float eta, float* x, const float* code_emb, const int* lens_host, int B, int T, int step,
                   unsigned long long seed, const int* sample_ids_host, const float* noise, float* x0_out, hipStream_t s);
    // DDIM inversion (ddim_reverse_sample, vqvae/utils/diffusion.py:785-817, iterated): steps 0 .. depth - 1 of integer-timestep schedule
    // `sched_id` upwards from x_start; x_out [B,128,T] = x at the level of step index `depth`; x_traj / x0_traj (optional)
    // [depth][B,128,T]: x after every step / every step's pred_xstart
    void diff_invert(int sched_id, const float* code_emb, const int* lens_host, int B, int T, const float* x_start, int depth, float* x_out,
                     float* x_traj, float* x0_traj, hipStream_t s);
    // diff_sample_ex from below the top of the schedule: x_init is x at the level of step `first_step`, steps first_step .. 0 run
    // (samplers 0 and 1).  Both are sample_loop, whose code-path table is evaluated in the launches the whole loop makes.
    void diff_sample_from(int sched_id, int sampler, float eta, int first_step, const float* code_emb, const int* lens_host, int B, int T,
                          unsigned long long seed, const int* sample_ids_host, const float* x_init, const float* step_noise, float* mel_out,
                          int denorm, hipStream_t s);
    // diff_sample_from with inpainting (RePaint): after every sampler update the frames with keep[b][t] != 0 are overwritten with
    // `known` noised to the level just reached, and every step above 0 is evaluated `resample` times with one forward step in between
    // (diff_inpaint.h).  x_init NULL: first_step = n - 1 and x_T is drawn (draw_x_T).  x_out: the normalised x_0.  The three
    // optional noise arrays are [first_step * resample + 1][B,128,T] in evaluation order; x_traj (optional), the same shape: x after
    // every evaluation's blend.
    void diff_inpaint(int sched_id, int sampler, float eta, int first_step, int resample, const float* code_emb, const int* lens_host,
                      int B, int T, unsigned long long seed, const int* sample_ids_host, const float* x_init, const float* known,
                      const unsigned char* keep, const float* step_noise, const float* known_noise, const float* renoise, float* x_out,
                      float* x_traj, hipStream_t s);
    // one launch of the inpainting blend on caller-supplied x (= u, in place) [B,C,T] (unit entry of the kernel's tests)
    void op_inpaint_blend(float* x, const float* known, const unsigned char* keep, const int* lens_host, int B, int C, int T,
                          InpaintCoefs k, int step0, int renoise, unsigned long long seed, const int* sample_ids_host, int pstep,
                          const float* known_noise, const float* renoise_noise, hipStream_t s);
    // one ddim_reverse_sample at spaced step `step`, x in place (diff_invert's step: the same bits)
    void diff_reverse_step(int sched_id, float* x, const float* code_emb, const int* lens_host, int B, int T, int step, float* x0_out,
                           hipStream_t s);
    // p_mean_variance (:284-386) at spaced step `step`: mean, variance, log_variance, pred_xstart [B,128,T]; x is read only
    void diff_mean_variance(int sched_id, const float* x, const float* code_emb, const int* lens_host, int B, int T, int step, float* mean,
                            float* variance, float* log_variance, float* pred_xstart, hipStream_t s);
    // DiffusionTts.forward at any model timestep in [0, diff_trained_steps): default-schedule timesteps take their step of that schedule
    void diff_forward_t(const float* x, const float* code_emb, const int* lens_host, int B, int T, int timestep, int cond_free,
                        float* out, hipStream_t s);
    // the schedule of these model timesteps (any order, duplicates ignored): built on s on first use, then cached; returns its id
    int diff_schedule(const int* timesteps, int n, hipStream_t s);
    // host copy of a schedule: tmap[n]; coefs: per step {sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, min_log, max_log, cfk, ac, ac_prev}
    int diff_schedule_info(int sched_id, int* tmap, float* coefs, int cap);
    // the DPM-Solver++(2M) schedule of n steps (dpm_schedule_table + its AdaGN table at the fractional model times): as diff_schedule
    int diff_schedule_dpm(int n, hipStream_t s);
    // one DPM-Solver++(2M) step of DPM schedule `sched_id` at step index `step` (n - 1 = first): x in place; x0_hist [B,128,T] holds the
    // previous step's x0 (read by a second-order step) and receives this step's; x0_out (optional) receives it too
    void diff_step_dpm(int sched_id, float* x, float* x0_hist, const float* code_emb, const int* lens_host, int B, int T, int step,
                       float* x0_out, hipStream_t s);
    // DiffusionTts.forward at a fp32 model time in [0, diff_trained_steps): integer values take diff_forward_t's route bit for bit
    void diff_forward_tf(const float* x, const float* code_emb, const int* lens_host, int B, int T, float timestep, int cond_free,
                         float* out, hipStream_t s);
    // DiffusionTts.forward, conditional branch only, with every batch row at its own column of integer-timestep schedule `sched_id`:
    // row b is evaluated at column step_of_row[b] (HOST, B) in the conditioning_timestep_integrator and in every ResBlock of the stack
    // and tail.  A B-sample stack on the caller's stream (no unconditional rows), three-product trunk, GroupNorm as its own pass.
    void diff_forward_rows(int sched_id, const float* x, const float* code_emb, const int* lens_host, int B, int T, const int* step_of_row,
                           float* out, hipStream_t s);
    // ---- evaluation losses (diff_loss.h; GaussianDiffusion.training_losses, vqvae/utils/diffusion.py:930-1012).  t_host [B]: columns of
    // the integer-timestep schedule `sched_id`.  The losses are means over the whole [128, T] rectangle of every row (mean_flat).
    void diff_q_sample(int sched_id, const float* mel, int normalize, const int* t_host, const float* noise, unsigned long long seed,
                       const int* sample_ids_host, int B, int T, float* x_start_out, float* x_t_out, float* noise_out, hipStream_t s);
    void diff_loss_terms(int sched_id, const float* model_out, const float* x_start, const float* x_t, const float* noise, const int* t_host,
                         int B, int T, float* terms_out, float* pred_xstart, hipStream_t s);
    void diff_training_losses(int sched_id, const float* x_start, const int* t_host, const float* noise, unsigned long long seed,
                              const int* sample_ids_host, const float* code_emb, const int* lens_host, int B, int T, float* terms_out,
                              float* pred_xstart, hipStream_t s);
    void l1_mean(const float* a, const float* b, int B, int C, int T, float* out, hipStream_t s);
    // ---- the variational bound in bits per dimension (diff_bpd.h; calc_bpd_loop, _vb_terms_bpd, _prior_bpd,
    // vqvae/utils/diffusion.py:903-928, 1098-1169).  terms_out [R][3] = (vb, xstart_mse, mse); vb / xstart_mse / mse [B][S], column j =
    // timestep S - 1 - j; noise [S][B][128][T] by timestep or null (Philox STAGE_DIFF_BPD); rows_per_pass 0: the library's choice
    void diff_bpd_terms(int sched_id, const float* model_out, const float* x_start, const float* x_t, const float* noise, const int* t_host,
                        int R, int T, float* terms_out, float* pred_xstart, hipStream_t s);
    void diff_prior_bpd(int sched_id, const float* x_start, int B, int T, float* prior_out, hipStream_t s);
    void diff_calc_bpd(int sched_id, const float* x_start, const float* code_emb, const int* lens_host, int B, int T, const float* noise,
                       unsigned long long seed, const int* sample_ids_host, int rows_per_pass, float* vb, float* xstart_mse, float* mse,
                       float* prior, float* total, hipStream_t s);
    // host copy of a schedule's forward-process tables: out[i] = {sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod} of column i
    int diff_schedule_qtable(int sched_id, float* out, int cap);
    // one p_sample at `step` on x in place (unit entry of the sampler parity tests)
    void diff_p_sample(float* x, const float* code_emb, const int* lens_host, int B, int T, int step, unsigned long long seed,
                       const int* sample_ids_host, const float* noise, float* x0_out, hipStream_t s);
    // ---- voices (voice.hip): out [S, D] = sum_j w[s][j] v[s, j, :] / sum_j w[s][j] over the n clips of speaker s; w_host nullptr = all 1
    void voice_pool(const float* v, const float* w_host, int S, int n, int D, float* out, hipStream_t s);
    // ---- long form (wav_join.hip): the loud span of every row of a padded waveform batch, and the rows' spans laid end to end
    void wav_edges(const float* wav, const int* lens_host, int B, int stride, int frame, float threshold, int keep, int* edges, hipStream_t s);
    void wav_join(const float* wav, int B, int stride, const int* begins, const int* counts, const int* offsets, long long total, int fade,
                  float* out, hipStream_t s);
    // ---- stage A
    // Every stage-A entry that takes the prompt mel `refer` also takes cond_in [B, gpt_dim] (device): the conditioning encoder's output,
    // computed earlier (a voice, voice.hip).  With cond_in the encoder is not launched and refer / refer_lens_host / Tr are not read.
    void gpt_generate(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host,
                      int Lt_max, int B, const dtts_gpt_options& o, int* codes_host, int* ncodes_host, float* latents_cm,
                      int lat_stride, hipStream_t s, const float* cond_in = nullptr);
    // decode session: prefill (+ first token) -> decode steps (eager / captured hipGraphs) -> results
    void gpt_prefill(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host, int Lt_max,
                     int B, const dtts_gpt_options& o, float* latents_cm, int lat_stride, hipStream_t s, const float* cond_in = nullptr);
    void gpt_decode_step(hipStream_t s);
    int gpt_decode(int n_steps, hipStream_t s);
    int gpt_all_finished(hipStream_t s);
    void gpt_finish(int* codes_host, int* ncodes_host, hipStream_t s);
    int gpt_steps() const { return gs_.active ? gs_.steps : 0; }
    // beam search: B utterances x o.num_beams beams, whole utterances per session; per utterance the best nrs finished hypotheses (HOST)
    void gpt_beam_generate(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host, int Lt_max,
                           int B, const dtts_gpt_options& o, int nrs, int* seqs_host, int* lens_host, float* scores_host, hipStream_t s,
                           const float* cond_in = nullptr);
    void gpt_beam_finish(int nrs, int* seqs_host, int* lens_host, float* scores_host, hipStream_t s);
    void op_beam_step(const float* logits, int U, int V, const dtts_gpt_options& o, int step, const int* prompt_host, int prompt_len,
                      int* run_seq, float* run_score, int* fin_seq, float* fin_score, int* fin_flag, int* fin_len, int* unsat, int* done,
                      int* parents, int* tokens, float* cand_score, int* cand_beam, int* cand_tok, hipStream_t s);
    void op_sample_logits(const float* logits, int R, int V, const int* history_host, int hist_len, const float* uniforms, int top_k,
                          float top_p, float temperature, float repetition_penalty, float typical_mass, int suppress_eos, int* tokens_host,
                          hipStream_t s);
    void op_sample_logits_opts(const float* logits, int R, int V, const dtts_gpt_options& o, const int* history_host, int hist_stride,
                               const int* hist_lens, const int* fills, const int* prompt_lens, const float* uniforms, int* tokens_host,
                               hipStream_t s);
    void gpt_latents(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host,
                     int Lt_max, const int* codes_host, const int* ncodes_host, int n_max, int B, float* latents_cm, int lat_stride,
                     hipStream_t s, const float* cond_in = nullptr);
    // log p(targets[b][k] | latents_cm[b, :, k]) under the unprocessed distribution (gpt_score.hip); targets / ntargets HOST; asynchronous
    void gpt_score(const float* latents_cm, int lat_stride, const int* targets_host, const int* ntargets_host, int n_max, int B,
                   float* logprob_out, float* logits_out, hipStream_t s);
    // UnifiedVoice.forward's loss mode (gpt/model.py:429-491) on a RECTANGULAR batch: every row has Lt text ids and n mel codes (HOST).
    // losses_out DEVICE [2] = (loss_text, loss_mel), the plain means over all B (Lt + 2) / B (n + 2) positions; optional DEVICE outputs:
    // text_logprob [B][Lt + 2], mel_logprob [B][n + 2] (log-softmax at the targets), mel_logits [B][V][n + 2].  Needs gpt.text_head.
    void gpt_forward_losses(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, int Lt, const int* codes_host, int n,
                            int B, float* losses_out, float* text_logprob, float* mel_logprob, float* mel_logits, hipStream_t s,
                            const float* cond_in = nullptr);
    // ---- text-to-audio alignment (model_align.hip; include/detail_hip.h "alignment")
    void gpt_attentions(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host, int Lt_max,
                        const int* codes_host, const int* ncodes_host, int n_max, int B, const int* layers_host, int n_layers, float* out,
                        int L_out, hipStream_t s, const float* cond_in = nullptr);
    void gpt_text_alignment(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host, int Lt_max,
                            const int* codes_host, const int* ncodes_host, int n_max, int B, const int* layers_host, int n_layers,
                            const float* head_weights_host, float* attn_out, float* text_mass_out, hipStream_t s, const float* cond_in = nullptr);
    void op_attn_probs(const float* qkv, const int* lens_host, int B, int rows, int cs, int T, int H, int D, int q_off, int k_off, int head_stride,
                       float scale, const int* q0_host, const int* nq_host, const int* k0_host, const int* nk_host, int nq_max, int nk_max,
                       int mode, const float* w_host, int first, float* out, hipStream_t s);
    void op_monotone_path(const float* score, const int* n_host, const int* m_host, int B, int n_max, int m_max, int* path, hipStream_t s);
    // ---- the decode chain's kernels (gpt_kernels.h), ONE launch each on the caller's buffers (model_gpt.hip; weightless handles serve them).
    // Every argument the launcher or the kernel cannot take is refused before anything is launched or uploaded.
    // op_gemv_block: launch_gemv_block(pro, W [K][CoutP], in, B) -> part [slices][B][CoutP]; `in` carries the caller's DEVICE pointers
    // (the fields the prologue does not read may be null); shape / slices: what the launcher chose.
    void op_gemv_block(int pro, const float* W, int K, int CoutP, const GemvIn& in, int B, float* part, GemvShape* shape, int* slices,
                       hipStream_t s);
    // op_decode_attention: launch_decode_attention_qkv with a control block built from lp / step (HOST [B]); cache DEVICE [B][cache_bs]
    // (K [C][cap] | V [cap][C]), updated in place; out = records [B][H][KS][ATT_REC], or with wproj [H D][768] partials [H][B][768]
    void op_decode_attention(const float* part, int slices, int CoutP, const float* stats, int stats_slices, const float* fold_c,
                             const float* fold_d, float* cache, long long cache_bs, int cap, const int* lp_host, const int* step_host,
                             int B, int H, int D, int ksplit, const float* wproj, int wpCoutP, float* out, hipStream_t s);
    // op_gpt_final_ln: launch_gpt_final_ln; step_host [B] / max_steps / latents [B][C][lat_cs] (may be null) make the control block
    void op_gpt_final_ln(const float* res, const float* bias, const float* parts, int in_slices, int in_stride, int B, const float* g1,
                         const float* b1, const float* g2, const float* b2, float* y, int C, const int* step_host, int max_steps,
                         float* latents, int lat_cs, hipStream_t s);
    void op_ln_fold_vectors(const float* W, int K, int CoutP, const float* gamma, const float* beta, const float* bias, float* c, float* d,
                            hipStream_t s);
    // op_kv_to_cache: launch_kv_to_cache on qkv [B][3 C][L], lens HOST [B] in [0, min(L, cap)] -> cache [B][cache_bs >= 2 C cap]
    void op_kv_to_cache(const float* qkv, const int* lens_host, int B, int C, int L, float* cache, long long cache_bs, int cap, hipStream_t s);
    // ---- stage C
    void mel_style(const MelStyleW& w, const float* mel, const int* lens_dev, const int* lens_host, int B, int T, float* g_out,
                   hipStream_t s, bool padded_batch = false);
    void op_mel_style(const char* which, const float* mel, const int* lens_host, int B, int T, float* g_out, hipStream_t s);
    void vocoder(const float* mel, const int* lens_host, int B, int T, unsigned long long seed, const int* sample_ids_host,
                 float noise_scale, const float* noise_override, float* wav, float* trace_z, hipStream_t s, int gen_chunk = 0);
    void generator(const float* z, const float* g, const int* lens_host, int B, int T, float* wav, hipStream_t s, long long z_bs = 0,
                   int z_cs = 0);
    void op_generator(const float* z, const float* g, const int* lens_host, int B, int T, float* wav, hipStream_t s);
    bool rb_fused_ok(const GenStageW& st, int ch) const;
    void rb_fused(const GenStageW& st, const float* x, float* y, int ch, const int* lens, int B, int T, int branch_mask, float scale, hipStream_t s);
    void op_resblock1(int stage, int branch, const float* x, const int* lens_host, int B, int T, float* y, hipStream_t s);
    // flow 0 .. 3: the WaveNet of that coupling layer; flow -1: enc_q's 16-layer WaveNet
    void op_wn(int flow, const float* h, const float* g, const int* lens_host, int B, int T, float* out, hipStream_t s);
    // ---- the flow-VAE stage forward (SynthesizerTrn.forward_flowvae, vqvae/model_24k.py:706-737); needs enc_q in the bound blob
    // enc_q: spec [B, spec_channels, T], g [B, gin] -> z, m_q, logs_q [B, inter, T] (zeros beyond each row's length); noise [B, inter, T]
    // or null: Philox STAGE_POSTERIOR keyed (seed, sample_ids[b])
    void posterior_encode(const float* spec, int spec_ch, const int* lens_host, const float* g, int B, int T, const float* noise, unsigned long long seed,
                          const int* sample_ids_host, float* z, float* m_q, float* logs_q, hipStream_t s);
    // flow(z, mask, g) in the forward direction: C0, Flip, C2, Flip, C4, Flip, C6, Flip -> z_p [B, inter, T], zero tails
    void flow_forward(const float* z, const float* g, const int* lens_host, int B, int T, float* z_p, hipStream_t s);
    void slice_segments(const float* x, const int* ids_host, int B, int C, int T, int seg, float* out, hipStream_t s);
    void kl_loss(const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, const int* lens_host, int B, int C, int T,
                 float* out, hipStream_t s);
    // the whole stage in one stage-C arena and one range-check ticket: ref_enc, enc_p, enc_q, flow, segment slice, generator
    void flowvae_forward(const float* mel, const float* spec, int spec_ch, const int* lens_host, int B, int T, const float* noise, unsigned long long seed,
                         const int* sample_ids_host, const int* ids_slice_host, int seg, float* o, float* z, float* z_p, float* m_p,
                         float* logs_p, float* m_q, float* logs_q, float* quantized, hipStream_t s);
    // ---- the flow-VAE stage's losses (model_disc.hip; include/detail_hip.h has the contracts)
    void bind_discriminator(const void* blob, size_t nbytes, const char* const* names, const unsigned long long* offsets,
                            const unsigned long long* numels, int n, hipStream_t stream);
    void disc_forward(const float* y, const float* y_hat, int B, int t, float* maps, hipStream_t s);
    void disc_losses(int n_maps, const float* const* r, const float* const* g, const long long* map_numel, int n_scores,
                     const float* const* dr, const float* const* dg, const long long* score_numel, float* out, hipStream_t s);
    void spec_to_mel(const float* spec, int B, int spec_ch, int T, float* mel_out, hipStream_t s);
    void op_conv1d_grouped(const float* x, const float* w, const float* bias, int B, int Cin, int Tin, int Cout, int groups, int K, int stride,
                           int pad, float slope, float* y, hipStream_t s);
    void op_period_split(const float* wav, int B, int t, int p, float* out, hipStream_t s);
    void flowvae_stage_losses(const float* mel, const float* spec, int spec_ch, const int* lens_host, int B, int T, const float* noise,
                              unsigned long long seed, const int* sample_ids_host, const int* ids_slice_host, int seg, const float* wav, int L,
                              float* o, float* z, float* z_p, float* m_p, float* logs_p, float* m_q, float* logs_q, float* quantized,
                              float* work, float* losses, hipStream_t s);
    void op_enc_p(const float* mel, const int* lens_host, int B, int T, float* m_p, float* logs_p, hipStream_t s);
    void enc_p_fwd(const float* mel, const int* dl, int B, int T, float* x, float* y, float* qkv, float* att, float* ffn, float* relk, float* ml,
                   float* stats, hipStream_t s, bool padded_batch = false);
    // ---- VQ decode path (infer_gpt)
    void vq_decode(const int* codes_host, const int* ncodes_host, int nmax, const float* refer, const int* refer_lens_host, int Tr,
                   int B, float* mel_out, hipStream_t s, const float* g_in = nullptr);
    // ---- prompt front-end
    void resample(const float* x, int B, int L, const float* kernel, int orig, int neu, int width, float* y, int Lout, hipStream_t s);
    void mel_spectrogram(const float* wav, const int* lens_host, int B, int L, int n_fft, int hop, float* mel_out, int Tmax, hipStream_t s,
                         float* spec_out = nullptr);
    // SynthesizerTrn.encode: mel [B,128,T] -> codes DEVICE int32 [B][nmax] (nmax = ceil(ceil(T/2)/2)), optional x_vq [B,768,nmax]
    void vq_encode(const float* mel, const int* lens_host, int B, int T, int* codes_out, float* xvq_out, hipStream_t s);
    // ---- unit ops used by the parity tests
    void op_attention_block(const char* prefix, const float* x, const int* lens_host, int B, int C, int T, float* y, hipStream_t s);
    void op_resblock(const char* prefix, const float* x, const int* lens_host, int B, int T, int step, float* y, hipStream_t s);
    void op_conv1d(const char* name, const float* x, const int* lens_in_host, int B, int Cin, int Tin, int Cout, int KW, int stride,
                   int dil, int pad, int pro_act, int epi_act, int gate, int phases, const float* res, float* y, int Tout_alloc,
                   hipStream_t s);
    // ONE conv through the split-precision kernel (conv_x3.h) on packed fp32 weights `name`: x [B, Cin, T] -> y [B, rows, T] (rows = Cout,
    // Cout / 2 when gated), k = 1 or 3 with "same" padding.  Every shape the kernel or the split passes cannot take is refused before
    // anything is launched; `chosen` receives what the launcher picked.
    void op_conv1d_x3(const char* name, const float* x, const int* lens_host, int B, int Cin, int T, int Cout, int KW, int epi_act,
                      float out_scale, int gate, const float* badd, const float* res, int p1, int ksplit_max, float* y, ConvX3Launch* chosen,
                      hipStream_t s);
    // The trunk attention's split-precision path alone: the 1 x 1 qkv conv `name` (144 H rows) writing the operand images, then
    // flash_attn_x3b on them -> y (the proj conv's input planes, or fp32 rows with out_f32); img_out (may be null): a copy of the images.
    void op_attention_x3(const char* name, const float* x, const int* lens_host, int B, int Cin, int T, int H, const float* bias_tab, int p1,
                         int out_f32, void* y, void* img_out, ConvX3Launch* conv_chosen, AttnX3Launch* attn_chosen, hipStream_t s);
    // ONE launch_flash_attention (flash_attn_kernel<D, MODE> of attention.hip) on the caller's fp32 rows qkv [B, rows, cs >= T] ->
    // y [B, H D, T] (+ ml [B, H, T, 2] unless null), columns < len only; at most one of bias_tab [H, 129], causal, band [B, H, T, 2 W + 1].
    void op_attention(const float* qkv, const int* lens_host, int B, int rows, int cs, int T, int H, int D, int q_off, int k_off, int v_off,
                      int head_stride, float scale, const float* bias_tab, int causal, const float* band, int band_w, float* y, float* ml,
                      hipStream_t s);
    // enc_p's windowed relative-position attention alone, with enc_p_fwd's strides: rel_key -> band-mode flash kernel (ml_out) ->
    // rel_value on qkv [B, 3 H D, T] (blocks [Q | K | V]), ek / ev [2 W + 1, D] -> y [B, H D, T], relk [B, H, T, 2 W + 1], ml [B, H, T, 2].
    void op_attention_rel(const float* qkv, const int* lens_host, int B, int T, int H, int D, const float* ek, const float* ev, int W,
                          float scale, float* y, float* relk, float* ml, hipStream_t s);
    void op_philox_normal(float* out, int n, int B, unsigned long long seed, const int* sample_ids_host, int stage, int step,
                          hipStream_t s);

    void set_option(const std::string& key, int value) {
        if (key == "two_streams") opt_two_streams_ = value != 0;
        else if (key == "conv_x3") {
            DTTS_REQUIRE(value != 0 || !opt_trunk_fp16_, "conv_x3 = 0 (exact fp32 kernels) has no trunk_fp16 mode: set trunk_fp16 = 0 first");
            opt_conv_x3_ = value != 0;
        }
        else if (key == "trunk_fp16") {
            DTTS_REQUIRE(value == 0 || value == 1, "trunk_fp16: 0 or 1");
            DTTS_REQUIRE(value == 0 || use_x3(), "trunk_fp16 = 1 needs the split-precision kernels (conv_x3 = 1): the exact fp32 kernels have no one-product mode");
            opt_trunk_fp16_ = value != 0;     // (a kernel choice made at launch time: the only captured graphs, stage A's decode graphs, hold no trunk launch)
        }
        else if (key == "gpt_graph") opt_gpt_graph_ = value != 0;
        else if (key == "x3_range_check") opt_range_check_ = value != 0;
        else if (key == "gpt_token_kernel") { opt_gpt_token_ = value != 0; if (value != 0) tok_failed_ = false; gpt_drop_graphs(); }
        // 0: the chain's attention leaves key-split records and a GP_ATTN GEMV projects them (the form of any model that is not 16 x 48
        // with a 768-column projection); latched per session at prefill.  DTTS_GPT_FUSE_PROJ, when set, wins
        else if (key == "gpt_fuse_proj") { DTTS_REQUIRE(value == 0 || value == 1, "gpt_fuse_proj: 0 or 1"); opt_gpt_fuse_proj_ = value != 0; gpt_drop_graphs(); }
        else if (key == "gpt_token_exclusive_cu") { opt_tok_exclusive_ = value != 0; gpt_drop_graphs(); }
        else if (key == "gpt_token_min_rows") { DTTS_REQUIRE(value == 1 || value == 4 || value == 8, "gpt_token_min_rows: 1, 4 or 8"); opt_tok_min_rows_ = value; gpt_drop_graphs(); }
        else if (key == "gpt_token_wgs") { DTTS_REQUIRE(value == 128 || value == 64 || value == 32, "gpt_token_wgs: 128, 64 or 32"); opt_tok_wgs_ = value; gpt_drop_graphs(); }
        else if (key == "gpt_token_fault") opt_tok_fault_ = value;       // test hook: the n-th token launch from now on times out
        else if (key == "gpt_token_fault_eos") opt_tok_fault_eos_ = value;   // ... and leaves every row flagged finished (a spurious stop token)
        // test hook: a prompted session's mel stream is [8192, c_1 .. c_m] (no fill id 1 in front, no stop token behind): what a tortoise
        // session holds after m forced decode steps, so that the prefill route can be compared with the step route
        else if (key == "gpt_prompt_raw") opt_prompt_raw_ = value != 0;
        // test hook: a beam session leaves the KV cache where it is (rows keep their own past instead of their parent's)
        else if (key == "gpt_beam_skip_reorder") { opt_beam_skip_reorder_ = value != 0; gpt_drop_graphs(); }
        else if (key == "cfg_streams") opt_cfg_streams_ = value < 0 ? 0 : value;
        else if (key == "conv_cols") opt_conv_cols_ = value != 0;
        else if (key == "uncond_cache_mb") set_uncond_cache_mb(value);      // budget of the unconditional code-path cache; 0 = off, its block freed
        else if (key == "voc_chain_planes") opt_voc_chain_ = value != 0;
        else if (key == "voc_x3") opt_voc_x3_ = value != 0;                 // 0: stage C on the exact fp32 kernels only (the trunk keeps conv_x3's choice)
        else if (key == "x3_fault") opt_x3_fault_ = value;                  // test hook: the n-th stage-C ticket from now on is raised as saturated
        else if (key == "attn_ksplit_cus") set_attn_ksplit_cus(value);
        else if (key == "attn_ksplit") set_attn_ksplit(value);             // process-wide: key split of the trunk attention's small launches (attention.h)
        else if (key == "ln_reg") set_ln_channels_reg(value != 0);          // process-wide: the register-resident channel LayerNorm (ops.h)
        // process-wide: the small-launch tile rule of the exact fp32 conv (conv_gemm.h).  A kernel choice made at launch time; the only
        // captured graphs, stage A's decode graphs, hold no conv_gemm launch (the prefill, which does, is never captured): nothing to drop
        else if (key == "conv_small_tiles") set_conv_small_tiles(value);
        else if (key == "conv_stages") set_conv_stages(value);               // process-wide: LDS stages of the split-precision conv (conv_x3.h); a launch-time choice like the above
        else throw Error(-1, "unknown option '" + key + "'");
    }
    int get_option(const std::string& key) const {      // the options a caller restores after a per-call override
        if (key == "conv_x3") return use_x3() ? 1 : 0;
        if (key == "trunk_fp16") return opt_trunk_fp16_ ? 1 : 0;
        if (key == "gpt_fuse_proj") return opt_gpt_fuse_proj_ ? 1 : 0;
        throw Error(-1, "option '" + key + "' cannot be read back");
    }
    std::string last_error;
    dtts_config cfg;
    int device;

private:
    friend struct Stage;
    const float* W(const std::string& name, size_t numel) const;
    const float* Wopt(const std::string& name, size_t numel) const;
    PackedConv conv(const std::string& name, int Cin, int Cout, int KW, bool bias = true, int cout_p = 0) const;
    AttnBlockW attn_block(const std::string& prefix, int C, int H) const;
    ResBlockW res_block(const std::string& prefix, int C, int index) const;
    void resblock1_fwd(const ResBlock1W& rb, const float* x, float* tmp, float* out, int ch, const int* lens, int B, int T, hipStream_t s,
                       void* xs = nullptr);
    bool vocoder_x3() const;
    void wn_fwd(const WnW& c, float* h, const float* g, int gin, float* Gc, float* acts, float* h2, float* skip, const int* dl, int B,
                int T, hipStream_t s);
    WnW wn_w(const std::string& prefix, int n_layers) const;
    // enc_q up to stats = proj(h) * mask [B, 2 inter, T] (live columns only), and the forward flow; both carve their scratch from ws()
    // (enc_q_ws_bytes / flow_ws_bytes, which the entry point has ensured) and give it back
    void enc_q_fwd(const float* spec, int spec_ch, const float* g, const int* dl, int B, int T, float* stats, hipStream_t s);
    void flow_fwd(const float* z, const float* g, const int* dl, int B, int T, float* z_p, hipStream_t s);
    size_t enc_q_ws_bytes(int B, int T) const;
    size_t flow_ws_bytes(int B, int T) const;
    std::vector<int> stage_lens(const int* lens_host, int B, int T, const char* who) const;
    void build_diffusion(hipStream_t s);
    void build_vocoder(hipStream_t s);
    void build_gpt(hipStream_t s);
    void gpt_head_and_sample(hipStream_t s);
    // The teacher-forced pass gpt_latents and gpt_forward_losses share: conditioning encoder, [cond | text | start, codes, stop]
    // embeddings, the GPT-2 stack, ln_f and final_norm.  enc [B, C, L] (in ws(), which was sized with extra_ws_bytes to spare for the
    // caller) holds final_norm(ln_f(h)) of every column; row b has 1 + tl[b] + ml[b] live columns.
    struct GptForced {
        float* enc = nullptr;
        int L = 0;
        std::vector<int> tl, ml;         // text positions (ids + 2) and mel positions (codes + 2) of every row
    };
    // What a teacher-forced pass reads out of its attention (attn_probs.h), per selected layer right behind that layer's qkv conv:
    //   HEADS  every head's map on the row's whole [lt_b, lt_b]       -> out [n_layers][B][H][L][L]      (nq_max = nk_max = 0: set by the pass)
    //   MEAN   sum over (layer, head) of w[layer][head] P on the window queries c0_b + j (the columns that PREDICT code j, c0_b = 1 + tl_b
    //          the start-mel column), keys 1 .. tl_b ([255, text, 0])   -> out [B][nq_max][nk_max], layers accumulating in list order
    // layers and w ([n_layers][H], MEAN) HOST, checked by the entry; the pass uploads w with the windows, behind its own id checks.
    struct GptAttnRequest {
        int mode = 0;
        const int* layers = nullptr;
        int n_layers = 0;
        const float* w = nullptr;
        float* out = nullptr;
        int nq_max = 0, nk_max = 0;
    };
    // ... and what gpt_prefill_layers gets of it: the windows [B] and the weights as device arrays
    struct GptAttnCapture {
        GptAttnRequest req;
        const int *q0 = nullptr, *nq = nullptr, *k0 = nullptr, *nk = nullptr;
        const float* w = nullptr;
    };
    GptForced gpt_teacher_forced(const float* refer, const int* refer_lens_host, int Tr, const int* text_host, const int* text_lens_host,
                                 int Lt_max, const int* codes_host, const int* ncodes_host, int n_max, int B, size_t extra_ws_bytes,
                                 hipStream_t s, const float* cond_in = nullptr, const GptAttnRequest* attn = nullptr);
    // one head through gpt_score.hip over columns of lat [B][C][lat_cs] (targets range-checked by the caller), rows in groups of 16
    void score_head(const PackedConv& head, const float* lat, long long lat_bs, int lat_cs, const int* targets_host, const int* ntargets_host,
                    int n_max, int B, float* logprob_out, float* logits_out, hipStream_t s);
    void gpt_step_launches(hipStream_t s);
    hipGraphExec_t gpt_capture(int n);
    void gpt_drop_graphs();
    void build_vq();
    void build_frontend();
    void gpt_prefill_layers(float* x, const int* lens, int B, int L, float* kv_cache, long long kv_layer_stride, long long kv_bs,
                            int kv_cs, hipStream_t s, const GptAttnCapture* capture = nullptr);
    void gpt_capture_probs(const GptAttnCapture& c, int layer, const float* qkv, const int* lens, int B, int L, hipStream_t s);
    MelStyleW mel_style_w(const std::string& prefix, int n_mel, int hidden, int out) const;
    // the one place a ConvParams is laid out: x [B, cin, Ta] -> y [B, cout, Ta], T live columns, lengths `lens` (device) on both sides
    ConvParams cp(const float* x, int cin, float* y, int cout, int B, int T, int Ta, const int* lens) const;
    // ... and with an output side of its own (strided convs): x [B, cin, Tin_a] / len_in -> y [B, cout, Nout_a] / len_out
    ConvParams cp(const float* x, int cin, int Tin, int Tin_a, const int* len_in, float* y, int cout, int Nout, int Nout_a, const int* len_out,
                  int B) const;
    // the input's split-precision planes xs (made for T columns) / a residual [., ., cs] added in the epilogue
    static void with_planes(ConvParams& p, const void* xs, int T) { p.x3 = xs; p.x3_tp = x3_tp(T); }
    static void with_res(ConvParams& p, const float* res, long long bs, int cs) { p.res = res; p.res_bs = bs; p.res_cs = cs; }

    const int* upload_ints(const int* host, int n, hipStream_t s);
    // Ragged batches: build, upload and remember (per host thread, keyed by the device address of the lengths) the table of live
    // (sample, N tile) columns of a stack of `nb` samples; cp() attaches the sub-range of the samples a launch covers to every trunk
    // conv whose `lens` points into that array (conv_gemm.h ConvParams::cols).  No table when every sample fills all its tiles.
    void register_cols(const int* lens_dev, const int* lens_host, int nb, int T, hipStream_t s);

    // building blocks on [B, C, T] buffers (all lens are device pointers)
    void run_conv(const PackedConv& pc, ConvParams p, hipStream_t s, ConvX3Launch* chosen = nullptr) const;
    // what every launch of a trunk block shares: the batch, its stream and scratch, and the kernel mode
    struct TrunkIo {
        const int* lens;             // device lengths [B]
        int B, T, Ta;                // samples, live columns, allocated columns of the [B, C, Ta] buffers
        hipStream_t s;
        float* ab;                   // GroupNorm coefficients [B, C, 2] of the exact fp32 path
        void* xs = nullptr;          // scratch for the split-precision input planes (x3_bytes(B, C, T)); null -> exact fp32 MFMA path
        bool p1 = false;             // option "trunk_fp16" covers this block: one fp16 product (ConvParams::p1 / AttnParams::p1) instead of three
        const int* step_idx = nullptr;   // ResBlock: per-sample step (device) of a batch whose samples sit at different sampling steps
    };
    // the norm in front of a block's first conv: planes of act(GN(x)) in io.xs (x3), else coefficients in io.ab for the conv's prologue
    void norm_input(const float* x, int C, const float* gamma, const float* beta, int act, bool x3, const TrunkIo& io);
    void attention_block(const AttnBlockW& w, const float* x, float* y, float* qkv, float* att, const TrunkIo& io);
    void res_block_fwd(const Schedule& sc, const ResBlockW& w, const float* x, float* h1, float* y, int step, const TrunkIo& io);
    // its two halves: h1 = conv1(SiLU(GN(x))) | y = x + conv3(SiLU(AdaGN(h1))), where alone the timestep enters.  bmod != 0: sample b reads
    // h1 and x of sample b % bmod (bidx [B]: that index on the device, for the exact fp32 conv)
    void res_block_front(const ResBlockW& w, const float* x, float* h1, const TrunkIo& io);
    void res_block_back(const Schedule& sc, const ResBlockW& w, const float* h1, const float* x, float* y, int step, const TrunkIo& io, int bmod = 0,
                        const int* bidx = nullptr);
    void code_half(const float* in, float* P, const TrunkIo& io);   // P = W_integ2 . in: the code half of integrating_conv
    bool use_x3() const;
    // lens2 [2B]: the stack's lengths; lens_i [B + Nu]: the integrator batch's; umap [2B]: integrator sample of stack sample b; xmap [2B]: b % B
    // lens_i_host: lens_i on the host (the B row lengths, then the Nu distinct ones)
    struct PairPlan { const int *lens2, *lens_i, *umap, *xmap; int Nu; std::vector<int> lens_i_host; };
    PairPlan plan_pair(const int* lens_host, int B, int T, hipStream_t s);
    // cbuf0: [B + Nu, C, T] = B conditional code embeddings followed by Nu unconditional inputs (one per distinct length)
    // integ (optional): [B + Nu, C, T] code-path terms P = W_integ2 . conditioning_timestep_integrator(cbuf0) of this step (precompute_integrator)
    // umap (optional, with integ): this step's [2B] code-path sample indices in place of pl.umap (CodePathTable::umap_at)
    void diff_forward_pair(const Schedule& sc, const float* x, const float* cbuf0, const PairPlan& pl, int B, int T, int step, float* out2,
                           hipStream_t s, const float* integ = nullptr, const int* umap = nullptr);
    // The integrator sees (code embedding | unconditioned embedding, timestep) only - never x_t - so its output for every sampling
    // step, and the code half of integrating_conv on it, is known before the loop starts: steps are evaluated J at a time as one batch of
    // J*(B+Nu) samples, each at its own step; the step-invariant front of its first ResBlock once.  lens_i: plan_pair's (device).
    // J (0: integ_chunk(B + Nu)): the steps per launch, for a caller that evaluates fewer unconditional rows than the call has lengths
    // and keeps the call's launch boundaries (code_path_table)
    void precompute_integrator(const Schedule& sc, const float* cbuf0, const int* lens_i, const int* lens_i_host, int B, int Nu, int T,
                               const std::vector<int>& steps, float* integ_all, hipStream_t s, int J = 0);
    // what the entry points around one diff_forward_pair share: the workspace sized for the call (+ extra_bytes, + hist_floats), the plan,
    // the sample ids (optional), cbuf0 = (code_emb, or the unconditioned embedding when null | unconditional inputs), out2 [2B, OC, T]
    // and the DPM-Solver++ history [hist_floats].  On top of it the sampling entries share, each written once (model_diffusion.hip):
    // draw_x_T, code_path_table (the table's launch rule), sampler_update (the ten strided-tensor arguments of every update kernel),
    // sample_loop (the descending loop of diff_sample_ex / diff_sample_from / diff_inpaint) and single_step (diff_step, diff_step_dpm,
    // diff_reverse_step, diff_mean_variance); diff_invert keeps its own short ascending loop on the same pieces.
    // defer_uncond: the unconditional inputs are left to code_path_table, which fills only the rows it evaluates
    struct PairCall { PairPlan pl; const int* sids; float *cbuf0, *out2, *hist; bool uncond_deferred; };
    PairCall begin_pair(const float* code_emb, const int* lens_host, const int* sample_ids_host, int B, int T, hipStream_t s,
                        size_t extra_bytes = 0, size_t hist_floats = 0, bool defer_uncond = false);
    // x_T into x [B,128,T]: Philox normals per row over its own [128, len] (pc.out2 is the compact scratch of a short row)
    void draw_x_T(float* x, const PairCall& pc, const int* lens_host, int B, int T, unsigned long long seed, hipStream_t s);
    // precompute_integrator's output for loop positions k0 .. : at(k) = position k's [B + Nu, C, T] terms (null without a table)
    // With rows served by the unconditional cache the block is [n][B + Nm] evaluated rows followed by one [n] slab per served length,
    // and umap [n][2B] holds every position's sample indices relative to at(k) (null: pl.umap, every row evaluated).
    struct CodePathTable {
        float* base = nullptr;
        int k0 = 0;
        size_t stride = 0;
        const int* umap = nullptr;
        int umap_stride = 0;
        const float* at(int k) const { return base ? base + (size_t)(k - k0) * stride : nullptr; }
        const int* umap_at(int k) const { return umap ? umap + (size_t)(k - k0) * umap_stride : nullptr; }
    };
    CodePathTable code_path_table(const Schedule& sc, const PairCall& pc, int B, int T, int k_first, int k_end, bool descending, bool pinned,
                                  hipStream_t s);
    enum { SAMPLER_DDIM_REVERSE = 3 };           // sampler_update's fourth kind, behind diff_invert / diff_reverse_step only
    void sampler_update(const Schedule& sc, const PairCall& pc, float* x, int B, int T, int sampler, float eta, int step,
                        unsigned long long seed, int pstep, const float* noise, int denorm, hipStream_t s, float* x0_out = nullptr,
                        float* x0_hist = nullptr);
    struct SampleLoop {
        int sampler = 0;                         // 0 (p), 1 (ddim), 2 (dpmsolver++: the history is the call's own)
        float eta = 0.f;
        int k_first = 0, k_end = 0;              // loop positions [k_first, k_end): position k runs step n - 1 - k
        int resample = 1;                        // evaluations of every step above 0
        const float* known = nullptr;            // inpainting blend after every update (null: none): known, keep and its two noise arrays
        const unsigned char* keep = nullptr;
        const float *known_noise = nullptr, *renoise = nullptr;
        const float* step_noise = nullptr;       // per evaluation, in place of the Philox draw
        float* x_traj = nullptr;                 // x after every evaluation
        int denorm = 0;                          // the last position's update writes the raw log-mel
    };
    void sample_loop(Schedule& sc, const SampleLoop& c, const float* code_emb, const int* lens_host, int B, int T, unsigned long long seed,
                     const int* sample_ids_host, const float* x_init, float* x, hipStream_t s);
    template <class Update>
    void single_step(Schedule& sc, const float* x, const float* code_emb, const int* lens_host, const int* sample_ids_host, int B, int T,
                     int step, bool pinned_table, hipStream_t s, Update&& update);
    void ensure_fork_events();
    // the per-row driver behind diff_forward_rows / diff_training_losses: carves rows_ws_bytes(B, C, T) of ws(), which the caller has sized
    void diff_forward_rows_s(const Schedule& sc, const float* x, const float* code_emb, const int* lens_host, int B, int T, const int* step_of_row,
                             float* out, hipStream_t s);
    size_t rows_ws_bytes(int B, int C, int T) const;
    // the integer-timestep schedule `sched_id` with t_host [B] checked against its columns; the rows' coefficients on the device
    const Schedule& loss_schedule(int sched_id, const int* t_host, int B, const char* who);
    const DiffLossCoefs* upload_loss_coefs(const Schedule& sc, const int* t_host, int B, hipStream_t s);

    std::unordered_map<std::string, std::pair<const float*, size_t>> weights_;
    bool bound_ = false;

    // diffusion
    std::vector<DiffLayerW> integ_, layers_;
    std::vector<ResBlockW> tail_;
    std::vector<AttnBlockW> latcond_, ctx_;
    PackedConv xpath_;               // inp_block composed with the x half of integrating_conv (+ both biases): built at bind time in persist_
    PackedConv integ2_, out_conv_, latcond0_, ctx0_, ctx1_, te0_, te2_;
    const float *out_gn_g_ = nullptr, *out_gn_b_ = nullptr, *code_gn_g_ = nullptr, *code_gn_b_ = nullptr, *uncond_ = nullptr;
    int n_resblocks_ = 0;
    Schedule sched0_;                // the default schedule (cfg.diff_steps), tables in persist_
    // cached schedules, most recently used first; at most MAX_SCHEDULES (an N = 200 schedule is ~20 MB at 1024 channels)
    static constexpr size_t MAX_SCHEDULES = 8;
    std::vector<std::unique_ptr<Schedule>> sched_cache_;
    int sched_next_id_ = 1;
    std::mutex sched_mu_;
    Schedule& schedule(int id);
    void diff_forward_s(Schedule& sc, const float* x, const float* code_emb, const int* lens_host, int B, int T, int step, int cond_free,
                        float* out, hipStream_t s);
    void build_ss_table(const Schedule& sc, float* ss_table, float* scratch, void* ts_dev, hipStream_t s);
    // the cached schedule with key's (kind, tmap, ftimes), else `key` itself (host tables filled) with its AdaGN table built on s; its id
    int cache_schedule(std::unique_ptr<Schedule> key, hipStream_t s);

    // vocoder
    MelStyleW ref_enc_, gpt_cond_;
    bool has_vocoder_ = false, has_gpt_ = false;
    PackedConv in_proj_, enc_out_, enc_proj_, dec_pre_, dec_cond_, dec_post_;
    std::vector<EncLayerW> enc_layers_;
    std::vector<CouplingW> flows_;
    PosteriorW enc_q_;
    bool has_enc_q_ = false;
    std::vector<GenStageW> gen_;

    // discriminator (optional, a blob of its own)
    std::unordered_map<std::string, std::pair<const float*, size_t>> disc_weights_;
    DiscW disc_;
    bool has_disc_ = false;
    const float* DW(const std::string& name, size_t numel) const;
    PackedConv disc_conv(const std::string& name, int Cin, int Cout, int KW) const;

    // gpt
    std::vector<GptLayerW> gpt_layers_;
    PackedConv mel_head_;
    PackedConv text_head_;                // optional (gpt.text_head.*): only UnifiedVoice.forward's loss mode reads it
    bool has_text_head_ = false;
    const float *lnf_g_ = nullptr, *lnf_b_ = nullptr, *fin_g_ = nullptr, *fin_b_ = nullptr;
    const float *text_emb_ = nullptr, *mel_emb_ = nullptr, *text_pos_ = nullptr, *mel_pos_ = nullptr;

    Arena gpt_persist_;                   // LayerNorm-algebra vectors (bind time)
    Arena gpt_tokw_;                      // weights repacked for the persistent token kernel (bind time)
    Arena gpt_score_ws_;                  // gpt_score's per-split partials, sized at bind time for 16 rows x gpt_max_mel_pos columns
    std::vector<GptTokenLayer> tok_layers_;   // host copy of the layer table (uploaded at bind time)
    GptTokenParams tokp_;                 // its launch parameters (weight side filled at bind time, session side at prefill)
    bool tok_ok_ = false;                 // the model has the shape the token kernel is written for
    bool opt_gpt_token_ = true;           // option "gpt_token_kernel"
    bool opt_gpt_fuse_proj_ = true;       // option "gpt_fuse_proj"
    bool opt_tok_exclusive_ = false;      // option "gpt_token_exclusive_cu": 1 = the token kernel asks for whole CUs (a CU's whole LDS).  Default 0 since round 6:
                                          // 2 x 500 headline requests through infer_stream, one run per setting, every waveform bit-identical to its
                                          // blocking infer() (profiles/r06_soak.txt), and sharing is 0.4 - 0.55 % faster
    int opt_tok_min_rows_ = 1;            // option "gpt_token_min_rows": 1-row sessions take the 1-row token kernel, <= 4 rows the 4-row one (4 / 8: the smallest instantiation allowed)
    int opt_tok_wgs_ = 128;               // option "gpt_token_wgs": workgroups of the token kernel for sessions of 5 .. 8 rows (64 / 32: gpt_token_n.hip, the same bits)
    bool tok_failed_ = false;             // an exchange timed out once: this handle stays on the chain (until the option is set again)
    int opt_tok_fault_ = 0;               // option "gpt_token_fault"
    int opt_tok_fault_eos_ = 0;           // option "gpt_token_fault_eos"
    bool opt_prompt_raw_ = false;         // option "gpt_prompt_raw"
    bool opt_beam_skip_reorder_ = false;  // option "gpt_beam_skip_reorder"
    Arena gpt_beam_in_;                   // the prompt mels of a beam group, one copy per beam row
    void gpt_beam_launches(const float* parts, int slices, const float* bias, int Vs, hipStream_t s);      // beam step + reorder behind the logits
    bool gpt_replay_failed(const GptCtl& hctl, hipStream_t s);      // a timed-out token kernel: replay the session on the chain
    // what dtts_gpt_prefill was called with, kept so that a session whose token kernel timed out can be replayed on the chain
    struct GptReplay {
        bool valid = false;
        int Tr = 0, Lt_max = 0, B = 0, lat_stride = 0;
        bool has_refer_lens = false, has_text_lens = false;
        bool has_cond = false;            // the session was given cond [B, C] instead of a prompt mel: gpt_replay_ holds that vector
        std::vector<int> refer_lens, text, text_lens, sample_ids, forced_codes, prompt_codes, prompt_lens, suppress, begin_suppress;
        std::vector<unsigned long long> row_seeds;
        std::vector<dtts_gpt_row_options> rows;         // dtts_gpt_options.row_options, and per row its two id lists ([2b], [2b + 1])
        std::vector<std::vector<int>> row_ids;
        dtts_gpt_options o;
        float* latents_cm = nullptr;
    } replay_;
    Arena gpt_replay_;                    // device copy of the prompt mel (or of the cond vector) of the running session
    bool replaying_ = false;
    bool gpt_use_token_kernel() const;
    Arena gpt_state_;                     // decode session state (fixed addresses: the captured graphs point into it)
    GptSession gs_;
    GptCtl ctl_host_;
    hipGraphExec_t gpt_graph_[2] = {nullptr, nullptr};   // [0]: a chunk of decode steps, [1]: one step
    hipStream_t sg_ = nullptr;            // capture / replay stream of the decode graphs
    hipEvent_t ev_g0_ = nullptr, ev_g1_ = nullptr;
    bool opt_gpt_graph_ = false;          // dtts_gpt_decode: replay captured hipGraphs (measured 0.8 us per kernel node SLOWER than the
                                          // same launches issued eagerly on ROCm 7.2 / MI355X: DESIGN.md section 4)

    bool opt_two_streams_ = true;
    // The unconditional code-path cache (uncond_cache.h): slabs P[n][C][T] of one (binding, schedule, length, width) in
    // one device block, produced on one call's stream and read on another's - `ready` is recorded behind the copy that fills a slot,
    // `read` behind every copy out of it; a slot is reused only once both have completed (queried, never waited for on the host).
    struct UcacheEvents { hipEvent_t ready = nullptr, read = nullptr; };
    std::mutex ucache_mu_;
    UncondCacheBook ucache_;             // its budget is set when the block is allocated, at first use
    char* ucache_mem_ = nullptr;
    std::vector<UcacheEvents> ucache_ev_;   // by slot
    size_t ucache_want_ = 0;             // option "uncond_cache_mb" in bytes (constructor: DTTS_UNCOND_CACHE_MB, default 4096)
    unsigned long long bind_gen_ = 0;    // bind_weights calls so far
    void set_uncond_cache_mb(int mb);
    void ucache_release();               // waits for the slots' events, frees the block, empties the book
    bool ucache_slot_busy(int slot);
    // May the cache serve / keep rows of this pre-pass?  Only where NO launch of it - with every unconditional row present (Bi_hi
    // samples per step) and with none (Bi_lo) - takes conv split-K or the attention's key split: there alone a row's bits do not depend
    // on what shares its launch.  n_pos steps in launches of J.
    bool integ_unsplit(int Bi_lo, int Bi_hi, int T, int n_pos, int J) const;
public:
    UncondCacheStats uncond_cache_stats();
private:
    int prof_rot_ = 0;               // precompute_integrator calls so far: rotates the chunk pairs the profiler brackets
    bool opt_voc_x3_ = true;         // stage C's split-precision kernels (ResBlock1 convs, WaveNet in_layers); 0 = exact fp32 (cannot saturate)
    int opt_x3_fault_ = 0;           // test hook (option x3_fault)
    bool opt_voc_chain_ = true;      // ResBlock1 (wide generator stages): conv epilogues write the next conv's planes (resblock1_fwd)
    bool opt_conv_cols_ = true;      // ragged batches: trunk convs launch their live (sample, N tile) columns only (register_cols)
    bool opt_range_check_ = false;      // vocoder: detect activations beyond the split-precision planes' range (synchronises)
    // Range check of the generator's split-precision planes: a ring of host-mapped flags, one slot per vocoder / generator call
    // ("ticket"), raised by the kernels and read without synchronising by vocoder_check(ticket) once the CALLER has waited for that
    // call - so a saturation fails the request that saturated, not the next one.
    static constexpr int X3_SAT_SLOTS = 8;
    int* x3_sat_ = nullptr;             // host-mapped ring [X3_SAT_SLOTS]
    int* x3_sat_ring_dev_ = nullptr;    // its device address
    int* x3_sat_dev_ = nullptr;         // the current call's slot (device address); null = check off
    long long x3_ticket_ = 0;           // ticket of the last vocoder / generator call (0: none yet)
    int* x3_sat_flag(hipStream_t s);    // new ticket; device address of its flag (null when DTTS_X3_RANGE_CHECK=0)
    void x3_sat_check(hipStream_t s);   // option x3_range_check: synchronise and report this call's saturation
public:
    long long vocoder_ticket() const { return x3_ticket_; }
    bool vocoder_check_active() const { return x3_sat_dev_ != nullptr && vocoder_x3(); }
    // one ticket per TOP-LEVEL stage-C call: vocoder() opens the scope before the flow (whose WaveNet planes can saturate too) and the
    // generator calls inside it - one per window when streamed - report into the same slot
    int x3_sat_depth_ = 0;
    struct SatScope {
        Model* m;
        hipStream_t s;
        SatScope(Model* m_, hipStream_t s_) : m(m_), s(s_) { if (m->x3_sat_depth_++ == 0) m->x3_sat_flag(s); }
        ~SatScope() { --m->x3_sat_depth_; }
        void check() { if (m->x3_sat_depth_ == 1) m->x3_sat_check(s); }
        SatScope(const SatScope&) = delete;
        SatScope& operator=(const SatScope&) = delete;
    };
    void vocoder_check(long long ticket);    // throws Error(-5) when call `ticket` saturated; the caller has waited for that call
private:
    int opt_cfg_streams_ = 0;             // chunks (= streams) the 2B-sample cond | uncond stack of a diffusion forward is cut into; 0 = by batch size
    bool opt_conv_x3_ = true;             // diffusion trunk convs on the 3 x bf16 split-precision path (conv_x3.h)
    // option "trunk_fp16" (the reference's DiffusionTts.enable_fp16, vqvae/diff_model.py:157, 299-309): layers[1:] of the trunk run
    // their convs and attention products as ONE fp16 product (ConvParams::p1 / AttnParams::p1) instead of three
    bool opt_trunk_fp16_ = false;
    Arena w3_;                            // split-precision weight copies
    Arena w3_voc_;                        // ... of the generator's wide ResBlock1 convs
    static constexpr int MAX_CFG_STREAMS = 4;
    hipStream_t sx_[MAX_CFG_STREAMS - 1] = {nullptr, nullptr, nullptr};   // extra streams of the diffusion forward
    hipEvent_t ev_fork_ = nullptr, ev_joinx_[MAX_CFG_STREAMS - 1] = {nullptr, nullptr, nullptr};

    // prompt front-end
    bool has_frontend_ = false;
    PackedConv fe_dft_, fe_mel_;
    int fe_nfft_ = 0;

    // vq decode path
    bool has_vq_ = false;
    MelStyleW vq_ref_enc_;
    PackedConv vq_up1_, vq_up2_, vq_out_;
    const float *vq_table_ = nullptr, *vq_ln_g_ = nullptr, *vq_ln_b_ = nullptr;
    bool has_vq_enc_ = false;
    PackedConv vqe_c1_, vqe_c2_, vqe_c3_, vq_proj_in_;
    const float *vqe_ln_g_ = nullptr, *vqe_ln_b_ = nullptr, *vq_embed_ = nullptr, *vq_embed_sq_ = nullptr;

    Arena ws_main_;   // per-call activations (stages B and everything else); see ws()
    Arena& ws() { Arena* o = arena_override(); return o ? *o : ws_main_; }
    Arena ws_voc_;    // stage C's own scratch (stands in for the duration of a vocoder call)
    Arena ws_gpt_;    // stage A's session prefill scratch: the next batch's decode session may run under this batch's diffusion
    Arena persist_;   // tables built at bind time
    // upload_ints: one ring PER ISSUING HOST THREAD (device ints + a pinned host mirror at the same offsets, 16 segments).  A segment
    // is reused only after everything enqueued so far on the streams that consumed it has completed (event per stream at re-entry);
    // with a ring per thread the consumers of a table were enqueued by program order before the thread laps its own ring.
    struct IntRing {
        static constexpr int SEGS = 16;
        int* dev = nullptr;
        int* pinned = nullptr;
        size_t off = 0;
        int seg = 0;
        std::vector<hipStream_t> users[SEGS];   // streams whose launches read tables of this segment (current lap)
        hipEvent_t ev = nullptr;
        unsigned long long last_use = 0;
        std::shared_ptr<std::atomic<int>> owner_alive;      // 1 while the owning host thread lives (its thread_local guard clears it)
    };
    static constexpr size_t MAX_INT_RINGS = 16;      // soft cap: from here on rings of host threads that are GONE are recycled before a new one is made
    unsigned long long ring_clock_ = 0;
    std::map<std::thread::id, std::unique_ptr<IntRing>> int_rings_;
    std::mutex ints_mu_;        // guards the map only; a ring is touched by its own thread
    IntRing& int_ring();
};

}  // namespace dtts
