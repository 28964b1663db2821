// Kernels of the GPT autoregressive decode loop (HBM-bound weight streaming + on-device sampler).
#pragma once
#include "common.h"

namespace dtts {

constexpr int GEMV_MAXB = 16;                // sequences per decode step (rows of the skinny GEMM): one request of <= 8, or two requests'
                                             // stage A decoded as one session (the weights stream once for both); larger batches run in groups
constexpr int GEMV_PART_FLOATS = 262144;     // per-row scratch of one split-K partial set (>= slices * CoutP for every decode GEMV)

// Device-side control block of a decode session.  Everything that changes from token to token (step) or from call to call (seed,
// sampling options, output pointers) is read from here by the kernels, so one decode step is a FIXED launch sequence with fixed
// arguments: it is captured once in a hipGraph and replayed (gpt/model.py:542-544 generate() loop -> no host work per token).
struct GptCtl {
    int step[GEMV_MAXB];          // index of the token each row generates next (0-based); advanced by the sampler
    int lp[GEMV_MAXB];            // prefix length of the row: cond (1) + text positions + start_mel (1)
    int sample_id[GEMV_MAXB];     // Philox stream id of the row
    unsigned long long seed[GEMV_MAXB];     // Philox seed of the row (rows of two requests may share a session)
    // ---- the sampling settings are the ROW's own (rows of different requests share a session); a uniform session holds its one value
    // in every slot.  The sampler runs one workgroup per row and reads slot blockIdx.x, so every value stays uniform over the workgroup.
    float repetition_penalty[GEMV_MAXB], temperature[GEMV_MAXB], top_p[GEMV_MAXB];
    int top_k[GEMV_MAXB];         // <= 0: disabled
    float typical_mass[GEMV_MAXB];      // TypicalLogitsWarper mass (HF: between the repetition penalty and the temperature); <= 0 or >= 1: off
    int suppress_eos;
    int max_steps;                // tokens to generate at most: steps >= max_steps are no-ops (a replayed graph may over-run)
    int row_max_steps[GEMV_MAXB]; // the row's own cap, 1 .. max_steps: a row whose cap is BELOW max_steps is latched finished by the step that
                                  // writes its last code (the session then ends with its slowest live row, not at the largest cap)
    const float* forced_u;        // optional [B][u_stride] uniforms replacing the Philox draw (tests)
    int u_stride;
    const int* forced_tokens;     // optional [B][f_stride] teacher-forced tokens (no sampling, still recorded)
    int f_stride;
    float* latents;               // optional [B][C][lat_cs] channel-major: column `step` receives final_norm(ln_f(h))
    long long lat_bs;
    int lat_cs;
    int pos_off[GEMV_MAXB];       // mel positions the row's prefix holds: 1 (start_mel alone) or m + 2 behind an acoustic prompt
                                  // [1, 8192, c_1 .. c_m]; the input embedding of generated token `step` sits at mel position step + pos_off
    // ---- HF's remaining decode-time logits processors (generation/logits_process.py), each behind a field that is uniform over the
    // workgroup; all zero / null = off (the sampler then does what it did without them).  "Step" is the row's ctl->step.
    int ngram[GEMV_MAXB];         // NoRepeatNGramLogitsProcessor(n), 1 .. SAMP_NGRAM_MAX; 0: off.  Needs hist (kept when ANY row's n > 0)
    int* hist;                    // [B][hist_stride] the row's ORDERED input_ids without the fill-id-1 prefix columns: hist_n0[b] ids seeded
    int hist_stride;              // at prefill (8192, an acoustic prompt's codes), then one token per step appended by the sampler
    int hist_n0[GEMV_MAXB];
    int nfill[GEMV_MAXB];         // min(n, fill ids in front of hist): the only fill ids an n-gram can reach (the prefix is not materialised)
    int stop_from[GEMV_MAXB];     // MinLength + MinNewTokensLength folded: the first step at which the stop token may be drawn
    const float* decay_mul;       // ExponentialDecayLengthPenalty: one table of float(factor^i - 1); row b owns the slice [decay_tab[b],
    int decay_tab[GEMV_MAXB];     // decay_tab[b] + decay_n[b]), indexed by i = step - decay_off[b] > 0 (clamped to the slice's last entry);
    int decay_n[GEMV_MAXB];       // decay_n[b] = 0: the row's penalty is off
    int decay_off[GEMV_MAXB];
    const unsigned char* tok_mask;      // [V] bit 0: SuppressTokens (always -inf), bit 1: SuppressTokensAtBegin (at step begin_step[b]); null: off
    int mask_stride;              // 0: one mask for the session; V: row b's mask starts at tok_mask + b * V
    int begin_step[GEMV_MAXB];
    float min_p[GEMV_MAXB];       // MinPLogitsWarper (after top-k / top-p); <= 0: off
    float eps_cutoff[GEMV_MAXB];  // EpsilonLogitsWarper (after min_p); <= 0: off
};
constexpr int SAMP_NGRAM_MAX = 16;

// lat = LN2(LN1(res + bias + sum_slices parts)) (ln_f then final_norm, gpt/model.py:173 + HF GPT2Model.ln_f) -> y [B][C] and, when
// ctl->latents is set, column ctl->step[b] of the latents tensor.  in_slices == 0: res alone.
void launch_gpt_final_ln(const float* res, const float* bias, const float* parts, int in_slices, int in_stride, int B, const float* g1,
                         const float* b1, const float* g2, const float* b2, float* y, int C, const GptCtl* ctl, hipStream_t s);

// c[n] = sum_k gamma[k] W[k][n], d[n] = sum_k beta[k] W[k][n] + bias[n]: the LayerNorm-algebra vectors of a GEMV that sits behind a LN
void launch_ln_fold_vectors(const float* W, int K, int CoutP, const float* gamma, const float* beta, const float* bias, float* c, float* d,
                            hipStream_t s);

// Decode GEMV against a K-major packed weight W[K][CoutP], workgroup form (8 waves x RPW rows x 64/256 columns), B <= 8:
//   part[slice][b][col] = sum_{k in slice} in(b, k) * W[k][col],   gemv_block_slices(K, CoutP) slices, summed by the consumer.
enum { GP_PLAIN = 0, GP_RESSUM = 1, GP_LNPARTS = 2, GP_ATTN = 3 };
constexpr int ATT_REC = 64;      // floats per (sample, head, key split) record of the decode attention: m, l, o[48], padding
struct GemvIn {
    const float* x = nullptr;        // PLAIN: input rows [B][x_stride]; RESSUM: residual rows
    int x_stride = 0;
    const float* parts = nullptr;    // RESSUM / LNPARTS: the producing GEMV's partials [in_slices][B][in_stride];
                                     // ATTN: the attention's key-split records [B][H][in_slices][ATT_REC], in_stride = head dim
    int in_slices = 0, in_stride = 0, in_act = 0;
    const float* in_bias = nullptr;  // RESSUM: bias of the producing GEMV
    const float* gamma = nullptr;    // RESSUM: weight of the LayerNorm this GEMV sits behind
    float* y_out = nullptr;          // RESSUM: the residual stream [B][K] (written by the column-block-0 workgroups)
    float* stats_out = nullptr;      // RESSUM: [slices][B][2] (sum, sum of squares) of y_out's rows
    const float* stats_in = nullptr; // LNPARTS: [stats_slices][B][2] over K_ln values per row
    int stats_slices = 0, K_ln = 0;
    const float* fold_c = nullptr;   // LNPARTS: c[k], d[k] of the producing GEMV (launch_ln_fold_vectors)
    const float* fold_d = nullptr;
};
int gemv_block_slices(int K, int CoutP);
// the instantiation launch_gemv_block takes for (K, CoutP, B): VEC columns per lane, RPW weight rows per wave, NB batch rows
struct GemvShape { int vec, rpw, nb; };
GemvShape gemv_block_shape(int K, int CoutP, int B);
void launch_gemv_block(int pro, const float* W, int K, int CoutP, const GemvIn& in, int B, float* part, hipStream_t s);

// single-query attention with c_attn's LN-algebra finish folded in (sums the qkv partials of its head, appends k/v to the cache at
// the row's position lp[b] + step[b] - 1); out = key-split records [B][H][decode_attention_splits()][ATT_REC] for a GP_ATTN GEMV
int decode_attention_splits();
void launch_decode_attention_qkv(const float* part, int slices, int CoutP, const float* stats, int stats_slices, const float* fold_c,
                                 const float* fold_d, float* cache, long long cache_bs, int cache_cs, const GptCtl* ctl, int B, int H, int D,
                                 float* out, hipStream_t s, const float* wproj = nullptr, int wpCoutP = 0, int ksplit = 0);
// wproj (K-major packed [C][wpCoutP] weight of the attention's output projection) given: the projection is applied in the same
// kernel; out = per-head partials [H][B][wpCoutP] for a GP_RESSUM GEMV with in_slices = H (no key split, no GP_ATTN GEMV)
// ksplit (split form only): key splits of this launch, 1 .. 8; 0 = decode_attention_splits()
// LDS the kernel needs for a cache of cache_cs columns (the dynamic score buffer + its static arrays), against the 64 KiB of a workgroup
bool decode_attention_fits(int cache_cs, bool fused);

// copy k,v rows of a prefill qkv buffer [B, 3C, L] into the cache (columns 0..len-1)
void launch_kv_to_cache(const float* qkv, long long bs, int cs, const int* lens, int L, int B, int C, float* cache, long long cache_bs,
                        int cache_cs, hipStream_t s);

// prefix assembly (gpt/model.py:517-526): emb[b][:, 0] = cond[b]; emb[b][:, 1+j] = text_emb[ids[b][j]] + text_pos[j];
// emb[b][:, P_b] = mel_emb[start] + mel_pos[0]; then for forced histories emb[b][:, P_b + 1 + k] = mel_emb[code_k] + mel_pos[k+1]
void launch_build_prefix(const float* cond, const int* text_ids, int text_stride, const int* text_lens, const float* text_emb,
                         const float* text_pos, const float* mel_emb, const float* mel_pos, const int* mel_ids, int mel_stride,
                         const int* mel_lens, int B, int C, int Lmax, float* emb, hipStream_t s);

// seen[b][ids[b][i]] = 1 for i < nids[b]: the repetition-penalty history a session starts with (ids DEVICE [B][stride], range-checked
// by the caller; seen is zeroed by the caller)
void launch_mark_seen(const int* ids, int stride, const int* nids, int B, int V, unsigned char* seen, hipStream_t s);

// gather column (lens[b]-1 + col_off) of [B,C,L] into [B][C]
void launch_gather_last(const float* x, long long bs, int cs, const int* lens, int col_off, int B, int C, float* y, hipStream_t s);

// HF GenerationMixin._sample logits processing + inverse-CDF multinomial of the Philox spec, one workgroup per row; the mel_head
// GEMV's finish (partials + bias) is its prologue.  Records the token, latches EOS, writes the next input embedding and advances
// ctl->step[b].
struct SamplerParams {
    const float* parts;       // mel_head partials [slices][B][Vs]  (slices = 1, bias = null: plain logits [B][Vs])
    int slices;
    const float* bias;
    int Vs, V, B;
    unsigned char* seen;      // [B][V] tokens present in the row's input_ids (fake prefix ids 1 and 8192 included)
    int* finished;            // [B]
    int* codes;               // [B][codes_stride] generated ids (stop included)
    int codes_stride;
    int eos;
    GptCtl* ctl;
    // next-step input embedding: x_next[b] = mel_emb[token] + mel_pos[step + ctl->pos_off[b]]  (may be null)
    const float* mel_emb;
    const float* mel_pos;
    float* x_next;
    int C;
    long long* trace = nullptr;   // debug: wall-clock stamps of row 0 (DTTS_SAMPLER_TRACE = n: the n-th launch), normally null
};
void launch_sampler(const SamplerParams& p, hipStream_t s);
int sampler_max_vocab();          // the largest V launch_sampler admits (from the kernel's LDS budget)

// ---- beam search (gpt_beam.hip): HF GenerationMixin._beam_search, do_sample=False, on the device.  A beam session's rows are U utterances
// x K beams (row u * K + k).  beam_step_kernel takes the sampler's place behind the logits, beam_reorder_kernel follows it.
constexpr int BEAM_MAXK = 16;                // beams per utterance at most (= rows of a session)
constexpr int BEAM_V_MAX = 12288;            // largest vocabulary of the beam step (one row's scores sit in LDS)
struct BeamParams {
    const float* parts;       // logits exactly as SamplerParams hands them: partials [slices][U * K][Vs] + bias, or plain rows
    int slices;
    const float* bias;
    int Vs, V, U, K;
    const unsigned char* seen;     // [U * K][V] ids in the row's input_ids (repetition penalty); maintained by the reorder kernel
    int* finished;            // [U * K] raised for every row of an utterance that is done (may be null)
    int eos;
    GptCtl* ctl;              // step (advanced here), max_steps = max new tokens, the processors' fields, pos_off
    const float* mel_emb;     // next input embedding of row j: mel_emb[token] + mel_pos[step + pos_off]  (x_next may be null)
    const float* mel_pos;
    float* x_next;
    int C;
    // the beam state, all DEVICE.  Sequences hold generated tokens only; unwritten positions hold the fill id the host put there.
    int *run_seq, *fin_seq;   // [U * K][seq_stride]
    int seq_stride;
    float *run_score, *fin_score;      // [U * K]: running_beam_scores ([0, -1e9, ...] at the start) / beam_scores (-1e9)
    int *fin_flag, *fin_len;  // [U * K]: is_sent_finished / generated length of the finished hypothesis
    int *unsat, *done;        // [U]: is_early_stop_heuristic_unsatisfied (1 at the start) / the utterance's loop has ended
    int *parents, *tokens;    // [U * K] out: the beam (0 .. K-1) row j continues, and its new token
    int *last_step, *ident;   // [U] out: the step this launch served (-1: none - over-run or done) / its parents are the identity
    const float* len_div;     // [max_steps + 1]: float(i ** length_penalty), the power in double as Python evaluates it
    float length_penalty;
    int early_stopping;       // 0 False, 1 True, 2 "never"
    float* cand_score;        // optional [U][2K] out (unit entry): the candidates' accumulated scores, beams and tokens, best first
    int *cand_beam, *cand_tok;
};
void launch_beam_step(const BeamParams& p, hipStream_t s);
struct BeamReorderParams {
    float* kv;                // the session's KV cache (GptTokenParams::kv layout); generated columns lp .. lp + step - 1 are moved
    long long kv_layer, kv_bs;
    int cap, NL, C;
    unsigned char* seen;      // [U * K][V]
    int V, U, K;
    const GptCtl* ctl;        // lp, hist, hist_stride, hist_n0
    const int *parents, *tokens, *last_step, *ident;
    int skip_kv;              // test hook (option gpt_beam_skip_reorder): leave the cache as it is
};
void launch_beam_reorder(const BeamReorderParams& p, hipStream_t s);

// ---- one decode token as ONE persistent kernel (gpt_token.hip): 128 resident workgroups, activations exchanged through memory as
// {value, tag} words.  Replaces the 5-launches-per-layer chain for sessions of <= 8 rows on the GPT-2 shape of the reference config.
constexpr int GPT_TOKEN_WGS = 128;
constexpr int GPT_TOKEN_MAX_LAYERS = 12;
constexpr int GPT_TOKEN_VS = 66 * GPT_TOKEN_WGS;                     // logits row stride (mel_head columns padded to 66 per workgroup)
constexpr int GPT_TOKEN_ROWS = 16;                                   // rows of a session the token kernel covers (four instantiations: 1, 4, 8 and 16)
constexpr int GPT_TOKEN_W2_WORDS = 18;                               // float4 per thread and virtual workgroup of the packed mlp c_proj (24 rows x 3 columns)
constexpr int GPT_TOKEN_N_WINDOW = 24;                               // gpt_token_n.hip: weight words (float4) a thread keeps in flight
constexpr int GPT_TOKEN_XCH_WORDS = 2 * (16 * 256 * 6 + 128 * 128 * 32);     // exchange arena of a 16-row session in 8-byte units (addressed in 16-byte words)
struct GptTokenLayer {
    const float4 *wq, *wp, *wf;      // c_attn / attention c_proj / c_fc repacked in register order (launch_gpt_token_pack 0 / 1 / 2)
    const float* w2;                 // mlp c_proj, K-major [3072][768] as bound
    const float4* w2p;               // ... and repacked in thread order for the 64 / 32-workgroup kernels (launch_gpt_token_pack 4)
    const float *bq, *bp, *bf, *b2, *g1, *be1, *g2, *be2;
};
struct GptTokenParams {
    const GptTokenLayer* L;          // [NL] in DEVICE memory (indexed by the layer loop: a by-value table would be copied to scratch)
    int NL;
    const float4* wh;                // mel_head repacked (which = 3)
    const float* bh;                 // its bias, zero-padded to GPT_TOKEN_VS
    int Vs;
    const float *lnf_g, *lnf_b, *fin_g, *fin_b;
    const float* x_in;               // [B][768] input embeddings of this token (the sampler's x_next)
    float* kv;                       // KV cache: per layer kv_layer floats, per row kv_bs, K [768][cap] | V [cap][768]
    long long kv_layer, kv_bs;
    int cap;
    const GptCtl* ctl;
    int B;
    unsigned long long* xch;         // GPT_TOKEN_XCH_WORDS words, zeroed when allocated
    float* lat;                      // [B][768] final_norm(ln_f(h))
    float* logits;                   // [B][Vs]
    int* err;                        // raised when an exchange poll times out
    unsigned* epoch;                 // launch counter (>= 1), bumped by the kernel
    long long* trace;                // debug: wall-clock stamps (DTTS_GPT_TOKEN_TRACE), normally null
    int exclusive_cu;                // ask for a CU's whole LDS: one token workgroup per CU, no LDS-using workgroup next to it
    int prio;                        // s_setprio 3 for the kernel's waves (default 1)
    int poll_nap;                    // extra sleep rounds between two polls of an exchange word (default 0)
    int ablate;                      // measurement only, results are garbage (DTTS_GPT_TOKEN_ABLATE): bit 0 = no weight loads (hops and CU hold as
                                     // they are, no weight bytes), bit 1 = no waiting at the exchanges (weight bytes as they are, no hold), bit 2 = exit at once
    int wgs;                         // 128 (gpt_token.hip) or 64 / 32 (gpt_token_n.hip: sessions of 5 .. 8 rows; the same bits on fewer CUs for longer)
    int min_rows;                    // smallest instantiation a session may take: 1 (default), 4 or 8 (e.g. 8: sessions of <= 4 rows run the 8-row kernel)
};
bool gpt_token_supported(int C, int H, int F, int NL, int V);
bool gpt_token_prepare();            // device check + kernel attributes at bind time; false = use the chain
size_t gpt_token_pack_floats(int which);
void launch_gpt_token_pack(int which, const float* W, int N, int CoutP, float* out, hipStream_t s);
void launch_gpt_token(const GptTokenParams& p, hipStream_t s);
bool gpt_token_n_prepare();          // gpt_token_n.hip: kernel attributes of the 64 / 32-workgroup instantiations
void launch_gpt_token_n(const GptTokenParams& p, hipStream_t s);      // called by launch_gpt_token when p.wgs < 128

// ---- log-probability of given codes from latents (gpt_score.hip): mel_head GEMM fused with an online log-sum-exp over V and the
// gather of the target logit; V is split over workgroups (SCORE_CHUNKS chunks of 128 packed rows each) and merged in split order
constexpr int SCORE_CHUNKS = 5;
struct ScoreParams {
    const float* lat;            // latents_cm [B][C][lat_cs]: column k = final_norm(ln_f(h)) at position k
    long long lat_bs;
    int lat_cs;
    const float *w, *bias;       // mel_head as bound: K-major [CinP][CoutP], bias [CoutP]
    int C, CinP, V, CoutP;
    const int* targets;          // DEVICE [B][n_max]
    const int* ntargets;         // DEVICE [B]
    const int* tiles;            // DEVICE [ntiles][2]: (row b, first column) of every live 128-column tile
    int B, n_max;
    float* part;                 // [splits][B][n_max][3] (max, sum, target logit): gpt_score_part_floats
    float* out;                  // [B][n_max]
    float* logits_out;           // [B][V][n_max] or null
};
int gpt_score_splits(int CoutP);
size_t gpt_score_part_floats(int B, int n_max, int CoutP);
void launch_gpt_score(const ScoreParams& p, int ntiles, hipStream_t s);      // ntiles = 0: only the zero fill of the merge pass

// the two cross-entropy means of UnifiedVoice.forward (gpt/model.py:489-491): out[i] = -mean(lp_i[0 .. n_i)), lp_i DEVICE log-probabilities
// as launch_gpt_score leaves them; fixed summation order (a function of n_i only), no atomics
void launch_gpt_loss_means(const float* lp0, int n0, const float* lp1, int n1, float* out, hipStream_t s);

}  // namespace dtts
