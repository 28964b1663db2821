// Beam search in the GPT decode: HF GenerationMixin._beam_search (transformers 5.15.0, do_sample=False) on the device.
// Reference: gpt/model.py:187-200 (GPT2InferenceModel._reorder_cache, which the reference ships for exactly this), :542-544 (the
// generate() call that hands num_beams / length_penalty / early_stopping on).  DESIGN.md section 4.6c.
//
// A beam session holds U utterances x K beams as U * K rows (row u * K + k, HF's repeat_interleave).  Per token two kernels take the
// sampler's place behind the logits:
//   beam_step_kernel     one workgroup per utterance: log-softmax per beam row, the processors that apply without sampling ON THE
//                        LOG-PROBABILITIES, + running_beam_scores, the top 2K of the K * V accumulated scores, then HF's bookkeeping
//                        (running beams, finished set, early-stop heuristic, loop-end test) for <= 16 rows and <= 32 candidates, the
//                        next input embeddings and the per-row parent index.  Everything stays on the device.
//   beam_reorder_kernel  makes row j the continuation of its parent: the generated columns of the KV cache, the seen flags and the
//                        n-gram history, in place.  A thread owns one position across all rows of an utterance: it reads every row's
//                        value from that row's parent, then writes them - no second cache, no other thread touches what it holds.
// Ties go to the lowest flat index (beam * V + token).  All score arithmetic is float32 in HF's order of operations.
#include <climits>

#include "gpt_kernels.h"

namespace dtts {

constexpr int BEAM_THREADS = 1024;
constexpr int BEAM_WAVES = BEAM_THREADS / 64;
constexpr int BEAM_PER = BEAM_V_MAX / BEAM_THREADS;       // scores a thread owns per row (ids tid + i * BEAM_THREADS)
constexpr int BEAM_MAXC = 2 * BEAM_MAXK;                  // candidates kept per utterance (HF's beams_to_keep with one stop token)
static_assert(BEAM_V_MAX % BEAM_THREADS == 0 && BEAM_PER <= 32, "beam step: a thread's removed-ids mask is one word");
static_assert(3 * BEAM_MAXK <= 64 && BEAM_MAXK == GEMV_MAXB, "beam step: the bookkeeping runs on one wave");

__device__ __forceinline__ float bwmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float bwsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// (a, ia) better than (b, ib): larger score, ties to the lower index; INT_MAX marks "nothing"
__device__ __forceinline__ bool beam_better(float a, int ia, float b, int ib) { return ib == INT_MAX ? ia != INT_MAX : (ia != INT_MAX && (a > b || (a == b && ia < ib))); }

__device__ __forceinline__ float beam_logit(const BeamParams& p, int row, int v) {
    if (p.slices == 1 && !p.bias) return p.parts[(long long)row * p.Vs + v];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    const float* q = p.parts + (long long)row * p.Vs + v;
    const long long ss = (long long)p.U * p.K * p.Vs;
    int sl = 0;
    for (; sl + 4 <= p.slices; sl += 4) {
        const float v0 = q[0], v1 = q[ss], v2 = q[2 * ss], v3 = q[3 * ss];
        a0 += v0; a1 += v1; a2 += v2; a3 += v3;
        q += 4 * ss;
    }
    for (; sl < p.slices; ++sl) { a0 += q[0]; q += ss; }
    return (p.bias ? p.bias[v] : 0.f) + ((a0 + a1) + (a2 + a3));
}

__global__ __launch_bounds__(BEAM_THREADS) void beam_step_kernel(const BeamParams p) {
    extern __shared__ float sv[];                        // [V] accumulated scores of the row in work
    __shared__ float red[BEAM_WAVES];
    __shared__ float wb_s[2][BEAM_WAVES];                // per-wave best of an argmax round, double-buffered: one barrier per round
    __shared__ int wb_i[2][BEAM_WAVES];
    __shared__ float c_s[BEAM_MAXK * BEAM_MAXC];         // per row its best min(2K, V) accumulated scores ...
    __shared__ int c_i[BEAM_MAXK * BEAM_MAXC];           // ... and their flat indices beam * V + token
    __shared__ float t_s[BEAM_MAXC], r_s[BEAM_MAXC], m_s[3 * BEAM_MAXK];      // top 2K; the same as running scores; merged finished scores
    __shared__ int t_i[BEAM_MAXC], t_stop[BEAM_MAXC], m_flag[3 * BEAM_MAXK], m_len[3 * BEAM_MAXK];
    __shared__ int nxt[BEAM_MAXK], keep[BEAM_MAXK], sh_par[BEAM_MAXK], sh_tok[BEAM_MAXK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x, K = p.K, V = p.V, row0 = u * K;
    GptCtl* ctl = p.ctl;
    const int step = ctl->step[row0], G = ctl->max_steps;
    if (step >= G || p.done[u]) {                        // a replayed graph may over-run; an utterance that is done changes nothing more
        if (tid == 0) p.last_step[u] = -1;
        return;
    }
    const int n_row = min(2 * K, V);                     // candidates a row can contribute
    // (a beam session is always uniform - per-row settings are refused on the host - so the utterance's first row speaks for all)
    const float rp = ctl->repetition_penalty[row0];
    const unsigned char* const tok_mask = ctl->tok_mask;
    const int ngram = ctl->ngram[row0];
    const float* const decay_row = ctl->decay_mul + ctl->decay_tab[row0];
    const int decay_n = ctl->decay_n[row0];
    int* const hist = ctl->hist;

    for (int k = 0; k < K; ++k) {
        const int row = row0 + k;
        // 1. logits (the head GEMV's finish) and their log-softmax, float32
        float x[BEAM_PER];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < BEAM_PER; ++i) {
            const int v = tid + i * BEAM_THREADS;
            x[i] = v < V ? beam_logit(p, row, v) : -INFINITY;
            mx = fmaxf(mx, x[i]);
        }
        mx = bwmax(mx);
        __syncthreads();                                 // (the previous row's last round is read by now)
        if (lane == 0) red[wave] = mx;
        __syncthreads();
        mx = red[0];
        for (int i = 1; i < BEAM_WAVES; ++i) mx = fmaxf(mx, red[i]);
        float z = 0.f;
#pragma unroll
        for (int i = 0; i < BEAM_PER; ++i)
            if (tid + i * BEAM_THREADS < V) z += expf(x[i] - mx);
        z = bwsum(z);
        __syncthreads();
        if (lane == 0) red[wave] = z;
        __syncthreads();
        z = 0.f;
        for (int i = 0; i < BEAM_WAVES; ++i) z += red[i];
        const float lse = logf(z);
        // 2. the processors, on log-probabilities (HF order; a ban commutes with the rest): repetition penalty over the row's own
        // input_ids, MinLength / MinNewTokens (stop_from), ExponentialDecayLengthPenalty, then the bans below
        const unsigned char* seen = p.seen + (long long)row * V;
        const int eos_off = (ctl->suppress_eos || step < ctl->stop_from[row]) ? p.eos : -1;
        int eos_dec = -1;
        float dmul = 0.f;
        if (decay_n > 0 && eos_off < 0) {
            const int i = step - ctl->decay_off[row];
            if (i > 0) { dmul = decay_row[i < decay_n ? i : decay_n - 1]; eos_dec = p.eos; }
        }
        const float base = p.run_score[row];
#pragma unroll
        for (int i = 0; i < BEAM_PER; ++i) {
            const int v = tid + i * BEAM_THREADS;
            if (v < V) {
                float s = __fsub_rn(__fsub_rn(x[i], mx), lse);
                if (seen[v]) s = s < 0.f ? __fmul_rn(s, rp) : s / rp;
                if (v == eos_off) s = -INFINITY;
                if (v == eos_dec) s = __fadd_rn(s, __fmul_rn(fabsf(s), dmul));
                x[i] = s;
                sv[v] = s;
            }
        }
        if (ngram > 0 || tok_mask) {
            __syncthreads();
            if (ngram > 0) {                             // NoRepeatNGram over nf fill ids (1) + hist[0 .. n0 + step), as the sampler does it
                const int* h = hist + (long long)row * ctl->hist_stride;
                const int nf = ctl->nfill[row], L = nf + ctl->hist_n0[row] + step;
#define SEQ(i) ((i) < nf ? 1 : h[(i) - nf])
                for (int i = tid; i <= L - ngram; i += BEAM_THREADS) {
                    bool same = true;
                    for (int j = 0; j < ngram - 1; ++j) same = same && SEQ(i + j) == SEQ(L - ngram + 1 + j);
                    if (same) {
                        const int t = SEQ(i + ngram - 1);
                        if (t >= 0 && t < V) sv[t] = -INFINITY;
                    }
                }
#undef SEQ
            }
            if (tok_mask) {
                const unsigned on = step == ctl->begin_step[row] ? 3u : 1u;
                for (int v = tid; v < V; v += BEAM_THREADS)
                    if (tok_mask[v] & on) sv[v] = -INFINITY;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < BEAM_PER; ++i)
                if (tid + i * BEAM_THREADS < V) x[i] = sv[tid + i * BEAM_THREADS];
        }
        // 3. + running_beam_scores (one float32 add), then the row's best n_row by repeated argmax: a thread keeps the best of its own
        // ids and rescans only when it owned the winner
#pragma unroll
        for (int i = 0; i < BEAM_PER; ++i) x[i] = __fadd_rn(x[i], base);
        unsigned removed = 0;
        float bs = 0.f;
        int bi = INT_MAX;
#pragma unroll
        for (int i = 0; i < BEAM_PER; ++i) {
            const int v = tid + i * BEAM_THREADS;
            if (v < V && beam_better(x[i], v, bs, bi)) { bs = x[i]; bi = v; }
        }
        for (int r = 0; r < n_row; ++r) {
            float ws = bs;
            int wi = bi;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float os = __shfl_xor(ws, o);
                const int oi = __shfl_xor(wi, o);
                if (beam_better(os, oi, ws, wi)) { ws = os; wi = oi; }
            }
            if (lane == 0) { wb_s[r & 1][wave] = ws; wb_i[r & 1][wave] = wi; }
            __syncthreads();
            ws = wb_s[r & 1][0];
            wi = wb_i[r & 1][0];
            for (int i = 1; i < BEAM_WAVES; ++i)
                if (beam_better(wb_s[r & 1][i], wb_i[r & 1][i], ws, wi)) { ws = wb_s[r & 1][i]; wi = wb_i[r & 1][i]; }
            if (tid == 0) { c_s[k * n_row + r] = ws; c_i[k * n_row + r] = k * V + wi; }
            if (wi != INT_MAX && (wi & (BEAM_THREADS - 1)) == tid) {
                removed |= 1u << (wi / BEAM_THREADS);
                bs = 0.f;
                bi = INT_MAX;
#pragma unroll
                for (int i = 0; i < BEAM_PER; ++i) {
                    const int v = tid + i * BEAM_THREADS;
                    if (v < V && !((removed >> i) & 1u) && beam_better(x[i], v, bs, bi)) { bs = x[i]; bi = v; }
                }
            }
        }
    }
    __syncthreads();
    // 4. the top 2K of the K * n_row kept candidates by rank (K * V >= 2K always: V >= 2)
    const int N = K * n_row, C2 = 2 * K;
    if (tid < N) {
        const float s = c_s[tid];
        const int id = c_i[tid];
        int rank = 0;
        for (int j = 0; j < N; ++j) rank += (c_s[j] > s || (c_s[j] == s && c_i[j] < id)) ? 1 : 0;
        if (rank < C2) { t_s[rank] = s; t_i[rank] = id; }
    }
    __syncthreads();
    // 5. HF's bookkeeping.  Candidate i: beam t_i / V, token t_i % V; it stops on the stop token or at max_length.
    const int es = p.early_stopping;
    if (tid < C2) {
        const int tok = t_i[tid] % V;
        const int stop = (tok == p.eos || step + 1 >= G) ? 1 : 0;
        t_stop[tid] = stop;
        r_s[tid] = __fadd_rn(t_s[tid], __fmul_rn(stop ? 1.f : 0.f, -1.0e9f));      // _get_running_beams_for_next_iteration
        // _update_finished_beams: only the first K may enter; three -1e9 terms in HF's order
        bool full = es == 1;
        for (int j = 0; j < K; ++j) full = full && p.fin_flag[row0 + j] != 0;
        const int just = (stop && tid < K) ? 1 : 0;
        float f = __fdiv_rn(t_s[tid], p.len_div[step + 1]);
        f = __fadd_rn(f, __fmul_rn(full ? 1.f : 0.f, -1.0e9f));
        f = __fadd_rn(f, __fmul_rn(p.unsat[u] ? 0.f : 1.f, -1.0e9f));
        f = __fadd_rn(f, __fmul_rn(just ? 0.f : 1.f, -1.0e9f));
        m_s[K + tid] = f;
        m_flag[K + tid] = just;
        m_len[K + tid] = step + 1;
        if (p.cand_score) {
            p.cand_score[u * C2 + tid] = t_s[tid];
            p.cand_beam[u * C2 + tid] = t_i[tid] / V;
            p.cand_tok[u * C2 + tid] = tok;
        }
    }
    if (tid < K) { m_s[tid] = p.fin_score[row0 + tid]; m_flag[tid] = p.fin_flag[row0 + tid]; m_len[tid] = p.fin_len[row0 + tid]; }
    __syncthreads();
    if (tid < C2) {                                      // the next running beams: the best K of the 2K by r_s
        int rank = 0;
        for (int j = 0; j < C2; ++j) rank += (r_s[j] > r_s[tid] || (r_s[j] == r_s[tid] && j < tid)) ? 1 : 0;
        if (rank < K) nxt[rank] = tid;
    }
    if (tid < 3 * K) {                                   // the finished set: the best K of previous K + 2K
        int rank = 0;
        for (int j = 0; j < 3 * K; ++j) rank += (m_s[j] > m_s[tid] || (m_s[j] == m_s[tid] && j < tid)) ? 1 : 0;
        if (rank < K) keep[rank] = tid;
    }
    __syncthreads();
    if (tid < K) {
        const int i = nxt[tid], src = keep[tid];
        sh_par[tid] = t_i[i] / V;
        sh_tok[tid] = t_i[i] % V;
        p.parents[row0 + tid] = t_i[i] / V;
        p.tokens[row0 + tid] = t_i[i] % V;
        p.run_score[row0 + tid] = r_s[i];
        p.fin_score[row0 + tid] = m_s[src];
        p.fin_flag[row0 + tid] = m_flag[src];
        p.fin_len[row0 + tid] = m_len[src];
        ctl->step[row0 + tid] = step + 1;                // only this workgroup reads or writes its rows' step inside this launch
    }
    __syncthreads();
    if (tid == 0) {
        // _check_early_stop_heuristic at the new length, then _beam_search_has_unfinished_sequences for this utterance alone
        const int hl = (es == 2 && p.length_penalty > 0.f) ? G : step + 1;
        const float best = __fdiv_rn(r_s[nxt[0]], p.len_div[hl]);
        float worst = INFINITY;
        bool all_fin = true, all_stop = true, ident = true;
        for (int j = 0; j < K; ++j) { worst = fminf(worst, m_s[keep[j]]); all_fin = all_fin && m_flag[keep[j]] != 0; ident = ident && sh_par[j] == j; }
        for (int j = 0; j < C2; ++j) all_stop = all_stop && t_stop[j] != 0;
        bool any = false;
        for (int j = 0; j < K; ++j) any = any || best > (m_flag[keep[j]] ? worst : -1.0e9f);
        const bool unsat = p.unsat[u] != 0 && any;
        const bool go = unsat && !(all_fin && es == 1) && !all_stop;
        p.unsat[u] = unsat ? 1 : 0;
        p.done[u] = go ? 0 : 1;
        p.last_step[u] = step;
        p.ident[u] = ident ? 1 : 0;
        if (!go && p.finished)
            for (int j = 0; j < K; ++j) p.finished[row0 + j] = 1;      // gpt_all_finished and the chunked drain work unchanged
    }
    // 6. sequences: a thread owns column t of every row; all reads, then the writes
    const int S = p.seq_stride;
    for (int t = tid; t <= step; t += BEAM_THREADS) {
        int nr[BEAM_MAXK], nf[BEAM_MAXK];
#pragma unroll
        for (int j = 0; j < BEAM_MAXK; ++j)
            if (j < K) {
                const int src = keep[j];
                if (t == step) {
                    nr[j] = sh_tok[j];
                    nf[j] = src < K ? p.fin_seq[(long long)(row0 + src) * S + t] : t_i[src - K] % V;
                } else {
                    nr[j] = p.run_seq[(long long)(row0 + sh_par[j]) * S + t];
                    nf[j] = src < K ? p.fin_seq[(long long)(row0 + src) * S + t] : p.run_seq[(long long)(row0 + t_i[src - K] / V) * S + t];
                }
            }
#pragma unroll
        for (int j = 0; j < BEAM_MAXK; ++j)
            if (j < K) {
                p.run_seq[(long long)(row0 + j) * S + t] = nr[j];
                p.fin_seq[(long long)(row0 + j) * S + t] = nf[j];
            }
    }
    // 7. next input embeddings: mel_embedding[token] + mel_pos_embedding[step + pos_off]   (gpt/model.py:134-136 with position k)
    if (p.x_next) {
        const int pos_row = step + ctl->pos_off[row0];
        for (int i = tid; i < K * p.C; i += BEAM_THREADS) {
            const int j = i / p.C, c = i - j * p.C;
            p.x_next[(long long)(row0 + j) * p.C + c] = p.mel_emb[(long long)sh_tok[j] * p.C + c] + p.mel_pos[(long long)pos_row * p.C + c];
        }
    }
}

void launch_beam_step(const BeamParams& p, hipStream_t s) {
    DTTS_REQUIRE(p.K >= 1 && p.K <= BEAM_MAXK && p.U >= 1 && p.U * p.K <= GEMV_MAXB, "beam step: 1 .. 16 beams, at most 16 rows");
    DTTS_REQUIRE(p.V >= 2 && p.V <= BEAM_V_MAX, "beam step: vocabulary outside 2 .. BEAM_V_MAX");
    const size_t lds = sizeof(float) * (size_t)((p.V + 3) & ~3);
    lds_optin(reinterpret_cast<const void*>(beam_step_kernel), (int)(sizeof(float) * BEAM_V_MAX));
    hipLaunchKernelGGL(beam_step_kernel, dim3(p.U), dim3(BEAM_THREADS), lds, s, p);
    DTTS_CHECK_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------- reorder
// grid (x, y, U): y < 2 NL: (layer, k | v) of the KV cache; y == 2 NL: the seen flags (+ the new token's); y == 2 NL + 1: the n-gram
// history (+ the new token).  The grid is fixed (sized for max_generate_length); the work is the device step's.
constexpr int REORDER_THREADS = 256;
constexpr int REORDER_XBLOCKS = 64;

__global__ __launch_bounds__(REORDER_THREADS) void beam_reorder_kernel(const BeamReorderParams p) {
    const int u = blockIdx.z, K = p.K, row0 = u * K, y = blockIdx.y;
    const int s = p.last_step[u];                        // the step the beam kernel just served: s generated columns sit in the cache
    if (s < 0) return;
    int par[BEAM_MAXK];
#pragma unroll
    for (int j = 0; j < BEAM_MAXK; ++j) par[j] = j < K ? p.parents[row0 + j] : j;
    const int gtid = blockIdx.x * REORDER_THREADS + threadIdx.x, gstride = gridDim.x * REORDER_THREADS;
    if (y < 2 * p.NL) {
        if (p.skip_kv || p.ident[u] || s == 0) return;   // identity parents: nothing moves
        const int layer = y >> 1, lp = p.ctl->lp[row0], C4 = p.C / 4;
        float* base = p.kv + (long long)layer * p.kv_layer;
        if ((y & 1) == 0) {                              // K [C][cap]: positions are contiguous, a thread takes 4 channels of one position
            for (int i = gtid; i < s * C4; i += gstride) {
                const int pos = lp + i % s, c0 = (i / s) * 4;
                float v[BEAM_MAXK][4];
#pragma unroll
                for (int j = 0; j < BEAM_MAXK; ++j)
                    if (j < K && par[j] != j) {
                        const float* q = base + (long long)(row0 + par[j]) * p.kv_bs + (long long)c0 * p.cap + pos;
#pragma unroll
                        for (int c = 0; c < 4; ++c) v[j][c] = q[(long long)c * p.cap];
                    }
#pragma unroll
                for (int j = 0; j < BEAM_MAXK; ++j)
                    if (j < K && par[j] != j) {
                        float* q = base + (long long)(row0 + j) * p.kv_bs + (long long)c0 * p.cap + pos;
#pragma unroll
                        for (int c = 0; c < 4; ++c) q[(long long)c * p.cap] = v[j][c];
                    }
            }
        } else {                                         // V [cap][C]: channels are contiguous, a thread takes one float4
            base += (long long)p.C * p.cap;
            for (int i = gtid; i < s * C4; i += gstride) {
                const int pos = lp + i / C4, c0 = (i % C4) * 4;
                float4 v[BEAM_MAXK];
#pragma unroll
                for (int j = 0; j < BEAM_MAXK; ++j)
                    if (j < K && par[j] != j)
                        v[j] = *reinterpret_cast<const float4*>(base + (long long)(row0 + par[j]) * p.kv_bs + (long long)pos * p.C + c0);
#pragma unroll
                for (int j = 0; j < BEAM_MAXK; ++j)
                    if (j < K && par[j] != j)
                        *reinterpret_cast<float4*>(base + (long long)(row0 + j) * p.kv_bs + (long long)pos * p.C + c0) = v[j];
            }
        }
    } else if (y == 2 * p.NL) {                          // seen[j][v] = seen[parent j][v] | (v is row j's new token)
        int tok[BEAM_MAXK];
#pragma unroll
        for (int j = 0; j < BEAM_MAXK; ++j) tok[j] = j < K ? p.tokens[row0 + j] : -1;
        for (int v = gtid; v < p.V; v += gstride) {
            unsigned char f[BEAM_MAXK];
#pragma unroll
            for (int j = 0; j < BEAM_MAXK; ++j)
                if (j < K) f[j] = p.seen[(long long)(row0 + par[j]) * p.V + v];
#pragma unroll
            for (int j = 0; j < BEAM_MAXK; ++j)
                if (j < K) p.seen[(long long)(row0 + j) * p.V + v] = (f[j] || v == tok[j]) ? 1 : 0;
        }
    } else {                                             // the ordered history the n-gram processor reads: generated part + the new token
        int* hist = p.ctl->hist;
        if (!hist) return;
        const int hs = p.ctl->hist_stride, n0 = p.ctl->hist_n0[row0];
        for (int t = gtid; t <= s; t += gstride) {
            int h[BEAM_MAXK];
#pragma unroll
            for (int j = 0; j < BEAM_MAXK; ++j)
                if (j < K) h[j] = t == s ? p.tokens[row0 + j] : hist[(long long)(row0 + par[j]) * hs + n0 + t];
#pragma unroll
            for (int j = 0; j < BEAM_MAXK; ++j)
                if (j < K) hist[(long long)(row0 + j) * hs + n0 + t] = h[j];
        }
    }
}

void launch_beam_reorder(const BeamReorderParams& p, hipStream_t s) {
    DTTS_REQUIRE(p.K >= 1 && p.K <= BEAM_MAXK && p.U >= 1 && p.U * p.K <= GEMV_MAXB && p.C % 4 == 0, "beam reorder: shape");
    hipLaunchKernelGGL(beam_reorder_kernel, dim3(REORDER_XBLOCKS, 2 * p.NL + 2, p.U), dim3(REORDER_THREADS), 0, s, p);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
