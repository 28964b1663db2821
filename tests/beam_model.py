"""numpy restatement of HF's GenerationMixin._beam_search (transformers 5.15.0, do_sample=False) as csrc/gpt_beam.hip runs it.

State of U utterances x K beams, generated tokens only (the prompt is an argument: the processors see it, the bookkeeping does not):
    run_seq [U, K, G] int, run_score [U, K] f32          the running beams ([0, -1e9, ...] at the start)
    fin_seq [U, K, G] int, fin_score [U, K] f32 (-1e9), fin_flag [U, K] bool, fin_len [U, K] int          the finished set, best first
    unsat [U] bool  (is_early_stop_heuristic_unsatisfied)      done [U] bool  (an utterance that is done changes nothing more)
`step` is the 0-based index of the token being chosen: HF's cur_len = prompt_len + step.  Unwritten positions hold the fill id (= eos).
All score arithmetic is float32, in HF's order of operations.  Ties go to the lowest flat index.

`mutate` switches on ONE deliberate error (tests/test_host_beam.py shows that the fixture catches each)."""
import numpy as np

NEG = np.float32(-1.0e9)
MUTATIONS = ("k_candidates", "finished_from_2k", "penalty_on_logits", "length_off_by_one", "stale_parent", "no_stop_penalty",
             "never_length", "no_running_penalty", "heuristic_on_last")
f32 = np.float32


def init_state(U, K, G, fill):
    rs = np.full((U, K), NEG, np.float32)
    rs[:, 0] = 0.0
    return dict(run_seq=np.full((U, K, G), fill, np.int64), run_score=rs, fin_seq=np.full((U, K, G), fill, np.int64),
                fin_score=np.full((U, K), NEG, np.float32), fin_flag=np.zeros((U, K), bool), fin_len=np.zeros((U, K), np.int64),
                unsat=np.ones(U, bool), done=np.zeros(U, bool), parents=np.tile(np.arange(K), (U, 1)))


def log_softmax(x):
    x = x.astype(np.float32)
    m = x.max()
    d = x - m
    return (d - np.log(np.exp(d).sum(dtype=np.float32))).astype(np.float32)


def penalise(s, ids, rp):
    """RepetitionPenaltyLogitsProcessor on whatever scores it is handed"""
    u = np.unique(ids)
    s = s.copy()
    s[u] = np.where(s[u] < 0, s[u] * f32(rp), s[u] / f32(rp))
    return s


def ban_ngrams(s, ids, n):
    """NoRepeatNGramLogitsProcessor(n)"""
    ids = [int(i) for i in ids]
    L = len(ids)
    s = s.copy()
    if L + 1 < n:
        return s
    tail = ids[L - n + 1:] if n > 1 else []
    for i in range(L - n + 1):
        if ids[i:i + n - 1] == tail:
            s[ids[i + n - 1]] = -np.inf
    return s


def process_row(logits, ids, o, step, mutate=None):
    """log_softmax, then the processors ON THE LOG-PROBABILITIES, in the order of _get_logits_processor"""
    rp, n, eos = o.get("rp", 1.0), o.get("ngram", 0), o["eos"]
    if mutate == "penalty_on_logits":
        s = log_softmax(penalise(logits.astype(np.float32), ids, rp) if rp != 1.0 else logits)
    else:
        s = log_softmax(logits)
        if rp != 1.0:
            s = penalise(s, ids, rp)
    if n:
        s = ban_ngrams(s, ids, n)
    if step < o.get("stop_from", 0):
        s[eos] = -np.inf
    for t in o.get("suppress", ()):
        s[t] = -np.inf
    if step == o.get("begin_step", 0):
        for t in o.get("begin_suppress", ()):
            s[t] = -np.inf
    return s


def _top(scores, k):
    """indices of the k largest, ties to the lowest index"""
    return np.argsort(-scores.astype(np.float64), kind="stable")[:k]


def _div(step_len, lp):
    return f32(float(step_len) ** float(lp))


def beam_step(st, logits, prompt, step, o, mutate=None):
    """One step for every utterance.  logits [U * K, V], prompt [U, P]; o: K, G, eos, lp, es (0 False, 1 True, 2 "never") + processors.
    Returns (new state, info): info[u] = dict(cand_score, cand_beam, cand_tok [2K], stop [2K]) or None for a done utterance."""
    K, G, eos, lp, es = o["K"], o["G"], o["eos"], o["lp"], o["es"]
    U, V = st["run_seq"].shape[0], logits.shape[1]
    new = {k: v.copy() for k, v in st.items()}
    info = []
    nc = K if mutate == "k_candidates" else 2 * K
    for u in range(U):
        if st["done"][u]:
            new["parents"][u] = np.arange(K)
            info.append(None)
            continue
        acc = np.empty((K, V), np.float32)
        for k in range(K):
            ids = np.concatenate([prompt[u], st["run_seq"][u, k, :step]])
            acc[k] = process_row(logits[u * K + k], ids, o, step, mutate) + st["run_score"][u, k]
        flat = acc.reshape(-1)
        top = _top(flat, nc)
        sc, beam, tok = flat[top], top // V, top % V
        stop = (tok == eos) | (step + 1 >= G)
        run_sc = sc if mutate == "no_stop_penalty" else (sc + stop.astype(np.float32) * NEG).astype(np.float32)
        nxt = _top(run_sc, K)
        src = st["parents"][u][:len(nxt)] if mutate == "stale_parent" else beam[nxt]
        seqs = st["run_seq"][u][beam].copy()               # [nc, G] the candidates' sequences
        seqs[:, step] = tok
        new["run_seq"][u] = st["run_seq"][u][src]
        new["run_seq"][u][:, step] = tok[nxt]
        new["run_score"][u] = run_sc[nxt]
        new["parents"][u] = beam[nxt]
        # finished set: only the first K candidates may enter
        first = np.arange(nc) < (nc if mutate == "finished_from_2k" else K)
        just = stop & first
        n_len = step + 1 + (1 if mutate == "length_off_by_one" else 0)
        fs = (sc / _div(n_len, lp)).astype(np.float32)
        full = bool(st["fin_flag"][u].all()) and es == 1
        fs = (fs + f32(full) * NEG).astype(np.float32)
        fs = (fs + f32(not st["unsat"][u]) * NEG).astype(np.float32)
        if mutate != "no_running_penalty":
            fs = (fs + (~just).astype(np.float32) * NEG).astype(np.float32)
        m_sc = np.concatenate([st["fin_score"][u], fs])
        m_seq = np.concatenate([st["fin_seq"][u], seqs])
        m_flag = np.concatenate([st["fin_flag"][u], just])
        m_len = np.concatenate([st["fin_len"][u], np.full(nc, step + 1)])
        keep = _top(m_sc, K)
        new["fin_score"][u], new["fin_seq"][u], new["fin_flag"][u], new["fin_len"][u] = m_sc[keep], m_seq[keep], m_flag[keep], m_len[keep]
        # _check_early_stop_heuristic at the new length, then _beam_search_has_unfinished_sequences
        hl = G if (es == 2 and lp > 0.0) else step + 1
        if mutate == "never_length":
            hl = step + 1 if (es == 2 and lp > 0.0) else hl
        if mutate == "heuristic_on_last":
            hl = max(step, 1)
        best = new["run_score"][u, 0] / _div(hl, lp)
        worst = np.where(new["fin_flag"][u], new["fin_score"][u].min(), NEG)
        new["unsat"][u] = st["unsat"][u] and bool((best > worst).any())
        open_beam = not (bool(new["fin_flag"][u].all()) and es == 1)
        new["done"][u] = not (new["unsat"][u] and open_beam and not bool(stop.all()))
        info.append(dict(cand_score=sc, cand_beam=beam, cand_tok=tok, stop=stop))
    return new, info


def results(st, nrs, fill):
    """per utterance the best nrs finished sequences (cropped to the longest returned one over ALL utterances, as HF's batch is),
    their lengths and sequences_scores"""
    U = st["fin_seq"].shape[0]
    lens = st["fin_len"][:, :nrs]
    n = int(lens.max()) if lens.size else 0
    seqs = st["fin_seq"][:, :nrs, :n].copy()
    return seqs, lens.copy(), st["fin_score"][:, :nrs].copy()
