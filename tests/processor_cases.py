"""The case table of HF's remaining decode-time logits processors (tests/golden/token_processor_edges.npz, written by
tests/golden/make_golden_processors.py from HF's own classes), and a numpy restatement of those processors.

A case is a numpy RandomState seed plus a documented transform: `case_inputs` regenerates its logits rows and, per row, HF's
input_ids as the device sees them - `fills` fill ids (1), then the ORDERED ids `hist` - and HF's prompt length `prompt_len` (fill ids
included).  The fixture stores SHA-1s, HF's kept sets and processed values, no logits.  The stop token is V - 1.

`process_row` is the restatement: oracle.gpt.process_logits' repetition penalty, then the processors here in the order of
GenerationMixin._get_logits_processor (NoRepeatNGram, MinLength, MinNewTokensLength, ExponentialDecayLengthPenalty, SuppressTokens,
SuppressTokensAtBegin), then process_logits' typical warper / temperature / top-k / top-p, then MinP and Epsilon."""
import hashlib

import numpy as np

F32 = np.float32
V0 = 8194
V1 = 65                 # <= 64 candidates whatever top-k says: the sampler's single-wave top-p path
DEFAULTS = dict(rp=2.0, temp=0.8, top_k=50, top_p=0.8, mass=0.0)
OPT_KEYS = ("no_repeat_ngram_size", "min_length", "min_new_tokens", "exponential_decay_length_penalty", "suppress_tokens",
            "begin_suppress_tokens", "min_p", "epsilon_cutoff")
FILLS = 20              # fill ids of a row unless its transform says otherwise


def _case(seed, transform, V=V0, R=3, scale=2.0, opts=None, **params):
    p = dict(DEFAULTS)
    p.update(params)
    return dict(seed=seed, transform=transform, scale=scale, V=V, R=R, params=p, opts=dict(opts or {}))


def _both(name, seed, transform, seed65=None, **kw):
    """the case at V = 8194 and at V = 65.  (Seeds of the MinP / Epsilon cases that are not the next in their row were moved on until
    no p / p_max lies within CUT_MARGIN of min_p and no p within CUT_MARGIN of epsilon: test_host_processors.py asserts it.)"""
    return {name: _case(seed, transform, **kw), name + "_V65": _case(seed65 or seed + 1000, transform, V=V1, **kw)}


CASES = {}
# ---- NoRepeatNGram.  rp = 1 unless stated: a banned id is always in input_ids, so the penalty would halve what the transform plants.
# "repeat": hist = 12 random ids + its own first n-1 ids -> the id behind them, hist[n-1], is banned; it is planted as the row's arg-max
for _n in (1, 2, 3, 5):
    CASES.update(_both(f"ng_n{_n}_argmax", 400 + _n, "repeat", rp=1.0, opts=dict(no_repeat_ngram_size=_n)))
# ... and with the penalty on: the banned id is an already penalised `seen` id (planted high enough to stay in the top 50)
CASES.update(_both("ng_n3_penalised_seen", 410, "repeat", rp=2.0, opts=dict(no_repeat_ngram_size=3)))
# a history shorter than n and one of exactly n-1 ids, no fill ids: len(input_ids) < n, nothing is banned (row 2: n ids, one window)
CASES.update(_both("ng_n5_short_history", 411, "short", rp=1.0, opts=dict(no_repeat_ngram_size=5)))
# overlapping matches: hist = a run of one id, every window matches and bans that id
CASES.update(_both("ng_n3_overlap", 412, "run", rp=1.0, opts=dict(no_repeat_ngram_size=3)))
# hist ends with n-1 ones: the window at position 0 of the fill prefix, (1, .., 1), bans id 1; the window (1, .., 1, hist[0]) bans hist[0]
CASES.update(_both("ng_n3_fill_window0", 413, "fill_tail", rp=1.0, opts=dict(no_repeat_ngram_size=3)))
# fewer fill ids (2) than n (5): input_ids = [1, 1, a, b, 1, 1, a, b] -> the window at 0 bans id 1 (row 0); one fill id: nothing (row 1)
CASES.update(_both("ng_n5_few_fills", 414, "few_fills", R=2, rp=1.0, opts=dict(no_repeat_ngram_size=5)))
# 1 600 ids over an alphabet of 12: the longest history a session holds, every thread's stride of window starts is walked twice
CASES["ng_n3_history_1600"] = _case(415, "long", R=2, rp=1.0, top_p=1.0, opts=dict(no_repeat_ngram_size=3))
CASES["ng_n2_history_1600_penalised"] = _case(416, "long", R=2, rp=2.0, top_p=1.0, opts=dict(no_repeat_ngram_size=2))
# ---- the stop token's processors: rows at the step before the first stop step, at it and behind it; the stop token is planted on top
CASES.update(_both("stop_min_new_tokens", 420, "stop_steps", rp=1.0, opts=dict(min_new_tokens=4)))
CASES.update(_both("stop_min_length", 421, "stop_steps", rp=1.0, opts=dict(min_length=FILLS + 1 + 4)))
CASES.update(_both("stop_both", 422, "stop_steps", rp=1.0, opts=dict(min_length=FILLS + 1 + 2, min_new_tokens=4)))
# ---- ExponentialDecayLengthPenalty (start 2, factor 1.3): rows 2, 3 and 10 tokens behind the prompt (off, i = 1, i = 8)
CASES.update(_both("decay_positive_stop", 430, "decay_pos", scale=0.5, rp=1.0, opts=dict(exponential_decay_length_penalty=(2, 1.3))))
CASES.update(_both("decay_negative_stop", 431, "decay_neg", scale=0.5, rp=1.0, opts=dict(exponential_decay_length_penalty=(2, 1.3))))
CASES.update(_both("decay_penalised_stop", 432, "decay_seen", scale=0.5, rp=2.0, opts=dict(exponential_decay_length_penalty=(1, 1.07))))
# ---- SuppressTokens / SuppressTokensAtBegin: the ids are the row's largest logits; rows at the first generated step and at the second
CASES.update(_both("suppress_always", 440, "suppress", R=2, opts=dict(suppress_tokens="top")))
CASES.update(_both("suppress_begin", 441, "suppress", R=2, opts=dict(begin_suppress_tokens="top")))
CASES.update(_both("suppress_both", 442, "suppress", R=2, opts=dict(suppress_tokens="top_even", begin_suppress_tokens="top_odd")))
# ---- MinP / Epsilon
CASES.update(_both("minp_topk50", 450, "plain", opts=dict(min_p=0.1)))                                        # <= 64 candidates
CASES.update(_both("minp_all_V", 451, "plain", top_k=0, top_p=1.0, opts=dict(min_p=0.05)))                    # all V candidates
CASES.update(_both("minp_after_topp", 452, "plain", top_p=0.6, opts=dict(min_p=0.2)))                         # top-p has cut already
CASES.update(_both("minp_tie_at_threshold", 453, "grid", scale=1.0, top_k=0, top_p=1.0, opts=dict(min_p=0.3)))      # tie groups on both sides
CASES.update(_both("minp_lone", 454, "dominant", opts=dict(min_p=0.5)))
CASES.update(_both("eps_topk50", 460, "plain", opts=dict(epsilon_cutoff=0.02)))
CASES.update(_both("eps_all_V", 561, "plain", seed65=1501, top_k=0, top_p=1.0, opts=dict(epsilon_cutoff=3e-3)))
CASES.update(_both("eps_after_topp", 462, "plain", top_p=0.6, opts=dict(epsilon_cutoff=0.05)))
CASES.update(_both("eps_tie_at_threshold", 463, "grid", scale=1.0, top_k=0, top_p=1.0, opts=dict(epsilon_cutoff=2e-3)))
CASES.update(_both("eps_lone", 464, "flat", scale=0.05, top_k=0, top_p=1.0, opts=dict(epsilon_cutoff=0.9)))   # every p < epsilon: the top stays
CASES.update(_both("minp_then_eps", 545, "plain", seed65=1465, top_k=0, top_p=1.0, opts=dict(min_p=0.02, epsilon_cutoff=0.01)))
# ---- everything at once
CASES.update(_both("all_together", 470, "repeat", rp=2.0, opts=dict(no_repeat_ngram_size=3, min_new_tokens=2,
                                                                   exponential_decay_length_penalty=(1, 1.2), suppress_tokens=[3],
                                                                   begin_suppress_tokens=[5], min_p=0.02, epsilon_cutoff=1e-3)))


def _plant(x, ids, rp, step=0.25):
    """ids become the row's largest logits, in the order given (what the penalty divides by is multiplied in first)"""
    top = F32(x.max())
    for i, t in enumerate(ids):
        x[t] = (top + F32(1.0 + step * i)) * F32(rp)


def case_inputs(name):
    """-> (logits float32 [R, V], rows): rows[r] = dict(hist int64 ordered ids, fills, prompt_len); see the table above for the transforms"""
    c = CASES[name]
    V, R, t, rp = c["V"], c["R"], c["transform"], c["params"]["rp"]
    n = int(c["opts"].get("no_repeat_ngram_size", 0))
    rs = np.random.RandomState(c["seed"])
    x = (rs.randn(R, V) * c["scale"]).astype(F32)
    rows = []
    for r in range(R):
        fills, prompt_len = FILLS, None
        ids = rs.randint(2, V - 1, size=12).astype(np.int64)          # (neither the fill id nor the stop token)
        if t == "repeat":
            base = np.unique(ids)[:12]
            base = rs.permutation(base)
            hist = np.concatenate([[V - 2], base, base[:max(n - 1, 0)]])
            _plant(x[r], [base[max(n - 1, 0)]], rp)
            prompt_len = fills + 1 + 2 * r                            # (matters to all_together only)
        elif t == "short":
            fills = 0
            hist = ids[:(n - 2, n - 1, n)[r]]
            if r == 2:
                hist = np.concatenate([hist[:n - 1], hist[:1]])[:n]
            _plant(x[r], hist[:2], rp)
        elif t == "run":
            hist = np.concatenate([[V - 2], ids[:3], np.full(5 + r, ids[4])])
            _plant(x[r], [ids[4]], rp)
        elif t == "fill_tail":
            fills = (30, 3, 2)[r]                                     # row 2: two fill ids, the window (1, 1, 1) does not exist
            hist = np.concatenate([[V - 2], ids[:4], [1] * (n - 1)])
            _plant(x[r], [1, V - 2], rp)
        elif t == "few_fills":
            fills = (2, 1)[r]
            hist = np.concatenate([ids[:2], [1] * fills, ids[:2]])
            _plant(x[r], [1, ids[0]], rp)
        elif t == "long":
            hist = np.concatenate([[V - 2], rs.randint(2, 14, size=1599)]).astype(np.int64)
            _plant(x[r], rs.permutation(np.arange(2, 14)), rp, step=0.02)      # the whole alphabet on top, nearly level: every ban shows
        elif t == "stop_steps":
            hist = np.concatenate([[V - 2], ids[:3 + r]])             # 3, 4, 5 tokens behind a prompt of fills + 1 ids
            prompt_len = fills + 1
            _plant(x[r], [V - 1], rp)
        elif t in ("decay_pos", "decay_neg", "decay_seen"):
            k = (2, 3, 10)[r]
            hist = np.concatenate([[V - 2], rs.randint(2, V - 1, size=k)])
            prompt_len = fills + 1
            x[r, V - 1] = F32(1.5) if t != "decay_neg" else F32(-1.5)
            if t == "decay_seen":
                hist[-1] = V - 1                                      # (a stop token inside input_ids: the penalty halves it first)
                x[r, V - 1] = F32(3.0)
        elif t == "suppress":
            hist = np.concatenate([[V - 2], ids[:r]])                 # row 0: the first generated step, row 1: the second
            prompt_len = fills + 1
        elif t == "grid":
            hist = np.concatenate([[V - 2], ids[:6]])
            x[r] = (np.round(x[r] * 4.0) / 4.0).astype(F32)
        elif t == "dominant":
            hist = np.concatenate([[V - 2], ids[:6]])
            x[r, int(rs.randint(2, V - 1))] = x[r].max() + F32(12.0)
        else:
            assert t in ("plain", "flat"), t
            hist = np.concatenate([[V - 2], ids[:6]])
        hist = np.asarray(hist, np.int64)
        rows.append(dict(hist=hist, fills=int(fills), prompt_len=int(fills + 1 if prompt_len is None else prompt_len)))
    return x, rows


def case_options(name, r, logits=None):
    """the case's options for row r with the symbolic id lists resolved: "top" = the row's six largest logits, "top_even" / "top_odd" =
    every second one of them"""
    c = CASES[name]
    o = dict(c["opts"])
    for k in ("suppress_tokens", "begin_suppress_tokens"):
        if isinstance(o.get(k), str):
            if logits is None:
                logits = case_inputs(name)[0]
            top = np.argsort(-logits[r], kind="stable")[:6]
            o[k] = sorted(int(i) for i in {"top": top, "top_even": top[0::2], "top_odd": top[1::2]}[o[k]])
    return o


def input_hash(logits, rows):
    h = hashlib.sha1()
    h.update(np.ascontiguousarray(logits, F32).tobytes())
    for r in rows:
        h.update(np.ascontiguousarray(r["hist"], np.int64).tobytes())
        h.update(np.array([r["fills"], r["prompt_len"]], np.int64).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ the restatement
def banned_ngram_ids(ids, n):
    """NoRepeatNGramLogitsProcessor on one row: the ids that would complete an n-gram already in `ids`"""
    ids = [int(i) for i in ids]
    if n <= 0 or len(ids) < n:
        return set()
    prefix = ids[len(ids) - (n - 1):] if n > 1 else []
    return {ids[i + n - 1] for i in range(len(ids) - n + 1) if ids[i:i + n - 1] == prefix}


def decay_multiplier(factor, i):
    """float32(factor ** i - 1): Python's double power and difference, rounded once (what torch multiplies the float32 |score| by)"""
    return F32(pow(float(factor), int(i)) - 1)


def apply_processors(s, hist, fills, prompt_len, opts, stop):
    """the processors between the repetition penalty and the typical warper, on penalised scores s float32 [V] (a copy is returned)"""
    s = np.array(s, F32)
    cur = int(fills) + len(hist)
    n = int(opts.get("no_repeat_ngram_size") or 0)
    if n:
        nf = min(n, int(fills))                                       # only the last min(n, fills) fill ids can matter
        seq = [1] * nf + [int(i) for i in hist]
        if cur >= n:
            for t in banned_ngram_ids(seq, n):
                s[t] = -np.inf
    if cur < int(opts.get("min_length") or 0) or cur - prompt_len < int(opts.get("min_new_tokens") or 0):
        s[stop] = -np.inf
    ed = opts.get("exponential_decay_length_penalty")
    if ed is not None and cur > ed[0] + prompt_len and np.isfinite(s[stop]):
        s[stop] = F32(s[stop] + F32(np.abs(s[stop]) * decay_multiplier(ed[1], cur - ed[0] - prompt_len)))
    for t in opts.get("suppress_tokens") or ():
        s[t] = -np.inf
    if cur == prompt_len:
        for t in opts.get("begin_suppress_tokens") or ():
            s[t] = -np.inf
    return s


def apply_warpers(s, opts):
    """MinPLogitsWarper then EpsilonLogitsWarper on filtered scores s (float32 softmax as the device forms it: exp(s - max) / Z)"""
    s = np.array(s, F32)
    for key in ("min_p", "epsilon_cutoff"):
        v = opts.get(key)
        if not v:
            continue
        with np.errstate(all="ignore"):
            e = np.where(np.isfinite(s), np.exp(s - s.max(), dtype=F32), F32(0)).astype(F32)
        p = (e / e.sum(dtype=F32)).astype(F32)
        thr = F32(v) * p.max() if key == "min_p" else F32(v)
        s[(p < thr) & (s < s.max())] = -np.inf
    return s


def process_row(x, row, params, opts, V):
    from oracle import gpt as G
    hist = row["hist"]
    seen = ([1] if row["fills"] else []) + [int(i) for i in hist]
    with np.errstate(all="ignore"):
        s = G.process_logits(x, seen, repetition_penalty=params["rp"], temperature=1.0, top_k=None, top_p=1.0)
        s = apply_processors(s, hist, row["fills"], row["prompt_len"], opts, V - 1)
        s = G.process_logits(s, [], repetition_penalty=1.0, temperature=params["temp"], top_k=params["top_k"] or None,
                             top_p=params["top_p"], typical_mass=params["mass"] or None)
        return apply_warpers(s, opts)


def restated(name, r, logits=None, rows=None):
    if logits is None:
        logits, rows = case_inputs(name)
    c = CASES[name]
    return process_row(logits[r], rows[r], c["params"], case_options(name, r, logits), c["V"])


def warper_margin(name, r, logits=None, rows=None):
    """Smallest distance, in float64, of a p / p_max to min_p and of a p to epsilon, over the tokens that enter the warper (inf for a
    case without them): above CUT_MARGIN float32 rounding cannot change the kept set."""
    if logits is None:
        logits, rows = case_inputs(name)
    c = CASES[name]
    opts = case_options(name, r, logits)
    out = np.inf
    s = process_row(logits[r], rows[r], c["params"], {k: v for k, v in opts.items() if k not in ("min_p", "epsilon_cutoff")}, c["V"])
    for key in ("min_p", "epsilon_cutoff"):
        v = opts.get(key)
        if not v:
            continue
        fin = np.isfinite(s)
        p = np.zeros(s.size, np.float64)
        p[fin] = np.exp(s[fin].astype(np.float64) - float(s[fin].max()))
        p /= p.sum()
        q = (p / p.max() - v) if key == "min_p" else (p - v)
        out = min(out, float(np.abs(q[fin]).min()))
        s = apply_warpers(s, {key: v})
    return out
