"""Sixteen rows, each with its own sampling settings and processors, for one launch of dtts_op_sample_logits_rows: the inputs, the NumPy
restatement's token for every (row, draw) and the margin bookkeeping that says which pairs may be compared against it.  Pure NumPy
(processor_cases.process_row + test_host_token_sampler.oracle_cdf): tests/test_host_row_sampling.py establishes the count without a
GPU, tests/test_gpu_row_sampling.py asserts the device against it."""
import numpy as np

import processor_cases as P
import test_host_token_sampler as H

ROWS = 16
DRAWS = 8
SEED = 81               # the RandomState seed of the case, chosen on the NumPy restatement alone (seeds 78 .. 81 gave 80, 96, 112, 120
                        # comparable pairs of 128): at least half of the pairs have to be comparable
COMPARED = 120          # ... and this many are: test_host_row_sampling.py counts them without a GPU, the GPU test compares as many

TOP_K = (0, 1, 5, 50)
TOP_P = (1.0, 0.95, 0.8, 0.3)
TEMP = (0.5, 0.8, 1.0, 1.7)
RP = (1.0, 1.3, 2.0)
NGRAM = (0, 2, 3, 16)


def settings(i, V):
    """row i's (params of process_row, processors) - every row differs from every other"""
    params = dict(top_k=TOP_K[i % 4], top_p=TOP_P[(i // 4) % 4], temp=TEMP[(i + i // 4) % 4], rp=RP[i % 3], mass=(0.9, 0.5, 0.7, 0.95)[i // 4] if i % 4 == 2 else 0.0)
    opts = {}
    if NGRAM[(i + 1) % 4]:
        opts["no_repeat_ngram_size"] = NGRAM[(i + 1) % 4]
    if i % 5 == 1:
        opts["suppress_tokens"] = list(range(3 + i, V - 1, 2 + i))              # wide masks, different per row
    if i == 6:
        opts["suppress_tokens"] = list(range(2, V - 1))                         # a full-width mask (ids 0, 1 and the stop token stay) ...
    if i in (0, 3, 9, 14):                                                      # (rows 0 and 14 sit AT their begin: fresh = 0)
        opts["begin_suppress_tokens"] = [V - 1, 5 + i]
    if i % 4 == 3:                                                              # (row 5: no mask at all beside row 6's full-width one)
        opts["exponential_decay_length_penalty"] = ((1, 1.3), (0, 1.05), (2, 1.6), (1, 2.0))[i // 4]
    if i % 3 == 0:
        opts["min_new_tokens"] = 1 + i % 4
    if i in (0, 5, 10):
        opts["min_p"] = (0.01, 0.05, 0.2)[i // 5]
    if i in (4, 8):
        opts["epsilon_cutoff"] = (3e-4, 2e-3)[i // 8]
    return params, opts


def row_dict(params, opts):
    """what Runtime.op_sample_logits_rows / op_sample_logits_opts take for these settings"""
    return dict(top_k=int(params["top_k"]), top_p=float(params["top_p"]), temperature=float(params["temp"]),
                repetition_penalty=float(params["rp"]), typical_mass=float(params["mass"]) or None, processors=opts)


def build(seed=SEED):
    """-> (x float32 [16, V], rows [dict(hist, fills, prompt_len)], settings [(params, opts)], uniforms float32 [DRAWS, 16]); built as
    test_gpu_processors.py::test_sixteen_different_rows_in_one_launch builds its rows (histories of 6 .. ~1600 ids)"""
    V = P.V0
    rs = np.random.RandomState(seed)
    x = (rs.randn(ROWS, V) * 2.0).astype(np.float32)
    rows, sets = [], []
    for i in range(ROWS):
        n = (4, 9, 40, 300, 1580)[i % 5] + i
        body = rs.randint(2, 14 + 3 * i, size=n)
        hist = np.concatenate([[V - 2], body, body[:1]]).astype(np.int64)
        fills = i % 4
        fresh = (0, 1, 2, 3, 5, 8, 13)[i % 7]
        rows.append(dict(hist=hist, fills=fills, prompt_len=fills + len(hist) - fresh))
        sets.append(settings(i, V))
        n_gram = sets[-1][1].get("no_repeat_ngram_size", 0)
        if n_gram:
            banned = P.banned_ngram_ids([1] * fills + hist.tolist(), n_gram)
            x[i, sorted(banned)[:3]] = x[i].max() + np.float32(1.0)             # a banned id on top: the hit decides the draw
    u = rs.rand(DRAWS, ROWS).astype(np.float32)
    return x, rows, sets, u


def row_margin(x, row, params, opts, V):
    """Smallest distance, in float64, of a quantity of this row to a cut that float32 rounding could move: the top-p cumulative sum to
    1 - top_p, the typical warper's to its mass (and its neighbouring keys to each other), p / p_max to min_p, p to epsilon."""
    from oracle import gpt as G
    plain = {k: v for k, v in opts.items() if k not in ("min_p", "epsilon_cutoff")}
    out = np.inf
    with np.errstate(all="ignore"):
        if params["top_p"] < 1.0:
            s = P.process_row(x, row, dict(params, top_p=1.0), plain, V).astype(np.float64)
            s = np.sort(s[np.isfinite(s)])
            cum = np.cumsum(np.exp(s - s.max()))
            cum /= cum[-1]
            if cum.size > 1:
                out = min(out, float(np.abs(cum[:-1] - (1.0 - params["top_p"])).min()))
        if params["mass"]:
            seen = ([1] if row["fills"] else []) + [int(i) for i in row["hist"]]
            s = G.process_logits(x, seen, repetition_penalty=params["rp"], temperature=1.0, top_k=None, top_p=1.0)
            s = P.apply_processors(s, row["hist"], row["fills"], row["prompt_len"], plain, V - 1).astype(np.float64)
            fin = np.isfinite(s)
            lp = np.full(s.size, -np.inf)
            lp[fin] = s[fin] - (s[fin].max() + np.log(np.exp(s[fin] - s[fin].max()).sum()))
            pr = np.exp(lp)
            ent = -np.sum(np.where(pr > 0, pr * np.where(fin, lp, 0.0), 0.0))
            key = np.where(fin, np.abs(-lp - ent), np.inf)
            order = np.lexsort((np.arange(s.size), key))
            cum = np.cumsum(pr[order])
            out = min(out, float(np.abs(cum[:-1] - params["mass"]).min()))
            last = int((cum < params["mass"]).sum())
            near = key[order][max(0, last - 2):last + 4]
            near = near[np.isfinite(near)]
            if near.size > 1:
                out = min(out, float(np.diff(near).min()))
        s = P.process_row(x, row, params, plain, V).astype(np.float64)
        s = s[np.isfinite(s)]
        e = np.exp(s - s.max())
        if opts.get("min_p"):
            out = min(out, float(np.abs(e - opts["min_p"]).min()))
            keep = e >= opts["min_p"]
            s, e = s[keep], e[keep]
        if opts.get("epsilon_cutoff"):
            out = min(out, float(np.abs(e / e.sum() - opts["epsilon_cutoff"]).min()))
    return out


def restatement(seed=SEED):
    """-> (want int [DRAWS, 16]: the restatement's token of every pair, ok bool [DRAWS, 16]: the pair may be compared - the row's
    margins hold (CUT_MARGIN) and the uniform sits inside a token wide enough (MIN_WIDTH, EDGE_MARGIN))"""
    x, rows, sets, u = build(seed)
    V = P.V0
    want, ok = np.zeros((DRAWS, ROWS), np.int64), np.zeros((DRAWS, ROWS), bool)
    for i in range(ROWS):
        params, opts = sets[i]
        c, lo, _ = H.oracle_cdf(P.process_row(x[i], rows[i], params, opts, V))
        sound = row_margin(x[i], rows[i], params, opts, V) > H.CUT_MARGIN
        for d in range(DRAWS):
            v = int(H.inverse_cdf(c, np.float64(u[d, i])))
            want[d, i] = v
            ok[d, i] = sound and (c - lo)[v] >= H.MIN_WIDTH and min(u[d, i] - lo[v], c[v] - u[d, i]) >= H.EDGE_MARGIN
    return want, ok
