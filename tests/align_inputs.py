"""Inputs, NumPy references and mutation tables of the alignment tests; shared by tests/golden/make_golden_attentions.py (the reference
side) and tests/test_gpu_attn_probs.py, test_gpu_align_path.py, test_gpu_alignment.py, test_host_alignment.py.  NumPy only."""
import numpy as np

# ---------------------------------------------------------------------------------------------------------------------------------
# peaked weights: under the plain seed-0 weights the GPT's maps are almost flat (a parity test would pass with a wrong scale or a
# shifted key); multiplying the q and k columns of every c_attn by `factor` sharpens them.  Applied identically to the reference and
# to the device model; the fixture records the factor.
PEAK_FACTOR = 1.75


def peaked_gpt_weights(state, factor):
    """a copy of `state` with columns [:2C] of every gpt.gpt.h.{l}.attn.c_attn.weight ([C, 3C], HF Conv1D) and .bias ([3C]) times factor"""
    out = dict(state)
    l = 0
    while f"gpt.gpt.h.{l}.attn.c_attn.weight" in state:
        w = np.array(state[f"gpt.gpt.h.{l}.attn.c_attn.weight"], copy=True)
        b = np.array(state[f"gpt.gpt.h.{l}.attn.c_attn.bias"], copy=True)
        C = w.shape[0]
        assert w.shape == (C, 3 * C) and b.shape == (3 * C,), (w.shape, b.shape)
        w[:, : 2 * C] *= w.dtype.type(factor)
        b[: 2 * C] *= b.dtype.type(factor)
        out[f"gpt.gpt.h.{l}.attn.c_attn.weight"], out[f"gpt.gpt.h.{l}.attn.c_attn.bias"] = w, b
        l += 1
    assert l > 0, "no gpt.gpt.h.*.attn.c_attn in the state dict"
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the monotone path, restated in NumPy fp32 (csrc/align_path.hip computes the same recurrence: one fp32 add and compares per cell)
def monotone_path(score, n=None, m=None):
    """score [n_max, m_max] -> int32 path [n]: dp[0] = score[0]; dp[j][i] = score[j][i] + max_{i' <= i} dp[j-1][i'], the prefix argmax
    and the final argmax both taking the LOWEST index among equal maxima"""
    s = np.asarray(score, np.float32)
    n = s.shape[0] if n is None else int(n)
    m = s.shape[1] if m is None else int(m)
    if n == 0:
        return np.zeros((0,), np.int32)
    s = s[:n, :m]
    back = np.zeros((n, m), np.int64)
    dp = s[0].copy()
    for j in range(1, n):
        pm = np.maximum.accumulate(dp)
        first = np.concatenate([[True], dp[1:] > pm[:-1]])              # a strictly larger value opens a new argmax; ties keep the old
        arg = np.maximum.accumulate(np.where(first, np.arange(m), 0))
        back[j] = arg
        dp = (s[j] + pm).astype(np.float32)
    path = np.zeros((n,), np.int32)
    path[n - 1] = int(np.argmax(dp))                                     # np.argmax: the first (lowest) of equal maxima
    for j in range(n - 1, 0, -1):
        path[j - 1] = back[j, path[j]]
    return path


def brute_force_path_score(score):
    """(the best total, every path that reaches it) over ALL monotone paths of a tiny score matrix, in float64"""
    import itertools
    s = np.asarray(score, np.float64)
    n, m = s.shape
    best, paths = -np.inf, []
    for p in itertools.product(range(m), repeat=n):
        if any(p[j] < p[j - 1] for j in range(1, n)):
            continue
        v = sum(s[j, p[j]] for j in range(n))
        if v > best + 1e-12:
            best, paths = v, [p]
        elif abs(v - best) <= 1e-12:
            paths.append(p)
    return best, paths


PATH_SIZES = [(1, 1), (1, 5), (5, 1), (3, 7), (64, 64), (65, 257), (300, 803), (1603, 803)]
PATH_KINDS = ["diagonal", "staircase", "constant", "random"]


def path_scores(kind, n, m, seed=0):
    """fp32 score [n, m] of one kind.  diagonal: a planted ridge i = j m / n over small noise; staircase: plateaus and jumps ahead;
    constant: every row one value (all ties: the path is all zeros); random: N(0, 1) rounded to 1/8 so that sums tie now and then"""
    rs = np.random.RandomState(1000 * seed + 7 * n + m)
    if kind == "constant":
        return np.full((n, m), np.float32(-0.5)) * np.arange(1, n + 1, dtype=np.float32)[:, None]
    if kind == "random":
        return (np.round(rs.randn(n, m) * 8) / 8).astype(np.float32)
    s = (rs.rand(n, m).astype(np.float32) - 1.0) * np.float32(0.25) - np.float32(4.0)
    j = np.arange(n)
    if kind == "diagonal":
        col = (j * m) // max(n, 1)
    else:                       # staircase: hold a column for a run of codes, then jump ahead by 1 .. 5 columns
        col, c = np.zeros(n, np.int64), 0
        k = 0
        while k < n:
            run = int(rs.randint(1, 6))
            col[k:k + run] = c
            k += run
            c = min(m - 1, c + int(rs.randint(1, 6)))
    s[j, np.minimum(col, m - 1)] = np.float32(-0.125)
    return s


# ---------------------------------------------------------------------------------------------------------------------------------
# the attention-probabilities kernel: cases, data, float64 reference, mutations
PROBS_T = [1, 15, 16, 17, 63, 64, 65, 129, 200]
PROBS_H, PROBS_D = 3, 48
PROBS_SCALE = 1.0 / np.sqrt(48.0)


def probs_layout(layout, H, D):
    """-> (rows, q_off, k_off, head_stride): "head" = per head [q | k | v] (QKVAttentionLegacy), "block" = [Q | K | V] of all heads (GPT-2)"""
    return (3 * H * D, 0, D, 3 * D) if layout == "head" else (3 * H * D, 0, H * D, D)


def probs_case(T, layout):
    """One unit case: B = 3 ragged samples (lens T, ceil(T / 2), 0), H = 3; q, k [B, H, D, T] float32 with logit std about 5 - random
    rows, and on head 0 a PLANTED pattern (query t and key s one-hot on channel t mod 48 / s mod 48: logits a^2 scale where (t - s) mod
    48 == 0, else 0) that moves by a whole peak under a key shift.  Windows: sample 0 starts off any multiple of 16 and its keys reach
    past t (zeros); sample 1's queries reach past len (untouched rows); sample 2 (len 0) stays untouched."""
    rs = np.random.RandomState(100 * T + (layout == "block"))
    B, H, D = 3, PROBS_H, PROBS_D
    sig = np.sqrt(5.0)
    q = (rs.randn(B, H, D, T) * sig).astype(np.float32)
    k = (rs.randn(B, H, D, T) * sig).astype(np.float32)
    amp = np.float32(np.sqrt(8.0 / PROBS_SCALE))
    q[:, 0], k[:, 0] = 0, 0
    for t in range(T):
        q[:, 0, t % D, t] = amp
        k[:, 0, (5 * t) % D, t] = amp
    lens = [T, (T + 1) // 2, 0]
    q0 = [T // 3, lens[1] // 4, 0]
    nq = [T - q0[0], min(T - q0[1], lens[1] - q0[1] + 5), min(T, 3)]
    k0 = [min(1, T - 1), 0, 0]
    nk = [T - k0[0], T, min(T, 3)]
    rows, qo, ko, hs = probs_layout(layout, H, D)
    x = np.full((B, rows, T), np.nan, np.float32)                        # v rows and every column >= len stay NaN: never read
    for b in range(B):
        for h in range(H):
            x[b, qo + h * hs: qo + h * hs + D, : lens[b]] = q[b, h, :, : lens[b]]
            x[b, ko + h * hs: ko + h * hs + D, : lens[b]] = k[b, h, :, : lens[b]]
    return dict(T=T, layout=layout, B=B, H=H, D=D, q=q, k=k, x=x, lens=lens, q0=q0, nq=nq, k0=k0, nk=nk, rows=rows, q_off=qo, k_off=ko,
                head_stride=hs, scale=float(PROBS_SCALE))


def probs_reference(q, k, length, scale, mutation=None, window=None):
    """float64 P [H, len, len] of one sample: the causal softmax over all keys s <= t.  mutation (for the gate's sanity table):
    "no_scale", "strict_causal" (s < t; row 0 keeps key 0), "window_denominator" (renormalised over `window` = (k0, nk)), "key_shift"
    (key s + 1 in the place of key s)"""
    L = int(length)
    qq, kk = np.asarray(q, np.float64)[:, :, :L], np.asarray(k, np.float64)[:, :, :L]
    if mutation == "key_shift":
        kk = np.concatenate([kk[:, :, 1:], kk[:, :, -1:]], axis=2)
    s = np.einsum("hdt,hds->hts", qq, kk) * (1.0 if mutation == "no_scale" else scale)
    t_idx, s_idx = np.arange(L)[:, None], np.arange(L)[None, :]
    mask = s_idx < t_idx if mutation == "strict_causal" else s_idx <= t_idx
    if mutation == "strict_causal":
        mask = mask | ((t_idx == 0) & (s_idx == 0))
    if mutation == "window_denominator":
        mask = mask & (s_idx >= window[0]) & (s_idx < window[0] + window[1])
    s = np.where(mask[None], s, -np.inf)
    mx = s.max(axis=2, keepdims=True)
    mx = np.where(np.isfinite(mx), mx, 0.0)
    e = np.exp(s - mx)
    den = e.sum(axis=2, keepdims=True)
    return e / np.where(den > 0, den, 1.0)


PROBS_MUTATIONS = ["no_scale", "strict_causal", "window_denominator", "key_shift"]


def window_of(P, length, q0, nq, k0, nk):
    """the window [nq, nk] of P [H, len, len] as the kernel writes it: NaN where it writes nothing (rows t >= len), 0 at keys s > t"""
    H = P.shape[0]
    out = np.full((H, nq, nk), np.nan)
    for i in range(nq):
        t = q0 + i
        if t >= length:
            continue
        out[:, i, :] = 0.0
        hi = min(k0 + nk, t + 1)
        if hi > k0:
            out[:, i, : hi - k0] = P[:, t, k0:hi]
    return out


def probs_mutation_table(cases):
    """{mutation: the SMALLEST, over the cases, of the max-abs deviation it causes in that case's windows}: every case on its own has to
    see every mutation, so a gate has to sit far below the smallest entry.  (A case of one key - T = 1 - cannot see any of them: its
    P is 1 whatever is done to the score.  Callers leave it out and say so.)"""
    tab = {}
    for mu in PROBS_MUTATIONS:
        per_case = []
        for c in cases:
            worst = 0.0
            for b in range(c["B"]):
                L = c["lens"][b]
                if L == 0:
                    continue
                a = window_of(probs_reference(c["q"][b], c["k"][b], L, c["scale"]), L, c["q0"][b], c["nq"][b], c["k0"][b], c["nk"][b])
                m = window_of(probs_reference(c["q"][b], c["k"][b], L, c["scale"], mu, (c["k0"][b], c["nk"][b])), L, c["q0"][b], c["nq"][b],
                              c["k0"][b], c["nk"][b])
                ok = ~np.isnan(a)
                if ok.any():
                    worst = max(worst, float(np.abs(a[ok] - m[ok]).max()))
            per_case.append(worst)
        tab[mu] = min(per_case)
    return tab


# ---------------------------------------------------------------------------------------------------------------------------------
# the model-level cases of tests/golden/gpt_attentions.npz
SEED_B = 11
WEIGHT_SEED = 1          # the non-uniform head weights
WEIGHT_HEADS = 2         # ... of which this many (layer, head) pairs carry WEIGHT_SHARE; the other heads share the rest evenly
WEIGHT_SHARE = 0.9


def case_a(gpt_forced):
    """B = 2 rectangle from gpt_forced.npz (13 text ids, 12 codes, L = 30): row 0 as it is, row 1 other ids and codes (7 c + 13) mod 8192"""
    text0 = np.asarray(gpt_forced["text"], np.int64)[0]
    codes0 = np.asarray(gpt_forced["codes"], np.int64)[0]
    text1 = (text0 * 5 + 11) % 254 + 1
    return dict(refer=np.repeat(np.asarray(gpt_forced["refer"], np.float32), 2, 0), text=np.stack([text0, text1]),
                codes=np.stack([codes0, (codes0 * 7 + 13) % 8192]))


def case_b(gpt_forced):
    """B = 1, 127 ids and 127 codes from RandomState(SEED_B): L = 259 crosses the 64-, 128- and 256-column seams"""
    rs = np.random.RandomState(SEED_B)
    return dict(refer=np.asarray(gpt_forced["refer"], np.float32).copy(), text=rs.randint(1, 255, (1, 127)).astype(np.int64),
                codes=rs.randint(0, 8192, (1, 127)).astype(np.int64))


def head_weights(n_layers=10, H=16):
    """seeded non-uniform weights [n_layers, H], positive, summing to 1, CONCENTRATED: WEIGHT_HEADS seeded (layer, head) pairs carry
    WEIGHT_SHARE between them, every head an even share of the rest.  The mean over many random-weight heads is nearly flat and its
    path never leaves the start-text column; one or two heads have a shape of their own, and the path through them moves."""
    rs = np.random.RandomState(WEIGHT_SEED)
    w = np.full(n_layers * H, (1.0 - WEIGHT_SHARE) / (n_layers * H))
    idx = rs.choice(n_layers * H, WEIGHT_HEADS, replace=False)
    w[idx] += WEIGHT_SHARE * rs.dirichlet(np.ones(WEIGHT_HEADS))
    return (w / w.sum()).reshape(n_layers, H).astype(np.float32)


def path_moves(path, m):
    """does a path [n] over m columns see the path step's arguments: at least 3 distinct columns, ending in column m // 3 or later"""
    p = np.asarray(path)
    return len(set(p.tolist())) >= 3 and int(p[-1]) >= m // 3


def alignment_from_maps(maps, w, tl, n, mutation=None):
    """attn [n, tl] float64 of ONE row from its per-layer maps [n_layers, H, L, L] (float64) as text_alignment defines it: queries
    c0 + j (c0 = 1 + tl, the column that PREDICTS code j), keys 1 .. tl, sum over (layer, head) of w.  mutation: "key_shift" (keys
    2 .. tl + 1), "query_late" (queries c0 + j + 1: the input-of-code-j column), "window_denominator", "heads_reversed" (w[:, ::-1])."""
    c0 = 1 + tl
    qs = np.arange(n) + c0 + (1 if mutation == "query_late" else 0)
    k0 = 2 if mutation == "key_shift" else 1
    w = np.asarray(w, np.float64)
    if mutation == "heads_reversed":
        w = w[:, ::-1]
    win = maps[:, :, qs][:, :, :, k0:k0 + tl]                         # [n_layers, H, n, tl]
    if mutation == "window_denominator":
        win = win / win.sum(axis=3, keepdims=True)
    return np.einsum("lh,lhnt->nt", w, win)


ALIGN_MUTATIONS = ["key_shift", "query_late", "window_denominator", "heads_reversed"]


def log_scores(attn):
    """what the path runs on: log(clamp_min(attn, 1e-12)) in fp32 (torch.log of an fp32 tensor; numpy's fp32 log may differ in the last
    bit, so the device's own log is what the tests feed to both sides)"""
    return np.log(np.maximum(np.asarray(attn, np.float32), np.float32(1e-12))).astype(np.float32)
