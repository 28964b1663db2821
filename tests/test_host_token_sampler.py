"""Edge cases of the token sampler's logits processors, pinned to the REFERENCE's HF processors (tests/golden/token_sampler_edges.npz,
written by tests/golden/make_golden_token_sampler.py): ties at the top-k threshold, 64 / 65 candidates into top-p, top_k in
{1, V-1, V, V+5}, top_p in {1, 1e-6}, a dominant token, flat rows, the repetition penalty's sign rule on a history that holds the
row's arg-max, -inf logits, the typical warper on smooth rows and on rows with -inf, and vocabularies from 2 to 9217.

This file holds (1) the case table: every case's logits and history are a numpy RandomState seed plus a documented transform, so the
fixture stores their SHA-1 and no logits row; (2) the CPU check that oracle.gpt.process_logits reproduces HF's kept set and values;
(3) the probe generator tests/test_gpu_token_sampler.py drives the device sampler with, and the CPU assertions of its exclusion
caps - a later change of the generator cannot widen what the GPU test leaves out without this file failing."""
import hashlib

import numpy as np
import pytest

F32 = np.float32
V0 = 8194
DEFAULTS = dict(rp=2.0, temp=0.8, top_k=50, top_p=0.8, mass=0.0)

# the project's margins for the fp32 resolution of the device's CDF (tests/test_gpu_fullsize.py: the peaked-logits test)
EDGE_MARGIN = 1e-5          # a probe closer than this to an edge of its token's interval is left out
MIN_WIDTH = 2e-5            # a token whose interval is narrower than this gets no probe and need not be drawn
CUT_MARGIN = 1e-5           # no cumulative probability of a case may lie this close to 1 - top_p (or to the typical mass)
# The typical warper sorts by key = | -log p - H |: a difference of two numbers near log V ~ 9 (float32 ulp 9.5e-7), H a sum of V terms.
# Two correct float32 evaluations (torch's, numpy's, the device's) differ by a few ulp there - measured: torch and numpy entropies 2 ulp
# apart, keys 3e-6 apart, which swapped two tokens at a cut.  A case must not hang on that: the keys next to the cut are >= 1e-5 apart.
KEY_MARGIN = 1e-5
MAX_EXCLUDED_MASS = 0.01    # kept tokens without a probe carry at most this much of a row's probability
MIN_PROBES = 16
N_RANDOM = 64


# ------------------------------------------------------------------------------------------------ the cases
def _case(seed, transform="plain", scale=2.0, V=V0, R=3, **params):
    p = dict(DEFAULTS)
    p.update(params)
    return dict(seed=seed, transform=transform, scale=scale, V=V, R=R, params=p)


CASES = {
    # a, b: logits on a 0.25 grid - at least 20 tokens share the 50th-largest value, top-k keeps them all (> 64 into top-p)
    "a_ties_topk_topp": _case(101, "grid", 1.0),
    "b_ties_topk_only": _case(101, "grid", 1.0, top_p=1.0),
    # c, d: no ties, exactly 64 / 65 candidates into top-p (the single-wave path's last size / the block path's first)
    "c_topp_64": _case(103, scale=4.0, top_k=64, top_p=0.999),
    "d_topp_65": _case(103, scale=4.0, top_k=65, top_p=0.999),
    "e_topk_1": _case(105, R=2, top_k=1),
    # f, g, h: flat rows (every token wide enough to be drawn), top-p off: whether the smallest token goes is all top-k decides
    "f_topk_Vm1": _case(106, scale=0.2, R=2, top_k=V0 - 1, top_p=1.0),
    "g_topk_V": _case(107, scale=0.2, R=2, top_k=V0, top_p=1.0),
    "h_topk_Vp5": _case(108, scale=0.2, R=2, top_k=V0 + 5, top_p=1.0),
    "i_topp_1": _case(109, top_p=1.0),
    "j_topp_1em6": _case(110, top_p=1e-6),
    # top_p = 1e-8: 1 - top_p is 1.0 in float32 and the whole ascending cumulative sum, its last element (exactly 1.0) included, is
    # <= the cut - ONLY the "keep at least one token" guard (HF: min_tokens_to_keep) keeps the lone token.  Once through the single-wave
    # top-p path (top-k 50: <= 64 candidates), once through the block path (top-k off: all V candidates).
    "j_topp_1em8_wave": _case(151, "lone", top_p=1e-8),
    "j_topp_1em8_block": _case(152, "lone", top_k=0, top_p=1e-8),
    "k_dominant": _case(111, "dominant"),
    "l_topp_half_flat": _case(112, scale=1.0, R=2, temp=5.0, top_k=0, top_p=0.5),
    # m, n, o: history = ids 0 and V-1, a duplicate, three tokens with negative logits, the row's arg-max.  The LAST row is shifted so that
    # every logit is negative and its three seen tokens are taken from its 20 largest: there the `x * rp` branch decides what top-k 50
    # keeps and with which values (a negative logit of a randn row never reaches the top 50, whichever way it is penalised)
    "m_penalty_2": _case(113, "penalty", rp=2.0),
    "n_penalty_1p3": _case(113, "penalty", rp=1.3),
    "o_penalty_1": _case(113, "penalty", rp=1.0),
    "p_temp_0p1": _case(116, scale=0.3, temp=0.1),
    "q_temp_1": _case(117, temp=1.0),
    "r_temp_5": _case(118, temp=5.0),
    # s: -inf at V-1, at a seen id and at 100 random ids; s_kinf: the k-th largest value itself is -inf (top-k removes nothing)
    "s_ninf": _case(119, "ninf"),
    "s_kinf": _case(150, "ninf", scale=0.2, R=2, top_k=V0 - 50, top_p=0.9),
    # t: the typical warper alone (top-k and top-p off: its whole kept set is drawn from), then once in front of the default warpers
    # (seeds picked so that no cumulative probability lies within CUT_MARGIN of the mass: test_probe_generator_caps)
    "t_smooth_0p2": _case(210, scale=0.5, R=2, mass=0.2, top_k=0, top_p=1.0),
    "t_smooth_0p9": _case(214, scale=0.5, R=2, mass=0.9, top_k=0, top_p=1.0),
    "t_smooth_0p999": _case(215, scale=0.5, R=2, mass=0.999, top_k=0, top_p=1.0),
    "t_ninf_0p2": _case(246, "ninf", scale=0.5, R=2, mass=0.2, top_k=0, top_p=1.0),
    "t_ninf_0p9": _case(255, "ninf", scale=0.5, R=2, mass=0.9, top_k=0, top_p=1.0),
    "t_ninf_0p999": _case(256, "ninf", scale=0.5, R=2, mass=0.999, top_k=0, top_p=1.0),
    "t_smooth_0p9_warpers": _case(267, scale=1.0, R=2, mass=0.9),
    "t_ninf_0p9_warpers": _case(271, "ninf", scale=1.0, R=2, mass=0.9),
    "u_V2": _case(130, V=2, R=4),
    "u_V65": _case(131, V=65, R=2),
    "u_V1000": _case(132, V=1000, R=2),
    "u_V1024": _case(133, V=1024, R=2),
    "u_V1025": _case(134, V=1025, R=2),
    "u_V9216": _case(135, V=9216, R=2),
    "u_V9217": _case(136, V=9217, R=2),
    # the deliberate tie-straddle: an all-equal row, the top-p cut falls inside the one tie group
    "x_all_equal": _case(140, "equal", R=2),
    "x_all_equal_V40": _case(141, "equal", V=40, R=2),          # the same through the single-wave top-p path (<= 64 candidates)
}
STRADDLE_CASES = ("a_ties_topk_topp", "x_all_equal", "x_all_equal_V40")          # the only cases whose top-p cut may fall inside a tie group


def case_inputs(name):
    """-> (logits float32 [R, V], history int64 [R, H]) of a case: RandomState(seed), `randn * scale`, 8 random history ids, then the
    case's transform."""
    c = CASES[name]
    V, R = c["V"], c["R"]
    rs = np.random.RandomState(c["seed"])
    x = (rs.randn(R, V) * c["scale"]).astype(F32)
    hist = rs.randint(0, V, size=(R, 8)).astype(np.int64)
    t = c["transform"]
    if t == "grid":                                    # quantise to a 0.25 grid: ties everywhere, the top-k threshold included
        x = (np.round(x * 4.0) / 4.0).astype(F32)
    elif t == "dominant":                              # one planted token far above the rest: probability > 0.9 on its own
        ids = rs.randint(0, V, size=R)
        x[np.arange(R), ids] = x.max(1) + F32(12.0)
    elif t == "ninf":                                  # -inf at V-1, at the first seen id and at 100 random ids
        for r in range(R):
            x[r, rs.choice(V - 1, size=100, replace=False)] = -np.inf
            x[r, V - 1] = -np.inf
            x[r, hist[r, 0]] = -np.inf
    elif t == "lone":                                  # one token (not a seen one) 40 above the rest: its float32 probability is exactly 1
        for r in range(R):
            i = int(rs.randint(0, V))
            while i in hist[r]:
                i = (i + 1) % V
            x[r, i] = x[r].max() + F32(40.0)
    elif t == "penalty":
        x[R - 1] -= x[R - 1].max() + F32(1.0)
        for r in range(R):
            neg = np.nonzero(x[r] < 0)[0] if r < R - 1 else np.sort(np.argsort(x[r], kind="stable")[-20:-1])
            hist[r] = np.concatenate([[0, V - 1, 7, 7, int(np.argmax(x[r]))], neg[rs.choice(neg.size, 3, replace=False)]])
    elif t == "equal":                                 # row 0 all +0.5, row 1 all -0.5 (the penalty's two branches)
        x[:] = F32(0.5)
        x[1::2] = F32(-0.5)
    else:
        assert t == "plain", t
    return x, hist


def input_hash(logits, history):
    h = hashlib.sha1()
    h.update(np.ascontiguousarray(logits, F32).tobytes())
    h.update(np.ascontiguousarray(history, np.int64).tobytes())
    return h.hexdigest()


def oracle_filtered(name, r, logits=None, history=None):
    from oracle import gpt as G
    if logits is None:
        logits, history = case_inputs(name)
    p = CASES[name]["params"]
    with np.errstate(all="ignore"):
        return G.process_logits(logits[r], history[r], repetition_penalty=p["rp"], temperature=p["temp"], top_k=p["top_k"] or None,
                                top_p=p["top_p"], typical_mass=p["mass"] or None)


# ------------------------------------------------------------------------------------------------ the fixture
def fixture_row(g, name, r):
    """-> (kept mask bool [V], filtered float32 [V] with HF's values at the kept positions, straddle) of row r.  straddle is None, or
    (value, count): the top-p cut fell inside the tie group of that value, the fixture holds NONE of the group's members in the mask
    and only how many of them HF kept (torch.sort defines no order inside a tie group)."""
    V = CASES[name]["V"]
    kept = np.unpackbits(g[name + ".kept"][r])[:V].astype(bool)
    off = np.concatenate([[0], np.cumsum(g[name + ".nkept"])])
    f = np.full(V, -np.inf, F32)
    f[kept] = g[name + ".values"][off[r]:off[r + 1]]
    cnt = int(g[name + ".straddle_count"][r])
    return kept, f, ((F32(g[name + ".straddle_value"][r]), cnt) if cnt >= 0 else None)


def pinned_filtered(g, name, r, logits=None, history=None):
    """The HF-pinned filtered row the GPU test builds its CDF from: HF's own values at HF's kept positions; inside a straddled tie
    group, HF's COUNT of members at the oracle's documented (value, id) order - the members with the largest ids stay."""
    kept, f, straddle = fixture_row(g, name, r)
    if straddle is not None:
        value, cnt = straddle
        o = oracle_filtered(name, r, logits, history)
        members = np.nonzero(o == value)[0]
        assert members.size == cnt, (name, r, members.size, cnt)
        f[members] = value
    return f


# ------------------------------------------------------------------------------------------------ the probes
def oracle_cdf(filtered):
    """float64 CDF in vocabulary order of a filtered row -> (c inclusive, lo exclusive, kept ids)"""
    f = np.asarray(filtered, np.float64)
    fin = np.isfinite(f)
    p = np.zeros(f.size, np.float64)
    p[fin] = np.exp(f[fin] - f[fin].max())
    c = np.cumsum(p) / p.sum()
    lo = np.concatenate([[0.0], c[:-1]])
    return c, lo, np.nonzero(fin)[0]


def inverse_cdf(c, u):
    return np.minimum(np.searchsorted(c, u, side="right"), c.size - 1)


def make_probes(filtered, seed):
    """The uniforms the device sampler is driven with for one filtered row, and the token each must give.
    -> dict(u float32 [n], want int [n], wide = the kept tokens that must each be drawn, excluded_mass, first, last).
    Candidates: every kept token's interval mid-point and its 2 % and 98 % points, N_RANDOM seeded uniforms.  A candidate is left out
    only if it lies within EDGE_MARGIN of an edge of its interval or inside an interval narrower than MIN_WIDTH (judged in float64;
    rounding the uniform to the float32 the device receives moves it by at most 6e-8).  Then u = 0, u = nextafter(1, 0) and u = 1, which must give the first / last kept token."""
    c, lo, kept = oracle_cdf(filtered)
    w = c - lo
    cand = [lo[kept] + frac * w[kept] for frac in (0.5, 0.02, 0.98)]
    cand.append(np.random.RandomState(seed).rand(N_RANDOM))
    u64 = np.concatenate(cand)
    u64 = u64[u64 < 1.0]
    tok = inverse_cdf(c, u64)
    ok = (w[tok] >= MIN_WIDTH) & (np.minimum(u64 - lo[tok], c[tok] - u64) >= EDGE_MARGIN)
    u, tok = u64[ok].astype(F32), tok[ok]
    wide = kept[w[kept] >= MIN_WIDTH]
    first, last = int(kept[0]), int(kept[-1])
    special_u = np.array([0.0, np.nextafter(F32(1.0), F32(0.0)), 1.0], F32)
    return dict(u=np.concatenate([u, special_u]), want=np.concatenate([tok, [first, last, last]]), n_swept=int(u.size), wide=wide,
                excluded_mass=float(w[kept][w[kept] < MIN_WIDTH].sum()), first=first, last=last, width=w)


def cut_margin(name, r, logits=None, history=None):
    if logits is None:
        logits, history = case_inputs(name)
    return row_cut_margin(logits[r], history[r], CASES[name]["params"])


def typical_key_gap(name, r, logits=None, history=None):
    if logits is None:
        logits, history = case_inputs(name)
    return row_typical_key_gap(logits[r], history[r], CASES[name]["params"])


def row_cut_margin(x, h, p):
    """Smallest distance, in float64, of a cumulative probability to the cut of a sorted-cumulative warper of the case: top-p's
    ascending cumulative sum (of the row as it enters top-p) against 1 - top_p, the typical warper's against its mass.  The last
    element of either sum is 1 by construction and is kept whatever the cut (min_tokens_to_keep / the clamp of last_ind): left out."""
    from oracle import gpt as G
    out = np.inf
    with np.errstate(all="ignore"):
        if p["top_p"] < 1.0:
            s = G.process_logits(x, h, repetition_penalty=p["rp"], temperature=p["temp"], top_k=p["top_k"] or None,
                                 top_p=1.0, typical_mass=p["mass"] or None).astype(np.float64)
            s = np.sort(s[np.isfinite(s)])
            cum = np.cumsum(np.exp(s - s.max()))
            cum /= cum[-1]
            out = min(out, float(np.abs(cum[:-1] - (1.0 - p["top_p"])).min()) if cum.size > 1 else np.inf)
        if p["mass"]:
            s = G.process_logits(x, h, repetition_penalty=p["rp"], temperature=1.0, top_k=None, top_p=1.0).astype(np.float64)
            lp = s - (s.max() + np.log(np.exp(s - s.max()).sum()))
            pr = np.exp(lp)
            ent = -np.sum(np.where(pr > 0, pr * lp, 0.0))
            key = np.abs(-lp - ent)
            cum = np.cumsum(pr[np.lexsort((np.arange(s.size), key))])
            out = min(out, float(np.abs(cum[:-1] - p["mass"]).min()))
    return out


def row_typical_key_gap(x, h, p):
    """Smallest gap, in float64, between neighbouring sorted typical keys from two places in front of the cut to two places behind it
    (inf for a case without the typical warper): above KEY_MARGIN, float32 rounding of the keys cannot change the kept set."""
    from oracle import gpt as G
    if not p["mass"]:
        return np.inf
    with np.errstate(all="ignore"):
        s = G.process_logits(x, h, repetition_penalty=p["rp"], temperature=1.0, top_k=None, top_p=1.0).astype(np.float64)
        lp = s - (s.max() + np.log(np.exp(s - s.max()).sum()))
        pr = np.exp(lp)
        key = np.abs(-lp - (-np.sum(np.where(pr > 0, pr * lp, 0.0))))
    order = np.lexsort((np.arange(s.size), key))
    last = int((np.cumsum(pr[order]) < p["mass"]).sum())
    near = key[order][max(0, last - 2):last + 4]
    return float(np.diff(near[np.isfinite(near)]).min())


# ------------------------------------------------------------------------------------------------ the CPU tests
@pytest.fixture(scope="module")
def edges(golden):
    return golden("token_sampler_edges")


def test_case_inputs_regenerate_bit_identically(edges):
    """Every case's logits and history come out of the seed and the transform exactly as the fixture's generator saw them."""
    assert sorted(str(n) for n in edges["cases"]) == sorted(CASES)
    for name, c in CASES.items():
        logits, hist = case_inputs(name)
        assert logits.shape == (c["R"], c["V"]) and logits.dtype == F32 and 2 <= c["R"] <= 4
        assert input_hash(logits, hist) == str(edges[name + ".sha1"]), name
        p = c["params"]
        assert np.array_equal(edges[name + ".params"], np.array([p["rp"], p["temp"], p["top_k"], p["top_p"], p["mass"]], np.float64)), name
        assert int(edges[name + ".seed"]) == c["seed"] and int(edges[name + ".V"]) == c["V"]


def test_cases_reach_the_edges_they_are_named_for(edges):
    """The transforms do what the case table says: ties at the top-k threshold, 64 / 65 candidates, a dominant token, a penalised
    arg-max, -inf where stated, the cut inside a tie group exactly where it is planned."""
    from oracle import gpt as G
    for name in ("a_ties_topk_topp", "b_ties_topk_only"):
        logits, hist = case_inputs(name)
        for r in range(CASES[name]["R"]):
            s = G.process_logits(logits[r], hist[r], top_k=None, top_p=1.0)
            kth = np.sort(s)[-50]
            assert int((s == kth).sum()) >= 20 and int((s >= kth).sum()) > 64, (name, r)
    for name, m in (("c_topp_64", 64), ("d_topp_65", 65)):
        logits, hist = case_inputs(name)
        for r in range(CASES[name]["R"]):
            p = CASES[name]["params"]
            s = G.process_logits(logits[r], hist[r], top_k=p["top_k"], top_p=1.0)
            fin = s[np.isfinite(s)]
            assert fin.size == m and np.unique(fin).size == m, (name, r, fin.size)
            kept = fixture_row(edges, name, r)[0]
            assert 1 < kept.sum() < m, (name, r, kept.sum())           # the cut removes something, not everything
    logits, hist = case_inputs("k_dominant")
    for r in range(3):
        c, lo, kept = oracle_cdf(G.process_logits(logits[r], hist[r], top_p=1.0))
        assert (c - lo).max() > 0.9 and fixture_row(edges, "k_dominant", r)[0].sum() == 1
    # the guard alone: 1 - top_p is 1.0 in float32 however it is formed, the float32 ascending cumulative sum ends at <= the cut (the
    # rest of the row sums to less than a quarter ulp of 1: ANY order of summation gives exactly 1.0), and HF keeps the lone token
    for name, wave in (("j_topp_1em8_wave", True), ("j_topp_1em8_block", False)):
        logits, hist = case_inputs(name)
        p = CASES[name]["params"]
        cut = F32(1.0) - F32(p["top_p"])
        assert cut == F32(1.0) and F32(1.0 - p["top_p"]) == F32(1.0)
        for r in range(CASES[name]["R"]):
            s = G.process_logits(logits[r], hist[r], repetition_penalty=p["rp"], temperature=p["temp"], top_k=p["top_k"] or None, top_p=1.0)
            s = np.sort(s[np.isfinite(s)])
            assert (s.size <= 64) if wave else (s.size > 64), (name, r, s.size)
            e = np.exp(s - s[-1], dtype=F32)
            cum = np.cumsum(e / e.sum(dtype=F32), dtype=F32)
            assert cum[-1] <= cut, (name, r, cum[-1])
            assert np.exp(s[:-1].astype(np.float64) - float(s[-1])).sum() < 2.0 ** -26, (name, r)
            kept = fixture_row(edges, name, r)[0]
            assert kept.sum() == 1 and kept[int(np.argmax(logits[r]))] and int(np.argmax(logits[r])) not in hist[r], (name, r)
    for name in ("m_penalty_2", "n_penalty_1p3", "o_penalty_1"):
        logits, hist = case_inputs(name)
        for r in range(3):
            h = hist[r].tolist()
            assert 0 in h and V0 - 1 in h and len(set(h)) < len(h) and int(np.argmax(logits[r])) in h and (logits[r][hist[r]] < 0).sum() >= 3
        # the last row: seen tokens with NEGATIVE logits are among the tokens HF keeps - the sign rule sets values the CDF is made of -
        # and dividing them by the penalty instead would have given another kept set
        r = 2
        kept = fixture_row(edges, name, r)[0]
        ids = np.unique(hist[r])
        assert (logits[r] < 0).all() and kept[ids].any(), name
        p = CASES[name]["params"]
        if p["rp"] != 1.0:
            wrong = logits[r].copy()
            wrong[ids] = wrong[ids] / F32(p["rp"])
            w = G.process_logits(wrong, [], repetition_penalty=1.0, temperature=p["temp"], top_k=p["top_k"], top_p=p["top_p"])
            assert not np.array_equal(np.isfinite(w), kept), name
    for name in ("s_ninf", "s_kinf", "t_ninf_0p9"):
        logits, hist = case_inputs(name)
        for r in range(CASES[name]["R"]):
            assert np.isneginf(logits[r, -1]) and np.isneginf(logits[r, hist[r, 0]]) and 101 <= np.isneginf(logits[r]).sum() <= 102
    for r in range(2):
        assert fixture_row(edges, "s_kinf", r)[0].sum() > 64                     # top-k's threshold is -inf: nothing went there
    for name in ("f_topk_Vm1", "g_topk_V", "h_topk_Vp5"):
        for r in range(2):
            assert fixture_row(edges, name, r)[0].sum() == (V0 - 1 if name == "f_topk_Vm1" else V0), name
    for name, c in CASES.items():
        for r in range(c["R"]):
            straddles = fixture_row(edges, name, r)[2] is not None
            assert straddles or not name.startswith("x_all_equal"), (name, r)
            assert not straddles or name in STRADDLE_CASES, (name, r)


# Observed on every case of this suite: the oracle's filtered values equal HF's BIT FOR BIT (largest difference 0.0, both are single
# float32 divisions / multiplications of the same operands), so 4 x the observed difference is 0: the comparison is exact.
VALUE_TOL = 0.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_process_logits_matches_hf_on_the_edges(edges, name):
    """oracle.gpt.process_logits keeps exactly the tokens the reference's HF processors keep and gives them HF's values.  Inside a tie
    group the top-p cut straddles, HF's choice of members is torch.sort's unspecified order: there the COUNT must agree, and the
    oracle keeps the members with the largest ids (ascending sort by (value, id), the front is removed)."""
    logits, hist = case_inputs(name)
    for r in range(CASES[name]["R"]):
        kept, f, straddle = fixture_row(edges, name, r)
        o = oracle_filtered(name, r, logits, hist)
        okept = np.isfinite(o)
        group = np.zeros(o.size, bool)
        if straddle is not None:
            value, cnt = straddle
            p = CASES[name]["params"]
            from oracle import gpt as G
            with np.errstate(all="ignore"):
                pre = G.process_logits(logits[r], hist[r], repetition_penalty=p["rp"], temperature=p["temp"], top_k=p["top_k"] or None,
                                       top_p=1.0, typical_mass=p["mass"] or None)
            group = pre == value
            members = np.nonzero(group)[0]
            assert 0 < cnt < members.size, (name, r, cnt, members.size)
            assert int(okept[group].sum()) == cnt, (name, r, int(okept[group].sum()), cnt)
            assert np.array_equal(np.nonzero(okept & group)[0], members[-cnt:]), (name, r)
            assert not kept[group].any()
        assert np.array_equal(okept & ~group, kept), (name, r, np.nonzero((okept & ~group) != kept)[0][:8])
        d = float(np.abs(o[kept].astype(np.float64) - f[kept].astype(np.float64)).max()) if kept.any() else 0.0
        assert d <= VALUE_TOL, (name, r, d)


@pytest.mark.parametrize("name", sorted(CASES))
def test_probe_generator_caps(edges, name):
    """The conditions under which the GPU test may leave something out, asserted on the reference CDF alone: no cumulative
    probability within CUT_MARGIN of a cut (so no case is dropped from the top-p comparison), no typical key within KEY_MARGIN of
    its neighbour at the cut, the kept tokens too narrow for a probe
    carry at most 1 % of the mass, every row keeps at least 16 probes, the first and the last kept token are wide enough for
    u = 0 / u -> 1 to be decided by them, and no kept token's exponential underflows in float32."""
    logits, hist = case_inputs(name)
    for r in range(CASES[name]["R"]):
        assert cut_margin(name, r, logits, hist) > CUT_MARGIN, (name, r, cut_margin(name, r, logits, hist))
        assert typical_key_gap(name, r, logits, hist) > KEY_MARGIN, (name, r, typical_key_gap(name, r, logits, hist))
        f = pinned_filtered(edges, name, r, logits, hist)
        pr = make_probes(f, 1000 + r)
        assert pr["excluded_mass"] <= MAX_EXCLUDED_MASS, (name, r, pr["excluded_mass"])
        assert pr["n_swept"] >= MIN_PROBES, (name, r, pr["n_swept"])
        assert set(pr["wide"].tolist()) <= set(pr["want"].tolist())                   # every wide token has a probe of its own
        assert pr["width"][pr["first"]] >= MIN_WIDTH and pr["width"][pr["last"]] >= MIN_WIDTH, (name, r)
        fin = f[np.isfinite(f)]
        assert float(fin.min()) - float(fin.max()) > -80.0, (name, r)
        u64 = pr["u"][:pr["n_swept"]].astype(np.float64)
        c, lo, _ = oracle_cdf(f)
        tok = pr["want"][:pr["n_swept"]]
        assert np.all(np.minimum(u64 - lo[tok], c[tok] - u64) >= EDGE_MARGIN - 6e-8) and np.all((c - lo)[tok] >= MIN_WIDTH)


def test_probe_generator_leaves_out_only_what_the_margins_allow():
    """On a hand-made row: a token narrower than MIN_WIDTH gets no probe, a token of width 4e-5 keeps its mid-point only (its 2 % and
    98 % points are within EDGE_MARGIN of an edge), a wide token keeps all three."""
    p = np.array([0.5, 1e-5, 4e-5, 0.3, 0.0, 0.2 - 5e-5])
    with np.errstate(divide="ignore"):
        f = np.log(p).astype(F32)
    pr = make_probes(f, 0)
    want = pr["want"][:pr["n_swept"]]
    assert pr["wide"].tolist() == [0, 2, 3, 5] and 1 not in want and 4 not in want
    assert (want == 2).sum() == 1 and all((want == v).sum() >= 3 for v in (0, 3, 5))
    assert abs(pr["excluded_mass"] - 1e-5) < 1e-7
    assert pr["want"][-3:].tolist() == [0, 5, 5]
