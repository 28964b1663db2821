"""HF's remaining decode-time logits processors, on the CPU: the numpy restatement of tests/processor_cases.py against HF's own classes
(tests/golden/token_processor_edges.npz), the conditions on the inputs the GPU tests rely on (the probe generator's exclusion caps, the
warper margins, the recorded option sets of tests/golden/gpt_generate_processors.npz biting), the host-side validation and the folded
"first stop step".  The margins are those of tests/test_host_token_sampler.py; none is defined here."""
import json

import numpy as np
import pytest

import processor_cases as P
from test_host_token_sampler import CUT_MARGIN, EDGE_MARGIN, MAX_EXCLUDED_MASS, MIN_PROBES, MIN_WIDTH, make_probes, oracle_cdf

F32 = np.float32
VALUE_TOL = 0.0          # two float32 operations on the same operands, as in test_host_token_sampler.py: the comparison is exact


@pytest.fixture(scope="module")
def edges(golden):
    return golden("token_processor_edges")


@pytest.fixture(scope="module")
def gen(golden):
    return golden("gpt_generate_processors")


def fixture_row(g, name, r):
    """-> (kept mask bool [V], float32 [V] with HF's values at the kept positions, -inf elsewhere)"""
    V = P.CASES[name]["V"]
    kept = np.unpackbits(g[name + ".kept"][r])[:V].astype(bool)
    off = np.concatenate([[0], np.cumsum(g[name + ".nkept"])])
    f = np.full(V, -np.inf, F32)
    f[kept] = g[name + ".values"][off[r]:off[r + 1]]
    return kept, f


def test_case_inputs_regenerate_bit_identically(edges):
    assert sorted(str(n) for n in edges["cases"]) == sorted(P.CASES)
    for name, c in P.CASES.items():
        logits, rows = P.case_inputs(name)
        assert logits.shape == (c["R"], c["V"]) and logits.dtype == F32 and 2 <= c["R"] <= 3
        assert P.input_hash(logits, rows) == str(edges[name + ".sha1"]), name
        p = c["params"]
        assert np.array_equal(edges[name + ".params"], np.array([p["rp"], p["temp"], p["top_k"], p["top_p"], p["mass"]], np.float64)), name
        assert int(edges[name + ".seed"]) == c["seed"] and int(edges[name + ".V"]) == c["V"]
        assert set(c["opts"]) <= set(P.OPT_KEYS)


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_restatement_matches_hf(edges, name):
    """process_row keeps exactly the tokens HF's processor classes keep and gives them HF's values."""
    logits, rows = P.case_inputs(name)
    for r in range(P.CASES[name]["R"]):
        kept, f = fixture_row(edges, name, r)
        o = P.restated(name, r, logits, rows)
        assert np.array_equal(np.isfinite(o), kept), (name, r, np.nonzero(np.isfinite(o) != kept)[0][:8])
        d = float(np.abs(o[kept].astype(np.float64) - f[kept].astype(np.float64)).max())
        assert d <= VALUE_TOL, (name, r, d)


def _without(name, r, logits, rows):
    c = P.CASES[name]
    return P.process_row(logits[r], rows[r], c["params"], {}, c["V"])


def test_cases_reach_the_edges_they_are_named_for(edges):
    V = P.V0
    for n in (1, 2, 3, 5):                                        # the banned id is the row's arg-max and HF removed it
        name = f"ng_n{n}_argmax"
        logits, rows = P.case_inputs(name)
        for r in range(3):
            top = int(np.argmax(logits[r]))
            assert top in P.banned_ngram_ids([1] * rows[r]["fills"] + rows[r]["hist"].tolist(), n) and not fixture_row(edges, name, r)[0][top]
            assert np.isfinite(_without(name, r, logits, rows)[top])
    logits, rows = P.case_inputs("ng_n3_penalised_seen")
    for r in range(3):
        top = int(np.argmax(logits[r]))
        assert top in rows[r]["hist"] and np.isfinite(_without("ng_n3_penalised_seen", r, logits, rows)[top])
        assert not fixture_row(edges, "ng_n3_penalised_seen", r)[0][top]
    logits, rows = P.case_inputs("ng_n5_short_history")             # 3, 4 and 5 ids, no fill ids: nothing banned, the option changes nothing
    assert [len(r["hist"]) for r in rows] == [3, 4, 5] and all(r["fills"] == 0 for r in rows)
    for r in range(3):
        assert np.array_equal(_without("ng_n5_short_history", r, logits, rows), P.restated("ng_n5_short_history", r, logits, rows))
    logits, rows = P.case_inputs("ng_n3_overlap")
    for r in range(3):
        h = rows[r]["hist"].tolist()
        assert len(set(h[-5:])) == 1 and sum(h[i:i + 2] == h[-2:] for i in range(len(h) - 2)) >= 3
        assert not fixture_row(edges, "ng_n3_overlap", r)[0][h[-1]]
    logits, rows = P.case_inputs("ng_n3_fill_window0")
    for r, one_banned in ((0, True), (1, True), (2, False)):      # (1, 1, 1) exists with >= 3 fill ids only; (1, 1, V-2) always
        kept = fixture_row(edges, "ng_n3_fill_window0", r)[0]
        assert kept[1] == (not one_banned) and not kept[V - 2], (r, kept[1], kept[V - 2])
    logits, rows = P.case_inputs("ng_n5_few_fills")
    assert [r["fills"] for r in rows] == [2, 1]
    assert not fixture_row(edges, "ng_n5_few_fills", 0)[0][1] and fixture_row(edges, "ng_n5_few_fills", 1)[0][1]
    for name in ("ng_n3_history_1600", "ng_n2_history_1600_penalised"):
        logits, rows = P.case_inputs(name)
        for r in range(2):
            n = P.CASES[name]["opts"]["no_repeat_ngram_size"]
            banned = P.banned_ngram_ids([1] * rows[r]["fills"] + rows[r]["hist"].tolist(), n)
            assert len(rows[r]["hist"]) == 1600 and len(banned) >= 2      # (a given pair of 12 x 12 recurs ~11 times in 1 600 ids)
            assert not np.array_equal(_without(name, r, logits, rows), P.restated(name, r, logits, rows))
    for name in ("stop_min_new_tokens", "stop_min_length", "stop_both"):      # banned the step before the first stop step, not at or behind it
        logits, rows = P.case_inputs(name)
        assert [fixture_row(edges, name, r)[0][V - 1] for r in range(3)] == [False, True, True], name
        assert all(np.isfinite(_without(name, r, logits, rows)[V - 1]) for r in range(3))
    for name, sign in (("decay_positive_stop", 1), ("decay_negative_stop", -1)):
        logits, rows = P.case_inputs(name)
        assert all(np.sign(logits[r, V - 1]) == sign for r in range(3))
        f = [P.restated(name, r, logits, rows)[V - 1] for r in range(3)]
        want = (sign * 1.5 + 1.5 * (1.3 ** 8 - 1)) / 0.8          # 13.3 from +1.5, 11.5 from -1.5: the row's largest score either way
        assert fixture_row(edges, name, 2)[0][V - 1] and abs(f[2] - want) < 1e-3 and f[2] == np.nanmax(P.restated(name, 2, logits, rows))
    logits, rows = P.case_inputs("suppress_begin")
    o0, o1 = P.case_options("suppress_begin", 0, logits), P.case_options("suppress_begin", 1, logits)
    assert not fixture_row(edges, "suppress_begin", 0)[0][o0["begin_suppress_tokens"]].any()
    assert fixture_row(edges, "suppress_begin", 1)[0][o1["begin_suppress_tokens"]].any()
    for name in ("minp_lone", "eps_lone", "minp_lone_V65", "eps_lone_V65"):
        assert all(fixture_row(edges, name, r)[0].sum() == 1 for r in range(3)), name
    for name in ("minp_after_topp", "eps_after_topp"):            # top-p removed something first, the warper something more
        logits, rows = P.case_inputs(name)
        c = P.CASES[name]
        for r in range(3):
            pre_topp = P.process_row(logits[r], rows[r], dict(c["params"], top_p=1.0), {}, c["V"])
            pre = _without(name, r, logits, rows)
            assert np.isfinite(pre_topp).sum() > np.isfinite(pre).sum() > fixture_row(edges, name, r)[0].sum() >= 1, (name, r)
    for name in ("minp_tie_at_threshold", "eps_tie_at_threshold"):      # tie groups next to the threshold on both sides: all in or all out
        logits, rows = P.case_inputs(name)
        for r in range(3):
            pre, kept = _without(name, r, logits, rows), fixture_row(edges, name, r)[0]
            low_kept, high_cut = pre[kept].min(), pre[np.isfinite(pre) & ~kept].max()
            assert (pre == low_kept).sum() >= 2 and (pre == high_cut).sum() >= 2 and kept[pre == low_kept].all()
    for name in P.CASES:                                          # <= 64 candidates into top-p at V = 65: the single-wave path
        assert (P.CASES[name]["V"] == P.V1) == name.endswith("_V65")


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_probe_generator_caps(edges, name):
    """What the GPU test may leave out, asserted on HF's values alone: no p / p_max within CUT_MARGIN of min_p and no p within
    CUT_MARGIN of epsilon, at most MAX_EXCLUDED_MASS of a row's mass without a probe, at least MIN_PROBES probes per row, the first
    and the last kept token wide enough for u = 0 / u -> 1."""
    logits, rows = P.case_inputs(name)
    for r in range(P.CASES[name]["R"]):
        assert P.warper_margin(name, r, logits, rows) > CUT_MARGIN, (name, r, P.warper_margin(name, r, logits, rows))
        f = fixture_row(edges, name, r)[1]
        pr = make_probes(f, 1000 + r)
        assert pr["excluded_mass"] <= MAX_EXCLUDED_MASS, (name, r, pr["excluded_mass"])
        assert pr["n_swept"] >= MIN_PROBES, (name, r, pr["n_swept"])
        assert set(pr["wide"].tolist()) <= set(pr["want"].tolist())
        assert pr["width"][pr["first"]] >= MIN_WIDTH and pr["width"][pr["last"]] >= MIN_WIDTH, (name, r)
        fin = f[np.isfinite(f)]
        assert float(fin.min()) - float(fin.max()) > -80.0, (name, r)
        c, lo, _ = oracle_cdf(f)
        tok = pr["want"][:pr["n_swept"]]
        u64 = pr["u"][:pr["n_swept"]].astype(np.float64)
        assert np.all(np.minimum(u64 - lo[tok], c[tok] - u64) >= EDGE_MARGIN - 6e-8)


def test_decay_table_of_the_library_is_hf_s_float32():
    """The table the LIBRARY uploads (dtts_gpt_decay_multipliers, host only: the function dtts_gpt_prefill fills the session's table
    with) holds, for every step a session can take (1603 mel positions), the number torch multiplies the float32 |score| by:
    pow(factor, i) - 1 in Python's double, rounded once - and the restatement's helper gives the same.  Behind 1e30, where HF's
    multiplier is about to leave float32 (or pow raises OverflowError), the table saturates instead of refusing the call: HF's own
    documented example (15, 1.6) is served at the default max_generate_length of 600."""
    torch = pytest.importorskip("torch")
    from detail_tts_amd.gpt.decode_options import decay_multipliers, validate_decode_options
    one = torch.ones(1, dtype=torch.float32)
    for factor in (1.3, 1.07, 1.2, 1.01, 1.005, 1.6, 2.0, 3.0, 4.0):
        t = decay_multipliers(factor, 1604)
        assert t.dtype == np.float32 and t.shape == (1604,) and t[0] == 0.0 and np.isfinite(t).all() and (np.diff(t) >= 0).all()
        for i in range(1, 1604):
            try:
                m = pow(factor, i) - 1
            except OverflowError:
                m = float("inf")
            if m < 1e30:
                assert float((one * m)[0]) == float(t[i]) == float(P.decay_multiplier(factor, i)), (factor, i)
            else:
                assert t[i] == np.float32(1e30), (factor, i, t[i])
    assert validate_decode_options(dict(exponential_decay_length_penalty=(15, 1.6))) == dict(exponential_decay_length_penalty=(15, 1.6))
    assert decay_multipliers(1.6, 601)[600] == np.float32(1e30) and decay_multipliers(1.6, 601)[100] == np.float32(1.6 ** 100 - 1)


def test_the_recorded_options_bite(gen):
    """Every option set of the generate fixture changes the reference's own codes: the GPU test's comparison could not pass on a
    decode that drops the keyword."""
    sets = [str(s) for s in gen["sets"]]
    assert {"no_repeat_ngram_size", "min_length", "min_new_tokens", "exponential_decay_length_penalty", "suppress_tokens",
            "begin_suppress_tokens", "min_p", "epsilon_cutoff", "valle_no_repeat_ngram_size", "all", "input_tokens_min_new_tokens",
            "valle_min_length"} == set(sets)
    G = int(gen["max_generate_length"])
    assert 12 <= G <= 24
    for s in sets:
        codes, base = gen[s + ".codes"], gen[s + ".base"]
        assert codes.shape == base.shape == (1 if s.startswith("input_tokens") else 2, G), s
        assert (codes != base).any(), s
        opt = json.loads(str(gen[s + ".option"]))
        assert opt and set(opt) <= set(P.OPT_KEYS), (s, opt)
    assert set(json.loads(str(gen["all.option"]))) == set(P.OPT_KEYS)
    # what the options promise, on the reference's codes
    n_new = lambda row: int(np.argmax(row == 8193)) + 1 if (row == 8193).any() else G      # noqa: E731
    k = json.loads(str(gen["min_new_tokens.option"]))["min_new_tokens"]
    assert min(n_new(r) for r in gen["min_new_tokens.codes"]) > k > min(n_new(r) for r in gen["min_new_tokens.base"])
    ml = json.loads(str(gen["min_length.option"]))["min_length"] - int(gen["input_len"])
    assert min(n_new(r) for r in gen["min_length.codes"]) > ml > min(n_new(r) for r in gen["min_length.base"])
    # what HF counts as prompt: min_new_tokens counts from behind input_tokens, min_length counts an acoustic prompt's codes
    s, k = "input_tokens_min_new_tokens", gen["input_tokens"].shape[1]
    opt = json.loads(str(gen[s + ".option"]))
    assert (gen[s + ".codes"][:, :k] == gen["input_tokens"]).all() and (gen[s + ".base"][:, :k] == gen["input_tokens"]).all()
    assert n_new(gen[s + ".codes"][0]) - 1 - k >= opt["min_new_tokens"] > n_new(gen[s + ".base"][0]) - 1 - k
    assert gen[s + ".codes"][0, k] not in opt["begin_suppress_tokens"]
    ml = json.loads(str(gen["valle_min_length.option"]))["min_length"] - int(gen["valle_input_len"])
    assert int(gen["valle_input_len"]) == int(gen["input_len"]) + 1 + gen["prompt"].shape[1] and ml > 0
    assert n_new(gen["valle_min_length.codes"][0]) > ml > n_new(gen["valle_min_length.base"][0])
    for s in ("no_repeat_ngram_size", "valle_no_repeat_ngram_size"):
        for row in gen[s + ".codes"]:
            pairs = list(zip(row[:-1], row[1:]))
            assert len(set(pairs)) == len(pairs), s                  # no pair of codes twice under n = 2
        assert any(len(set(zip(b[:-1], b[1:]))) < G - 1 for b in gen[s + ".base"]), s
    sup = json.loads(str(gen["suppress_tokens.option"]))["suppress_tokens"]
    assert not np.isin(gen["suppress_tokens.codes"], sup).any() and np.isin(gen["suppress_tokens.base"], sup).any()
    bs = json.loads(str(gen["begin_suppress_tokens.option"]))["begin_suppress_tokens"]
    assert not np.isin(gen["begin_suppress_tokens.codes"][:, 0], bs).any() and np.isin(gen["begin_suppress_tokens.base"][:, 0], bs).all()


BAD = [dict(no_repeat_ngram_size=17), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.5), dict(min_p=-0.1), dict(min_p=1.5),
       dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-0.5), dict(epsilon_cutoff=7), dict(epsilon_cutoff=float("nan")), dict(suppress_tokens=[8194]),
       dict(suppress_tokens=[-1]), dict(begin_suppress_tokens=[3, 9000]), dict(exponential_decay_length_penalty=(3, 1.0)),
       dict(exponential_decay_length_penalty=(3, 0.5)), dict(exponential_decay_length_penalty=(-1, 1.5)),
       dict(exponential_decay_length_penalty=1.5), dict(min_length=-1), dict(min_new_tokens=-3), dict(min_length=2.0),
       dict(bad_words_ids=[[1]]), dict(min_p=float("nan"))]


class _NoLibrary:
    """a Runtime whose library must not be reached"""
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the options were checked")


@pytest.mark.parametrize("bad", BAD, ids=lambda d: next(iter(d)) + "=" + str(next(iter(d.values()))))
def test_bad_values_raise_before_any_library_call(bad):
    from detail_tts_amd import _lib
    from detail_tts_amd.gpt.decode_options import validate_decode_options
    from detail_tts_amd.runtime import Runtime
    with pytest.raises(ValueError):
        validate_decode_options(bad)
    with pytest.raises(ValueError):                               # the runtime's own entry: refused while filling the struct
        Runtime._processors(_lib.DttsGptOptions(), bad)
    if "bad_words_ids" not in bad:                                # the mirror still drops keywords it does not know
        from detail_tts_amd.gpt.model import UnifiedVoice
        uv = UnifiedVoice.__new__(UnifiedVoice)
        uv.rt, uv.max_mel_tokens = _NoLibrary(), 604
        torch = pytest.importorskip("torch")
        with pytest.raises(ValueError):
            uv.inference_speech_tortoise(torch.zeros(1, 128, 8), None, np.array([[5, 6, 0]]), **bad)


def test_validation_normalises_and_switches_off():
    from detail_tts_amd.gpt.decode_options import validate_decode_options as v
    assert v(None) == {} and v({}) == {}
    assert v(dict(no_repeat_ngram_size=0, min_length=0, min_new_tokens=None, min_p=0.0, epsilon_cutoff=0, suppress_tokens=[])) == {}
    got = v(dict(no_repeat_ngram_size=np.int64(16), suppress_tokens=[9, 3, 3], begin_suppress_tokens=8193, min_p=1, epsilon_cutoff=0.5,
                 exponential_decay_length_penalty=[4, 1.5], min_length=30, min_new_tokens=2))
    assert got == dict(no_repeat_ngram_size=16, suppress_tokens=[3, 9], begin_suppress_tokens=[8193], min_p=1.0, epsilon_cutoff=0.5,
                       exponential_decay_length_penalty=(4, 1.5), min_length=30, min_new_tokens=2)
    # under do_sample=False HF builds no warpers: checked, then dropped
    assert v(dict(min_p=0.3, epsilon_cutoff=0.1, min_length=5), do_sample=False) == dict(min_length=5)
    with pytest.raises(ValueError):
        v(dict(min_p=2.0), do_sample=False)
    assert v(dict(top_k=5, do_sample=True, min_length=3), strict=False) == dict(min_length=3)


def test_options_struct_carries_the_processors():
    """Runtime._processors fills the fields dtts_gpt_options gained, the struct's size is the C header's (the library refuses another)."""
    from detail_tts_amd import _lib
    from detail_tts_amd.runtime import Runtime
    o = _lib.DttsGptOptions()
    keep = Runtime._processors(o, dict(no_repeat_ngram_size=4, min_length=40, min_new_tokens=20, exponential_decay_length_penalty=(7, 1.25),
                                       suppress_tokens=[5, 2], begin_suppress_tokens=[8193], min_p=0.25, epsilon_cutoff=0.001))
    assert (o.no_repeat_ngram_size, o.min_length, o.min_new_tokens, o.exp_decay_start, o.exp_decay_factor) == (4, 40, 20, 7, 1.25)
    assert [o.suppress_tokens[i] for i in range(o.n_suppress_tokens)] == [2, 5] and o.n_begin_suppress_tokens == 1
    assert o.begin_suppress_tokens[0] == 8193 and o.min_p == 0.25 and abs(o.epsilon_cutoff - 0.001) < 1e-9 and len(keep) == 2
    assert Runtime._processors(_lib.DttsGptOptions(), None) is None and Runtime._processors(_lib.DttsGptOptions(), {}) is None


def test_first_stop_step_fold():
    """The per-row "first step at which the stop token may be drawn" the control block carries: tortoise, input_tokens, a valle prompt.
    first_stop_step is the library's own fold (dtts_gpt_first_stop_step, which dtts_gpt_prefill calls), checked against HF's two rules
    applied step by step."""
    from detail_tts_amd.gpt.decode_options import first_stop_step

    def brute(input_len, k, min_length, min_new_tokens):
        for j in range(k, 4000):          # HF samples from step k on: input_ids hold input_len + j ids, j - k of them new
            if not (input_len + j < min_length or j - k < min_new_tokens):
                return j
    Lt = 7
    tortoise = 1 + (Lt + 2) + 1                                   # cond + text positions + 8192
    valle = 1 + (Lt + 2) + (9 + 2)                                # ... + [1, 8192, c_1 .. c_9]
    assert first_stop_step(tortoise, 0) == 0
    assert first_stop_step(tortoise, 0, min_new_tokens=20) == 20
    assert first_stop_step(tortoise, 0, min_length=tortoise + 5) == 5
    assert first_stop_step(tortoise, 0, min_length=tortoise - 3) == 0          # the prefix columns alone are long enough
    assert first_stop_step(tortoise, 3, min_new_tokens=20) == 23               # input_tokens are prompt: 20 NEW tokens behind them
    assert first_stop_step(tortoise, 3, min_length=tortoise + 5) == 5          # ... but they count towards min_length
    assert first_stop_step(valle, 0, min_length=valle + 4, min_new_tokens=2) == 4
    assert first_stop_step(valle, 0, min_length=tortoise + 4, min_new_tokens=2) == 2      # the prompt's codes count towards min_length
    for input_len in (tortoise, valle):
        for k in (0, 3):
            for ml in (0, 5, input_len, input_len + 9):
                for mn in (0, 1, 12):
                    assert max(k, first_stop_step(input_len, k, ml, mn)) == brute(input_len, k, ml, mn), (input_len, k, ml, mn)
