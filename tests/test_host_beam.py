"""Beam search, host side: tests/beam_model.py (the numpy restatement of HF's _beam_search that csrc/gpt_beam.hip implements) against
tests/golden/beam_steps.npz (HF's own functions chained over planted logits), the mutations the fixture must catch, and the fixture's
own consistency.  No GPU."""
import os

import numpy as np
import pytest

import beam_cases as BC
import beam_model as BM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_steps.npz")
REAL = -1.0e8


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def case_options(case):
    return dict(K=case["K"], G=case["G"], eos=case["V"] - 1, lp=case["lp"], es=case["es"], rp=case["rp"], ngram=case["ngram"])


def compare_step(name, g, s, st, info, was_done, rtol=1e-6):
    """state `st` after step s (and the candidates `info`) against the fixture; was_done[u]: the utterance was done before this step"""
    def rec(k):
        return g[f"{name}.{k}"][s]
    for u in range(st["run_seq"].shape[0]):
        real = rec("fin_score")[u] > REAL
        assert np.array_equal(st["fin_flag"][u], rec("fin_flag")[u]), (name, s, u, "fin_flag")
        assert np.array_equal(real, st["fin_score"][u] > REAL), (name, s, u)
        np.testing.assert_allclose(st["fin_score"][u][real], rec("fin_score")[u][real], rtol=rtol, err_msg=f"{name} step {s} fin_score")
        assert np.array_equal(st["fin_seq"][u][real], rec("fin_seq")[u][real]), (name, s, u, "fin_seq")
        assert np.array_equal(st["fin_len"][u][real], rec("fin_len")[u][real]), (name, s, u, "fin_len")
        assert bool(st["done"][u]) == bool(rec("done")[u]), (name, s, u, "done")
        if was_done[u]:
            continue
        assert bool(st["unsat"][u]) == bool(rec("unsat")[u]), (name, s, u, "unsat")
        c = info[u]
        live = rec("cand_score")[u] > REAL
        assert np.array_equal(c["cand_score"] > REAL, live), (name, s, u)
        assert np.array_equal(c["cand_tok"][live], rec("cand_tok")[u][live]), (name, s, u, "cand_tok")
        assert np.array_equal(c["cand_beam"][live], rec("cand_beam")[u][live]), (name, s, u, "cand_beam")
        assert np.array_equal(c["stop"][live], rec("stop")[u][live]), (name, s, u, "stop")
        np.testing.assert_allclose(c["cand_score"][live], rec("cand_score")[u][live], rtol=rtol, err_msg=f"{name} step {s} cand_score")
        if st["done"][u]:
            continue                      # (at max_length every continuation carries -1e9: the running beams are a tie)
        assert np.array_equal(st["run_seq"][u], rec("run_seq")[u]), (name, s, u, "run_seq")
        assert np.array_equal(st["parents"][u], rec("parents")[u]), (name, s, u, "parents")
        np.testing.assert_allclose(st["run_score"][u], rec("run_score")[u], rtol=rtol, err_msg=f"{name} step {s} run_score")


def run_case(name, g, mutate=None, teacher=True):
    """teacher: every step starts from the fixture's state (an error shows at the step that makes it)"""
    case = BC.CASES[name]
    logits, prompt = BC.case_logits(case, int(g[name + ".seed"])), BC.prompts(case)
    assert BC.input_hash(logits, prompt) == str(g[name + ".sha1"]), "the regenerated inputs are not the fixture's"
    o = case_options(case)
    st = BM.init_state(case["U"], case["K"], case["G"], o["eos"])
    for s in range(case["steps"]):
        was_done = st["done"].copy()
        st, info = BM.beam_step(st, logits[s], prompt, s, o, mutate)
        compare_step(name, g, s, st, info, was_done)
        if teacher:
            st = fixture_state(name, g, s, st)


def fixture_state(name, g, s, st):
    """the fixture's state after step s in the model's form; utterances that are done keep the model's own (frozen) state"""
    out = {k: v.copy() for k, v in st.items()}
    for k in ("run_seq", "run_score", "fin_seq", "fin_score", "fin_flag", "fin_len", "unsat", "parents"):
        ref = g[f"{name}.{k}"][s]
        for u in range(ref.shape[0]):
            if not st["done"][u]:
                out[k][u] = ref[u]
    return out


@pytest.mark.parametrize("name", sorted(BC.CASES))
def test_model_reproduces_hf(gold, name):
    run_case(name, gold, teacher=False)
    run_case(name, gold, teacher=True)


def test_fixture_covers_what_it_claims(gold):
    assert sorted(BC.CASES) == list(gold["cases"])
    K = {BC.CASES[n]["K"] for n in BC.CASES}
    assert {2, 3, 8} <= K and {BC.CASES[n]["V"] for n in BC.CASES} >= {8194, 40}
    assert {BC.CASES[n]["U"] for n in BC.CASES} == {1, 2, 3}
    assert {BC.CASES[n]["lp"] for n in BC.CASES} >= {0.0, 0.5, 1.0, 2.0, -1.0} and {BC.CASES[n]["es"] for n in BC.CASES} == {0, 1, 2}
    first = second = allk = maxlen = early = False
    for n in sorted(BC.CASES):
        c = BC.CASES[n]
        assert float(gold[n + ".min_gap"]) >= BC.MIN_GAP, n
        stop, tok = gold[n + ".stop"], gold[n + ".cand_tok"]
        eos = tok == c["V"] - 1
        first |= bool(eos[:, :, :c["K"]].any())
        second |= bool(eos[:, :, c["K"]:].any())
        allk |= bool(eos[:, :, :c["K"]].all(-1).any())
        maxlen |= bool(stop.all(-1).any())
        early |= bool(gold[n + ".done"].any() and not stop[-1].all())
    assert first and second and allk and maxlen and early


@pytest.mark.parametrize("mutation", BM.MUTATIONS)
def test_mutations_are_caught(gold, mutation):
    """every deliberate error of the restatement fails at least one case"""
    caught = []
    for name in sorted(BC.CASES):
        try:
            run_case(name, gold, mutate=mutation, teacher=True)
        except AssertionError:
            caught.append(name)
    assert caught, f"no case notices the mutation {mutation!r}"
    assert len(BM.MUTATIONS) >= 8


# ---------------------------------------------------------------------------------------------------------------- options and ABI
def test_beam_option_validation():
    from detail_tts_amd.gpt.decode_options import split_beam_options, validate_beam_options, validate_decode_options
    assert validate_beam_options(None, None, None) == (0, 1.0, 0)
    assert validate_beam_options(1, 2.0, "never") == (0, 2.0, 2)                    # one beam: today's decode, the knobs are only checked
    assert validate_beam_options(4, 0.5, True, do_sample=False, num_return_sequences=4) == (4, 0.5, 1)
    for bad in (dict(num_beams=0), dict(num_beams=2.0), dict(num_beams=True), dict(num_beams=17), dict(num_beams=2, length_penalty="x"),
                dict(num_beams=2, length_penalty=float("nan")), dict(num_beams=2, early_stopping="sometimes"), dict(num_beams=2, early_stopping=1),
                dict(num_beams=2, do_sample=True), dict(num_beams=2, typical_sampling=True), dict(num_beams=2, input_tokens=[[1]]),
                dict(num_beams=2, forced_codes=[[1]]), dict(num_beams=2, forced_uniforms=[0.5]), dict(num_beams=2, num_candidates=2),
                dict(num_beams=2, num_return_sequences=3), dict(num_beams=2, stream=True)):
        with pytest.raises(ValueError) as e:
            validate_beam_options(**bad)
        key = [k for k in bad if k != "num_beams"] or ["num_beams"]
        assert any(k in str(e.value) for k in key + ["num_beams"]), (bad, str(e.value))
    # the same keys inside decode_options (infer / infer_gpt): validated, then split off the processors
    v = validate_decode_options(dict(num_beams=3, length_penalty=2.0, early_stopping="never", no_repeat_ngram_size=2, min_p=0.1))
    proc, beam = split_beam_options(v)
    assert proc == dict(no_repeat_ngram_size=2) and beam == dict(num_beams=3, length_penalty=2.0, early_stopping="never")      # (min_p: sampling only)
    assert split_beam_options(validate_decode_options(dict(num_beams=1, min_p=0.1))) == (dict(min_p=0.1), None)
    assert split_beam_options(validate_decode_options(None)) == ({}, None)
    with pytest.raises(ValueError):
        validate_decode_options(dict(num_beams=40))


def test_beam_fields_of_the_options_struct():
    """num_beams, length_penalty, early_stopping sit with the option fields in front of token_wgs; the library's init leaves beams off
    with HF's length_penalty 1.0; the struct's size is the library's"""
    import ctypes as C
    from detail_tts_amd import _lib
    names = [n for n, _ in _lib.DttsGptOptions._fields_]
    i = names.index("token_wgs")
    assert names[i - 3:i] == ["num_beams", "length_penalty", "early_stopping"] and names[i - 4] == "epsilon_cutoff"
    assert names[-4:] == ["token_wgs", "prompt_codes", "prompt_lens", "prompt_stride"]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "detail_hip.h")).read()
    body = hdr[hdr.index("typedef struct dtts_gpt_options {"):hdr.index("} dtts_gpt_options;")]
    import re
    pos = [re.search(r"\n\s+(?:int|float) %s;" % n, body).start() for n in ("epsilon_cutoff", "num_beams", "length_penalty", "early_stopping", "token_wgs")]
    assert pos == sorted(pos)
    lib = _lib.load()
    o = _lib.DttsGptOptions()
    lib.dtts_gpt_options_init(C.byref(o))
    assert o.struct_size == C.sizeof(_lib.DttsGptOptions)
    assert (o.num_beams, o.early_stopping) == (0, 0) and o.length_penalty == 1.0
    for sym in ("dtts_gpt_beam_generate", "dtts_gpt_beam_finish", "dtts_op_beam_step"):
        assert hasattr(lib, sym)


def test_public_entries_refuse_what_beams_exclude():
    """infer / infer_gpt / infer_stream themselves (not the validator alone): a beam option together with forced_codes, num_candidates > 1
    or return_candidates, and any beam option in infer_stream, is a ValueError naming the keyword, raised before the model, the
    runtime or a stream is touched - `self` is a bare object here, which anything later would trip over.  Runtime refuses a processors
    dict that still carries a beam key (dropped there, the call would decode sampled and tell nobody)."""
    from detail_tts_amd import _lib
    from detail_tts_amd.runtime import Runtime
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    me, beams = object(), dict(num_beams=4, length_penalty=1.0)
    with pytest.raises(ValueError, match="stream"):
        next(SynthesizerTrn.infer_stream(me, iter([]), decode_options=beams))
    with pytest.raises(ValueError, match="stream"):
        next(SynthesizerTrn.infer_stream(me, iter([]), decode_options=dict(num_beams=2, min_p=0.1)))
    with pytest.raises(ValueError, match="num_beams"):
        next(SynthesizerTrn.infer_stream(me, iter([]), decode_options=dict(num_beams=17)))
    a = (None, None, None, None)
    with pytest.raises(ValueError, match="forced_codes"):
        SynthesizerTrn.infer(me, *a, forced_codes=[[1, 2]], decode_options=beams)
    with pytest.raises(ValueError, match="num_candidates"):
        SynthesizerTrn.infer(me, *a, num_candidates=2, decode_options=beams)
    with pytest.raises(ValueError, match="return_candidates"):
        SynthesizerTrn.infer(me, *a, return_candidates=True, decode_options=beams)
    with pytest.raises(ValueError, match="forced_codes"):
        SynthesizerTrn.infer_gpt(me, *a, forced_codes=[[1, 2]], decode_options=beams)
    # one beam is no beam search: the calls get past the check (and then trip over the bare object)
    with pytest.raises(AttributeError):
        next(SynthesizerTrn.infer_stream(me, iter([]), decode_options=dict(num_beams=1)))
    for key, v in (("num_beams", 4), ("length_penalty", 2.0), ("early_stopping", True)):
        with pytest.raises(ValueError, match=key):
            Runtime._processors(_lib.DttsGptOptions(), {key: v, "min_length": 3})
