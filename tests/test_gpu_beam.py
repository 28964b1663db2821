"""Beam search on the DEVICE (csrc/gpt_beam.hip): every case of tests/golden/beam_steps.npz (HF's own beam functions chained over
planted logits) through dtts_op_beam_step, one step at a time from the fixture's state."""
import numpy as np
import pytest

import beam_cases as BC
import beam_model as BM
from test_host_beam import case_options, compare_step, fixture_state

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def rt(weights):
    from detail_tts_amd.runtime import Runtime
    return Runtime(weights, folded=True, parts=("gpt",))


@pytest.fixture(scope="module")
def steps(golden):
    return golden("beam_steps")


def device_step(rt, case, st, logits, prompt, s):
    """one device step in the restatement's form: (state, info per utterance)"""
    o = case_options(case)
    new, inf = rt.op_beam_step(dev(logits), st, prompt, s, num_beams=o["K"], max_new_tokens=o["G"], length_penalty=o["lp"],
                               early_stopping={0: False, 1: True, 2: "never"}[o["es"]], repetition_penalty=o["rp"],
                               processors=dict(no_repeat_ngram_size=o["ngram"]) if o["ngram"] else None)
    new["parents"] = inf["parents"]
    G = o["G"]
    info = []
    for u in range(case["U"]):
        tok = inf["cand_tok"][u]
        info.append(None if st["done"][u] else dict(cand_score=inf["cand_score"][u], cand_beam=inf["cand_beam"][u], cand_tok=tok,
                                                     stop=(tok == o["eos"]) | (s + 1 >= G)))
    return new, info


@pytest.mark.parametrize("name", sorted(BC.CASES))
def test_op_beam_step_reproduces_hf(rt, steps, name):
    """selections, parents, sequences and flags exactly, scores to 1e-6 relative; every step starts from HF's own state, and the chained
    device state is carried along as well (it has to end in the same finished set)"""
    case = BC.CASES[name]
    logits, prompt = BC.case_logits(case, int(steps[name + ".seed"])), BC.prompts(case)
    assert BC.input_hash(logits, prompt) == str(steps[name + ".sha1"])
    o = case_options(case)
    st = BM.init_state(case["U"], case["K"], case["G"], o["eos"])
    chained = {k: v.copy() for k, v in st.items()}
    for s in range(case["steps"]):
        was_done = st["done"].copy()
        st, info = device_step(rt, case, st, logits[s], prompt, s)
        compare_step(name, steps, s, st, info, was_done)
        st = fixture_state(name, steps, s, st)
        cwas = chained["done"].copy()
        chained, cinfo = device_step(rt, case, chained, logits[s], prompt, s)
        compare_step(name, steps, s, chained, cinfo, cwas, rtol=1e-5)


def test_op_beam_step_refusals(rt):
    st = BM.init_state(1, 2, 4, 39)
    x = dev(np.zeros((2, 40), np.float32))
    pr = np.zeros((1, 2), np.int64)
    for kw in (dict(num_beams=17), dict(num_beams=2, early_stopping="sometimes"), dict(num_beams=2, length_penalty=float("inf"))):
        with pytest.raises(ValueError):
            rt.op_beam_step(x, st, pr, 0, max_new_tokens=4, **kw)
    with pytest.raises(RuntimeError):
        rt.op_beam_step(x, st, pr, 4, num_beams=2, max_new_tokens=4)          # step outside 0 .. G - 1


# ---------------------------------------------------------------------------------------------------------------- end to end
# tests/golden/gpt_generate_beams.npz: the reference's generate(num_beams=K, do_sample=False) under the synthetic weights.
import json          # noqa: E402

E2E = sorted(BC.E2E_CASES)
# Measured on one MI355X (profiles/beam_measured_errors.txt): the largest |device - reference| accumulated score is 1.764e-05 (the fixture's
# decision gaps are >= E2E_MIN_GAP = 20 x that), and the teacher-forced sum of a returned hypothesis scatters by at most 1.218e-05 around
# the decode's own accumulated score: both tolerances are 20 x the latter, rounded up.
SCORE_TOL = 2.5e-4
LINEAGE_TOL = 2.5e-4


@pytest.fixture(scope="module")
def gen(golden):
    return golden("gpt_generate_beams")


@pytest.fixture(scope="module")
def uv(rt):
    from detail_tts_amd.config import load_config
    from detail_tts_amd.gpt.model import UnifiedVoice
    return UnifiedVoice(rt, load_config()["gpt"])


def case_inputs(gen, name, us=None):
    c = BC.E2E_CASES[name]
    us = range(c["U"]) if us is None else us
    refer = dev(np.stack([gen[f"{name}.u{u}.refer"] for u in us]))
    texts = [gen[f"{name}.u{u}.text"] for u in us]
    prompt = [gen[f"{name}.u{u}.prompt"] for u in us] if c["prompt_m"] else None
    return refer, texts, prompt


def padded_texts(texts):
    """the mirror takes a rectangle and text_lengths"""
    tl = [len(t) for t in texts]
    out = np.zeros((len(texts), max(tl)), np.int32)
    for i, t in enumerate(texts):
        out[i, : len(t)] = t
    return out, tl


def options_of(name):
    c = BC.E2E_CASES[name]
    common = dict(c["common"])
    kw = dict(num_beams=c["K"], num_return_sequences=c["nrs"], repetition_penalty=common.pop("repetition_penalty"), **c["beam"])
    return kw, (common or None)


def run_device(rt, gen, name, us=None, **extra):
    refer, texts, prompt = case_inputs(gen, name, us)
    kw, proc = options_of(name)
    return rt.gpt_generate_beams(refer, None, texts, max_generate_length=int(gen["max_generate_length"]), prompt_codes=prompt,
                                 processors=proc, **kw, **extra)


def check_against_reference(gen, name, got, us=None):
    c = BC.E2E_CASES[name]
    seqs, lens, scores = got
    for i, u in enumerate(range(c["U"]) if us is None else us):
        k = f"{name}.u{u}."
        assert np.array_equal(lens[i], gen[k + "lens"]), (name, u, lens[i], gen[k + "lens"])
        assert np.array_equal(seqs[i], gen[k + "seqs"]), (name, u, seqs[i].tolist(), gen[k + "seqs"].tolist())
        ref = gen[k + "scores"]
        assert np.all(np.abs(scores[i] - ref) <= SCORE_TOL * np.maximum(1.0, np.abs(ref))), (name, u, scores[i], ref)


def test_fixture_margins(gen):
    """the fixture's own recorded smallest decision gap is at least 20 x the measured device error; it differs from greedy; at least two
    cases finish hypotheses before max_length"""
    early = 0
    G = int(gen["max_generate_length"])
    for name in E2E:
        assert float(gen[name + ".min_gap"]) >= BC.E2E_MIN_GAP, name
        c = BC.E2E_CASES[name]
        assert json.loads(str(gen[name + ".options"]))["K"] == c["K"]
        fin = False
        for u in range(c["U"]):
            assert not np.array_equal(gen[f"{name}.u{u}.seqs"][0], gen[f"{name}.u{u}.base"][0]), (name, u)
            fin |= bool((gen[f"{name}.u{u}.lens"] < G).any())
        early += fin
    assert early >= 2
    assert {(BC.E2E_CASES[n]["U"], BC.E2E_CASES[n]["K"]) for n in E2E} >= {(1, 2), (2, 3), (3, 8), (3, 5)}


@pytest.mark.parametrize("mode", ["wgs128", "wgs64", "chain", "graph"])
@pytest.mark.parametrize("name", E2E)
def test_beams_reproduce_the_reference(rt, gen, name, mode):
    """token for token, sequences_scores to the measured tolerance: on the 128- and 64-workgroup token kernels, on the launch chain,
    and replayed from the captured graphs"""
    opt = {"chain": ("gpt_token_kernel", 0, 1), "graph": ("gpt_graph", 1, 0)}.get(mode)
    if opt:
        rt.set_option(opt[0], opt[1])
    try:
        got = run_device(rt, gen, name, token_wgs=64 if mode == "wgs64" else 0)
    finally:
        if opt:
            rt.set_option(opt[0], opt[2])
    check_against_reference(gen, name, got)


def test_two_groups_equal_the_utterances_alone(rt, gen):
    """3 x 8 = 24 rows: two sessions (2 + 1 utterances); every utterance gives what it gives alone"""
    whole = run_device(rt, gen, "b3k8")
    for u in range(3):
        alone = run_device(rt, gen, "b3k8", us=[u])
        for a, b in zip(whole, alone):
            assert np.array_equal(a[u], b[0]), u


def penalised_sum(lp, seq, seen0, common):
    """sum of a hypothesis's processed log-probabilities, from its raw ones: the repetition penalty multiplies the (negative) scores of
    ids seen before, ExponentialDecayLengthPenalty((start, f)) lifts the stop token's by |s| * float32(f ** i - 1) from step start + 1
    on.  suppress_tokens leaves the survivors' log-probabilities as they are (HF takes the log-softmax first)."""
    rp = common["repetition_penalty"]
    start, f = common.get("exponential_decay_length_penalty", (0, None))
    seen, s = set(seen0), np.float64(0.0)
    for step, (t, x) in enumerate(zip(seq, lp)):
        x = np.float32(x) * np.float32(rp if int(t) in seen else 1.0)
        if f is not None and int(t) == 8193 and step - start > 0:
            x = x + np.abs(x) * np.float32(float(f) ** (step - start) - 1.0)
        s += np.float64(x)
        seen.add(int(t))
    return s


def lineage_errors(uv, gen, name, got):
    """| sequences_scores x length ** length_penalty - sum of the teacher-forced mel_logprobs of that sequence |, every returned hypothesis.
    Needs no reference: a row that did not inherit its parent's cache decodes from the wrong past, and its scores are another sequence's.
    (The tortoise cases: behind an acoustic prompt mel_logprobs has no prompt to condition on.)"""
    c = BC.E2E_CASES[name]
    refer, texts, prompt = case_inputs(gen, name)
    seqs, lens, scores = got
    lp = c["beam"]["length_penalty"]
    errs = []
    for u in range(c["U"]):
        rows = [seqs[u, j, : lens[u, j]] for j in range(c["nrs"])]
        lps = uv.mel_logprobs(refer[u:u + 1].repeat(c["nrs"], 1, 1), None, [texts[u]] * c["nrs"], None, rows)
        for j, row in enumerate(rows):
            want = penalised_sum(lps[j], row, {1, 8192}, c["common"])
            errs.append(abs(float(scores[u, j]) * float(len(row)) ** lp - want))
    return errs


LINEAGE_CASES = [n for n in E2E if not BC.E2E_CASES[n]["prompt_m"]]


def test_lineage_scores_are_the_sequences_own(rt, uv, gen):
    """the cache reorder's own test, and the hook that breaks it"""
    assert LINEAGE_CASES
    worst = 0.0
    for name in LINEAGE_CASES:
        errs = lineage_errors(uv, gen, name, run_device(rt, gen, name))
        print(f"lineage {name}: max |score x len^lp - teacher-forced sum| = {max(errs):.3e}")
        worst = max(worst, max(errs))
        assert max(errs) <= LINEAGE_TOL, (name, errs)
    name = "b3k5"                                     # its parents are not the identity (the penalty reshuffles the beams every step)
    rt.set_option("gpt_beam_skip_reorder", 1)
    try:
        broken = run_device(rt, gen, name)
    finally:
        rt.set_option("gpt_beam_skip_reorder", 0)
    errs = lineage_errors(uv, gen, name, broken)
    print(f"lineage {name} without the reorder: max error {max(errs):.3e}")
    assert max(errs) > 100 * LINEAGE_TOL, errs


def test_measured_score_error(rt, uv, gen):
    """Teacher-forced comparison behind E2E_MIN_GAP: the reference's running_beam_scores of EVERY step and beam against the device's
    teacher-forced log-probabilities of the same running sequence (printed: profiles/beam_measured_errors.txt holds the figures).
    The tortoise cases; valle_b1k3 is left out: the teacher-forced pass has no acoustic prompt (nor its fill id at mel position 0) to
    condition on.  Its sequences and sequences_scores are compared with the reference's like every other case's."""
    worst, count = 0.0, 0
    for name in LINEAGE_CASES:
        c = BC.E2E_CASES[name]
        refer, texts, _ = case_inputs(gen, name)
        for u in range(c["U"]):
            k = f"{name}.u{u}."
            steps = int(gen[k + "steps"])
            rows, refs = [], []
            for t in range(steps):
                for j in range(c["K"]):
                    if float(gen[k + "run_score"][t, j]) > -1.0e8:          # (a stopped continuation carries -1e9)
                        rows.append(gen[k + "run_seq"][t, j, : t + 1])
                        refs.append(float(gen[k + "run_score"][t, j]))
            lps = uv.mel_logprobs(refer[u:u + 1].repeat(len(rows), 1, 1), None, [texts[u]] * len(rows), None, rows)
            errs = [abs(penalised_sum(lps[i], row, {1, 8192}, c["common"]) - refs[i]) for i, row in enumerate(rows)]
            print(f"score error {name} u{u}: {len(rows)} running beams over {steps} steps, largest {max(errs):.3e}")
            worst, count = max(worst, max(errs)), count + len(rows)
    print(f"largest |device - reference| accumulated score over {count} running beams: {worst:.3e}  "
          f"(E2E_MIN_GAP = {BC.E2E_MIN_GAP:.1e} has to be >= 20 x it)")
    assert 20 * worst <= BC.E2E_MIN_GAP


def test_num_beams_one_is_todays_decode(rt, uv, gen):
    refer, texts, _ = case_inputs(gen, "b2k3")
    texts, tl = padded_texts(texts)
    kw = dict(do_sample=True, top_p=0.8, temperature=0.8, repetition_penalty=2.0, max_generate_length=12, seed=3, sample_ids=[5, 6], text_lengths=tl)
    base = uv.inference_speech_tortoise(refer, None, texts, **kw).cpu().numpy()
    for nb in (None, 1):
        got = uv.inference_speech_tortoise(refer, None, texts, num_beams=nb, length_penalty=1.0, **kw).cpu().numpy()
        assert np.array_equal(got, base), nb


def test_mirror_and_session_order(rt, uv, gen):
    """through UnifiedVoice (return_scores, last_latents None), and a beam call after a sampled call and the reverse give what each gives alone"""
    name = "b2k3"
    refer, texts, _ = case_inputs(gen, name)
    c = BC.E2E_CASES[name]
    texts, tl = padded_texts(texts)
    skw = dict(do_sample=True, top_p=0.8, temperature=0.8, repetition_penalty=2.0, max_generate_length=16, seed=3, sample_ids=[5, 6], text_lengths=tl)
    bkw = dict(num_beams=c["K"], num_return_sequences=c["nrs"], max_generate_length=16, return_scores=True, text_lengths=tl, **c["common"],
               **c["beam"])
    sampled = uv.inference_speech_tortoise(refer, None, texts, **skw).cpu().numpy()
    out, scores = uv.inference_speech_tortoise(refer, None, texts, **bkw)
    assert uv.last_latents is None
    again = uv.inference_speech_tortoise(refer, None, texts, **skw).cpu().numpy()
    assert np.array_equal(again, sampled)
    out2, scores2 = uv.inference_speech_tortoise(refer, None, texts, **bkw)
    assert np.array_equal(out.cpu().numpy(), out2.cpu().numpy()) and np.array_equal(scores.numpy(), scores2.numpy())
    out = out.cpu().numpy()
    G = 16
    out = np.concatenate([out, np.full((out.shape[0], G - out.shape[1]), 8193, out.dtype)], 1).reshape(c["U"], c["nrs"], G)
    check_against_reference(gen, name, (out, uv.last_ncodes.reshape(c["U"], c["nrs"]), scores.numpy().reshape(c["U"], c["nrs"])))


def test_refusals_come_before_a_launch(rt, uv, gen):
    refer, texts, _ = case_inputs(gen, "b1k2")
    texts = np.stack(texts)
    ok = dict(num_beams=2, max_generate_length=4)
    for bad in (dict(do_sample=True), dict(typical_sampling=True), dict(input_tokens=np.zeros((1, 2), np.int64)),
                dict(forced_uniforms=torch.zeros(1, 4).cuda()), dict(num_return_sequences=3), dict(num_beams=17),
                dict(early_stopping="sometimes"), dict(length_penalty=float("nan"))):
        with pytest.raises(ValueError):
            uv.inference_speech_tortoise(refer, None, texts, **dict(ok, **bad))
    with pytest.raises(ValueError):
        uv.inference_speech_tortoise(refer, None, texts, return_scores=True, max_generate_length=4)


# ---------------------------------------------------------------------------------------------------------------- infer / infer_gpt
@pytest.fixture(scope="module")
def synth(weights):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(weights, folded=True)


def public_case(gen, name="b2k3"):
    refer, texts, _ = case_inputs(gen, name)
    text, tl = padded_texts(texts)
    c = BC.E2E_CASES[name]
    common = dict(c["common"])
    common.pop("repetition_penalty")          # (infer decodes under the reference's own 2.0: not the fixture's sequences, beams all the same)
    opts = dict(num_beams=c["K"], **c["beam"], **common)
    return (torch.from_numpy(text), torch.tensor(tl), refer.cpu(), torch.tensor([refer.shape[2]] * refer.shape[0])), opts, common


PUBLIC_KW = dict(batch=True, seed=9, sample_ids=[21, 22], max_generate_length=16)


def test_infer_and_infer_gpt_under_beams(synth, gen):
    """decode_options={'num_beams': K, ...}: infer / infer_gpt decode with the beam search - the waveform is, bit for bit, the one the
    same call gives when the best hypothesis of Runtime.gpt_generate_beams is handed in as forced_codes (latents from the teacher-forced
    pass on the chosen codes, the same diffusion and vocoder noise) - and not the sampled decode's."""
    args, opts, common = public_case(gen)
    texts = [args[0][b, : int(args[1][b])].numpy().astype(np.int32) for b in range(2)]
    seqs, lens, _ = synth.rt.gpt_generate_beams(args[2].cuda(), [int(v) for v in args[3]], texts, opts["num_beams"], max_generate_length=16,
                                                 length_penalty=opts["length_penalty"], early_stopping=opts["early_stopping"],
                                                 repetition_penalty=2.0, processors=common)
    best = [seqs[b, 0, : lens[b, 0] - 1] for b in range(2)]
    assert all(len(c) >= 1 for c in best)
    wav = synth.infer(*args, diffusion_steps=4, decode_options=opts, **PUBLIC_KW)
    assert torch.equal(wav, synth.infer(*args, diffusion_steps=4, forced_codes=best, **PUBLIC_KW))
    sampled = synth.infer(*args, diffusion_steps=4, decode_options=common, **PUBLIC_KW)
    assert sampled.shape != wav.shape or not torch.equal(sampled, wav)
    wav = synth.infer_gpt(*args, decode_options=opts, **PUBLIC_KW)
    assert torch.equal(wav, synth.infer_gpt(*args, forced_codes=best, **PUBLIC_KW))


def test_public_refusals_on_a_live_model(synth, gen):
    """the refusals of tests/test_host_beam.py on a bound model: nothing is launched, the keyword is named"""
    args, opts, common = public_case(gen)
    reqs = [dict(text=args[0], text_length=args[1], refer=args[2], refer_lengths=args[3], seed=9, sample_ids=[21, 22])]
    with pytest.raises(ValueError, match="stream"):
        list(synth.infer_stream(iter(reqs), decode_options=opts, max_generate_length=16, diffusion_steps=4))
    forced = [[5229, 6940]] * 2
    for bad, key in ((dict(forced_codes=forced), "forced_codes"), (dict(num_candidates=2), "num_candidates"),
                     (dict(return_candidates=True), "return_candidates")):
        with pytest.raises(ValueError, match=key):
            synth.infer(*args, diffusion_steps=4, decode_options=opts, **PUBLIC_KW, **bad)
    with pytest.raises(ValueError, match="forced_codes"):
        synth.infer_gpt(*args, decode_options=opts, forced_codes=forced, **PUBLIC_KW)
    with pytest.raises(ValueError, match="num_beams"):
        synth.rt.gpt_generate(args[2].cuda(), None, [np.array([5, 0], np.int32)] * 2, 1, [0, 1], max_generate_length=4,
                              processors=dict(num_beams=2))
