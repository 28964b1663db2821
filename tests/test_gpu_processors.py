"""HF's remaining decode-time logits processors on the DEVICE (csrc/gpt_kernels.hip: sampler_kernel): every case of
tests/golden/token_processor_edges.npz through dtts_op_sample_logits_opts, sixteen different rows in one launch, the reference's
generate() under each keyword (tests/golden/gpt_generate_processors.npz) through the mirror, and the public path's decode_options."""
import json

import numpy as np
import pytest

import processor_cases as P
import test_host_token_sampler as H
from test_host_processors import fixture_row

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS = 16          # GEMV_MAXB: rows of one sampler launch


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def rt(weights):
    from detail_tts_amd.runtime import Runtime
    return Runtime(weights, folded=True, parts=("gpt",))


@pytest.fixture(scope="module")
def edges(golden):
    return golden("token_processor_edges")


@pytest.fixture(scope="module")
def gen(golden):
    return golden("gpt_generate_processors")


def kwargs_of(params, opts):
    return dict(top_k=int(params["top_k"]), top_p=float(params["top_p"]), temperature=float(params["temp"]),
                repetition_penalty=float(params["rp"]), typical_mass=float(params["mass"]) or None, processors=opts)


def draw(rt, logits_row, row, us, **kw):
    """the device's token for every uniform of `us` on ONE row: 16 rows per launch (the row repeated, 16 uniforms)"""
    logits = dev(np.repeat(np.asarray(logits_row, np.float32)[None], ROWS, 0))
    got = []
    for i in range(0, len(us), ROWS):
        chunk = us[i:i + ROWS]
        got.extend(rt.op_sample_logits_opts(logits, [row["hist"]] * ROWS, [row["fills"]] * ROWS, [row["prompt_len"]] * ROWS,
                                            dev(np.resize(chunk, ROWS)), **kw).tolist()[:len(chunk)])
    return np.array(got)


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_device_sampler_on_the_processor_cases(rt, edges, name):
    """Every case, every row: the drawn token equals the inverse CDF of HF's filtered values at every probe, nothing HF removed is
    drawn, every kept token wide enough for a probe is drawn, u = 0 / u -> 1 give the first / last kept token."""
    logits, rows = P.case_inputs(name)
    assert P.input_hash(logits, rows) == str(edges[name + ".sha1"])
    for r in range(P.CASES[name]["R"]):
        kept, f = fixture_row(edges, name, r)
        assert np.array_equal(np.isfinite(P.restated(name, r, logits, rows)), kept)
        pr = H.make_probes(f, 1000 + r)
        assert pr["n_swept"] >= H.MIN_PROBES and pr["excluded_mass"] <= H.MAX_EXCLUDED_MASS
        got = draw(rt, logits[r], rows[r], pr["u"], **kwargs_of(P.CASES[name]["params"], P.case_options(name, r, logits)))
        want = pr["want"]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, r, bad.size, bad[:5], pr["u"][bad[:5]], got[bad[:5]], want[bad[:5]])
        assert set(got.tolist()) <= set(np.nonzero(kept)[0].tolist()), (name, r)
        assert set(pr["wide"].tolist()) <= set(got[:pr["n_swept"]].tolist()), (name, r)
        assert got[-3:].tolist() == [pr["first"], pr["last"], pr["last"]], (name, r)


def test_options_off_is_the_plain_entry(rt):
    """With every new field at its off value the new entry draws what dtts_op_sample_logits_ex draws."""
    rs = np.random.RandomState(91)
    x = (rs.randn(ROWS, P.V0) * 2.0).astype(np.float32)
    hist = rs.randint(2, P.V0, size=(ROWS, 8))
    u = rs.rand(ROWS).astype(np.float32)
    plain = rt.op_sample_logits(dev(x), np.concatenate([np.ones((ROWS, 1), np.int64), hist], 1), dev(u))
    for processors in (None, {}):
        got = rt.op_sample_logits_opts(dev(x), list(hist), [3] * ROWS, [4] * ROWS, dev(u), processors=processors)
        assert np.array_equal(got, plain)


SIXTEEN_OPTS = dict(no_repeat_ngram_size=2, min_new_tokens=3, exponential_decay_length_penalty=(1, 1.3), suppress_tokens=[7, 9],
                    begin_suppress_tokens=[11], min_p=0.01)
SIXTEEN_DRAWS = 8


def row_margin(x, row, params, opts, V):
    """smallest distance, in float64, of a cumulative probability to the top-p cut and of a p / p_max to min_p on a row the cases were
    not made for (test_host_token_sampler.py: row_cut_margin, processor_cases.py: warper_margin)"""
    plain = {k: v for k, v in opts.items() if k not in ("min_p", "epsilon_cutoff")}
    s = P.process_row(x, row, dict(params, top_p=1.0), plain, V).astype(np.float64)
    s = np.sort(s[np.isfinite(s)])
    cum = np.cumsum(np.exp(s - s.max()))
    cum /= cum[-1]
    out = float(np.abs(cum[:-1] - (1.0 - params["top_p"])).min()) if cum.size > 1 else np.inf
    s = P.process_row(x, row, params, plain, V).astype(np.float64)
    s = s[np.isfinite(s)]
    return min(out, float(np.abs(np.exp(s - s.max()) - opts["min_p"]).min()))


def test_sixteen_different_rows_in_one_launch(rt):
    """Sixteen rows with different logits, histories of different lengths (6 .. 1 596 ids), fill counts, prompt lengths and n-gram hits
    in ONE launch: every row gives the token of its own single-row launch, and the restatement's wherever the probe margins hold
    (tests/test_gpu_token_sampler.py::test_sixteen_different_rows_in_one_launch)."""
    V = P.V0
    rs = np.random.RandomState(78)
    x = (rs.randn(ROWS, V) * 2.0).astype(np.float32)
    rows, banned_counts = [], []
    for i in range(ROWS):
        n = (4, 9, 40, 300, 1580)[i % 5] + i
        body = rs.randint(2, 14 + 3 * i, size=n)
        hist = np.concatenate([[V - 2], body, body[:1]]).astype(np.int64)              # ends on its own first id: at least one hit
        fills = i % 4
        fresh = (0, 1, 2, 3, 5, 8, 13)[i % 7]                                          # tokens behind HF's prompt: every processor's on and off side
        rows.append(dict(hist=hist, fills=fills, prompt_len=fills + len(hist) - fresh))
        banned = P.banned_ngram_ids([1] * fills + hist.tolist(), 2)
        banned_counts.append(len(banned))
        x[i, sorted(banned)[:3]] = x[i].max() + np.float32(1.0)                      # a banned id on top: the hit decides the draw
    assert len(set(banned_counts)) >= 4 and min(banned_counts) >= 1
    params = dict(H.DEFAULTS, rp=1.3)
    kw = kwargs_of(params, SIXTEEN_OPTS)
    cdfs, sound = [], []
    for i in range(ROWS):
        f = P.process_row(x[i], rows[i], params, SIXTEEN_OPTS, V)
        cdfs.append(H.oracle_cdf(f))
        sound.append(row_margin(x[i], rows[i], params, SIXTEEN_OPTS, V) > H.CUT_MARGIN)
    compared = 0
    for _ in range(SIXTEEN_DRAWS):
        u = rs.rand(ROWS).astype(np.float32)
        packed = rt.op_sample_logits_opts(dev(x), [r["hist"] for r in rows], [r["fills"] for r in rows], [r["prompt_len"] for r in rows],
                                          dev(u), **kw)
        for i in range(ROWS):
            alone = rt.op_sample_logits_opts(dev(x[i:i + 1]), [rows[i]["hist"]], [rows[i]["fills"]], [rows[i]["prompt_len"]], dev(u[i:i + 1]), **kw)
            assert packed[i] == alone[0], (i, packed[i], alone[0])
            c, lo, _ = cdfs[i]
            v = int(H.inverse_cdf(c, np.float64(u[i])))
            if (c - lo)[v] >= H.MIN_WIDTH and min(u[i] - lo[v], c[v] - u[i]) >= H.EDGE_MARGIN:
                if sound[i]:
                    assert packed[i] == v, (i, packed[i], v)
                    compared += 1
    assert compared >= SIXTEEN_DRAWS * ROWS // 2, (compared, sound)


def _generate(uv, gen, name, with_option, **extra):
    common = json.loads(str(gen[name + ".common"]))
    opt = json.loads(str(gen[name + ".option"])) if with_option else {}
    for d in (common, opt):
        if "exponential_decay_length_penalty" in d:
            d["exponential_decay_length_penalty"] = tuple(d["exponential_decay_length_penalty"])
    n = 1 if name.startswith("input_tokens") else 2          # (the reference admits input_tokens for one prompt only: the first row)
    refer = torch.from_numpy(gen["refer"][:n]).cuda()
    if n == 1:
        extra = dict(extra, input_tokens=gen["input_tokens"])
    kw = dict(num_return_sequences=1, max_generate_length=int(gen["max_generate_length"]), seed=int(gen["seed"]),
              sample_ids=[int(gen["sample_id"]) + b for b in range(n)], **common, **opt, **extra)
    if name.startswith("valle"):
        out = uv.inference_speech_valle(refer, None, gen["text"][:n], gen["prompt"][:n], **kw)
    else:
        out = uv.inference_speech_tortoise(refer, None, gen["text"][:n], **kw)
    out = out.cpu().numpy()
    G = int(gen["max_generate_length"])
    return np.concatenate([out, np.full((out.shape[0], G - out.shape[1]), 8193, out.dtype)], 1)


GEN_SETS = ("no_repeat_ngram_size", "min_length", "min_new_tokens", "exponential_decay_length_penalty", "suppress_tokens",
            "begin_suppress_tokens", "min_p", "epsilon_cutoff", "valle_no_repeat_ngram_size", "all", "input_tokens_min_new_tokens",
            "valle_min_length")


@pytest.mark.parametrize("name", GEN_SETS)
def test_generate_under_each_keyword_matches_the_reference(rt, gen, name):
    """inference_speech_tortoise / inference_speech_valle with the keyword reproduce the reference's codes token for token (a decode
    that drops the keyword returns the recorded no-option codes, which differ); the same session replayed from the captured graphs
    (gpt_graph = 1) gives the same codes."""
    from detail_tts_amd.config import load_config
    from detail_tts_amd.gpt.model import UnifiedVoice
    assert name in [str(s) for s in gen["sets"]]
    uv = UnifiedVoice(rt, load_config()["gpt"])
    base = _generate(uv, gen, name, False)
    assert np.array_equal(base, gen[name + ".base"]), (name, base, gen[name + ".base"])
    codes = _generate(uv, gen, name, True)
    assert np.array_equal(codes, gen[name + ".codes"]), (name, codes, gen[name + ".codes"])
    rt.set_option("gpt_graph", 1)
    try:
        replayed = _generate(uv, gen, name, True)
    finally:
        rt.set_option("gpt_graph", 0)
    assert np.array_equal(replayed, codes), (name, replayed, codes)


def test_decay_at_the_default_length_is_served(rt):
    """HF's own documented example, exponential_decay_length_penalty = (15, 1.6), at the default max_generate_length of 600: factor^i - 1
    leaves float32 long before step 600, the table saturates and the call is served - every row draws the stop token a few dozen
    steps behind `start` (by i = 60 the multiplier is 1.8e12), none before the decay starts unless the plain decode stops there too."""
    rs = np.random.RandomState(31)
    B, G, start = 2, 600, 15
    refer = dev((rs.randn(B, 128, 40) * 2 - 5))
    texts = [np.concatenate([rs.randint(3, 255, 6), [0]]).astype(np.int32) for _ in range(B)]
    codes, ncodes, _ = rt.gpt_generate(refer, [40] * B, texts, 4, [51, 52], max_generate_length=G,
                                       processors=dict(exponential_decay_length_penalty=(start, 1.6)))
    plain, nplain, _ = rt.gpt_generate(refer, [40] * B, texts, 4, [51, 52], max_generate_length=start + 1)
    for b in range(B):
        assert start + 1 < ncodes[b] <= start + 1 + 60 and codes[b, ncodes[b] - 1] == 8193, (b, ncodes)
        assert np.array_equal(codes[b, :start + 1], plain[b, :start + 1])          # i <= 0 up to step `start`: the plain decode
    # ... and far behind the saturation point, through the unit entry: a row 1 500 tokens behind its prompt draws the stop token
    x = dev((rs.randn(1, P.V0) * 2.0))
    hist = rs.randint(2, P.V0 - 1, size=1520)
    got = rt.op_sample_logits_opts(x, [hist], [20], [40], dev(np.array([0.5])), processors=dict(exponential_decay_length_penalty=(start, 1.6)))
    assert got.tolist() == [P.V0 - 1]


@pytest.fixture(scope="module")
def synth(weights):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(weights, folded=True)


def public_request(B=2):
    """the smallest text, B utterances; `stoppy` makes the stop token likely (ids 0, 1 and the stop token alone are left)"""
    rs = np.random.RandomState(3)
    text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, 4)), np.zeros((B, 1), np.int64)], 1))
    refer = torch.from_numpy((rs.randn(B, 128, 40) * 2 - 5).astype(np.float32))
    return (text, torch.tensor([5] * B), refer, torch.tensor([40] * B)), dict(suppress_tokens=list(range(2, 8193)))


def test_infer_stream_decodes_under_the_options(synth):
    """infer_stream(decode_options=) gives, request by request, the waveform of infer(..., batch=True, decode_options=) bit for bit,
    and longer rows than the stream under min_new_tokens = 1 (the least that keeps the stop token from coming first, which the pipeline
    refuses)."""
    (text, tl, refer, rl), stoppy = public_request()
    opts = dict(stoppy, min_new_tokens=6)
    reqs = [dict(text=text, text_length=tl, refer=refer, refer_lengths=rl, seed=9 + i, sample_ids=[21, 22]) for i in range(2)]
    kw = dict(max_generate_length=12, diffusion_steps=4)
    got = [(w.clone(), np.array(n)) for w, n in synth.infer_stream(iter(reqs), decode_options=opts, **kw)]
    plain = [(w.clone(), np.array(n)) for w, n in synth.infer_stream(iter(reqs), decode_options=dict(stoppy, min_new_tokens=1), **kw)]
    assert len(got) == len(plain) == 2
    for i, r in enumerate(reqs):
        want = synth.infer(r["text"], r["text_length"], r["refer"], r["refer_lengths"], batch=True, seed=r["seed"], sample_ids=r["sample_ids"],
                           decode_options=opts, **kw)
        assert torch.equal(got[i][0], want), i
        assert (got[i][1] >= plain[i][1]).all() and (got[i][1] > plain[i][1]).any(), (i, got[i][1], plain[i][1])


def test_candidates_decode_under_the_options_and_score_unconstrained(synth):
    """infer(num_candidates=2, decode_options=): EVERY candidate decodes under the options (min_new_tokens: at least k codes in front of
    the stop token), and a candidate's score is the unconstrained model's mean log-probability of its codes - the teacher-forced
    log_softmax of UnifiedVoice.mel_logprobs, which knows nothing of the options - not the constrained distribution's (which, with
    three ids left, is above -log 3 per token on average only if the model agreed; here it lies far below)."""
    (text, tl, refer, rl), stoppy = public_request()
    k = 6
    out = synth.infer(text, tl, refer, rl, batch=True, seed=9, sample_ids=[21, 22], max_generate_length=12, diffusion_steps=4,
                      num_candidates=2, return_candidates=True, decode_options=dict(stoppy, min_new_tokens=k))
    cand = out[-1]
    assert cand["ncodes"].shape == (2, 2) and (cand["ncodes"] - 1 >= k).all(), cand["ncodes"]
    assert np.isin(cand["codes"], [0, 1, 8193]).all()
    for b in range(2):
        for c in range(2):
            row = cand["codes"][b, c, :cand["ncodes"][b, c]]
            lp = synth.gpt.mel_logprobs(refer[b:b + 1].cuda(), rl[b:b + 1], text[b:b + 1], tl[b:b + 1], [row])[0]
            assert abs(float(np.mean(lp.astype(np.float64))) - cand["scores"][b, c]) < 1e-3, (b, c, float(np.mean(lp)), cand["scores"][b, c])
            assert cand["scores"][b, c] < -np.log(3.0) - 1.0


def test_public_path_decode_options(synth):
    """infer_gpt(decode_options=dict(min_new_tokens=k)) on the smallest text: no row's code count is below k (the default decode of the
    same request stops earlier: the stop token is made likely by suppressing most of the vocabulary); decode_options = {} and None give
    today's waveform bit for bit."""
    m = synth
    (text, tl, refer, rl), stoppy = public_request()
    k, G = 6, 12
    kw = dict(batch=True, seed=9, sample_ids=[21, 22], max_generate_length=G)
    seen = {}
    orig = m.rt.gpt_generate

    def spy(*a, **k2):
        out = orig(*a, **k2)
        seen["ncodes"] = np.array(out[1])
        return out
    m.rt.gpt_generate = spy
    try:
        m.infer_gpt(text, tl, refer, rl, decode_options=stoppy, **kw)
        short = seen["ncodes"].copy()
        m.infer_gpt(text, tl, refer, rl, decode_options=dict(stoppy, min_new_tokens=k), **kw)
        long = seen["ncodes"].copy()
    finally:
        m.rt.gpt_generate = orig
    assert short.min() <= k, short                   # generated tokens + the stop token: fewer than k tokens in front of the stop
    assert (long - 1 >= k).all(), long
    w0 = m.infer_gpt(text, tl, refer, rl, **kw)
    for d in ({}, None):
        assert torch.equal(m.infer_gpt(text, tl, refer, rl, decode_options=d, **kw), w0)
    with pytest.raises(ValueError):
        m.infer_gpt(text, tl, refer, rl, decode_options=dict(min_p=2.0), **kw)
    with pytest.raises(ValueError):
        m.infer(text, tl, refer, rl, decode_options=dict(no_repeat_ngram_size=17), **kw)
