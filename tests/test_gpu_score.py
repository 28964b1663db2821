"""GPU: dtts_gpt_score (csrc/gpt_score.hip: mel_head GEMM fused with an online log-sum-exp over V and the gather of the target logit),
UnifiedVoice.mel_logprobs and best-of-N candidates in SynthesizerTrn.infer.

GATE follows the project's 20 x rule (profiles/r06_measured_errors.txt): 20 x the largest absolute log-probability error of tests 1 - 4
below (against float64 numpy and against the reference's own values in tests/golden/gpt_score.npz), rounded up to one significant
digit.  PROVISIONAL: the value below is 20 x 9.0e-5, the largest error of an fp32 emulation of the same arithmetic on the CPU (numpy
fp32 GEMM + fp32 log-sum-exp against float64 on the shapes of test 1; the latents x 30 cases, whose logits reach 83, set it; unit-scale
latents give 5.6e-6) - no MI355X was available when this file was written, so these tests have NOT run on the device yet
(profiles/score_measured_errors.txt).  Whoever runs them first replaces the value by 20 x what every test below prints.  Either way
the gate stays below 1 / 100 of the fixture's log-probability spread (std 0.555), so a wrong gather cannot pass."""
import numpy as np
import pytest
from conftest import tol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GATE = 2e-3
V = 8194
EPS = 2.0 ** -24


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if np.size(a) else 0.0


def lse64(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))).squeeze(axis)


@pytest.fixture(scope="module")
def rt(weights):
    from detail_tts_amd.runtime import Runtime
    return Runtime(weights, folded=True, parts=("gpt",))


@pytest.fixture(scope="module")
def head64(weights):
    return np.asarray(weights["gpt.mel_head.weight"], np.float64), np.asarray(weights["gpt.mel_head.bias"], np.float64)


SHAPES = [(1, [1]), (1, [63]), (1, [65]), (3, [1, 65, 130]), (2, [0, 7])]


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("B,nts", SHAPES)
def test_kernel_vs_float64_numpy(rt, head64, B, nts, scale):
    """Random latents through the bound gpt.mel_head against float64: log-probabilities within GATE, raw logits within the worst-case
    fp32 bound of a 768-term dot product in ANY summation order, (768 + 2) * 2^-24 * (|W| |x| + |b|); exact zeros beyond ntargets; the
    V tail (targets 8192, 8193) and row 0; logsumexp(logits_out) reproduces logprob_out; two runs give the same bits.  scale 30 puts the
    logits in the hundreds, where a log-sum-exp without the running maximum overflows."""
    W, bias = head64
    n_max = max(nts)
    stride = n_max + 3
    rs = np.random.RandomState(100 * B + n_max)
    lat = (rs.randn(B, 768, stride) * scale).astype(np.float32)
    special = [0, 8192, 8193]
    codes = []
    for b, nt in enumerate(nts):
        c = rs.randint(0, V, nt)
        c[: min(nt, 3)] = np.roll(special, b)[: min(nt, 3)]
        if nt > 64:
            c[64] = 8193                                              # first column of the second wave pair / second tile region
        codes.append(c.astype(np.int32))
    lp, lg = rt.gpt_score(dev(lat), codes, want_logits=True)
    lp_only = rt.gpt_score(dev(lat), codes)
    lp2, lg2 = rt.gpt_score(dev(lat), codes, want_logits=True)
    lp, lg, lp_only, lp2, lg2 = host(lp), host(lg), host(lp_only), host(lp2), host(lg2)
    assert lp.shape == (B, n_max) and lg.shape == (B, V, n_max)
    assert np.array_equal(lp, lp2) and np.array_equal(lg, lg2) and np.array_equal(lp, lp_only)      # bit-identical runs, with and without logits_out
    x64 = lat.astype(np.float64)
    worst_lp, worst_lg, worst_self = 0.0, 0.0, 0.0
    for b, nt in enumerate(nts):
        assert np.all(lp[b, nt:] == 0.0), "columns beyond ntargets must be exactly 0.0"
        assert np.all(lg[b, :, nt:] == 0.0), "logits_out beyond ntargets is left untouched"
        if nt == 0:
            continue
        ref = W @ x64[b, :, :nt] + bias[:, None]                       # [V, nt]
        bound = (768 + 2) * EPS * (np.abs(W) @ np.abs(x64[b, :, :nt]) + np.abs(bias)[:, None])
        err = np.abs(lg[b, :, :nt].astype(np.float64) - ref)
        assert np.all(err <= bound), float((err / bound).max())
        worst_lg = max(worst_lg, float(err.max()))
        ref_lp = ref[codes[b], np.arange(nt)] - lse64(ref, 0)
        worst_lp = max(worst_lp, maxabs(lp[b, :nt], ref_lp))
        own = lg[b, :, :nt].astype(np.float64)
        worst_self = max(worst_self, maxabs(lp[b, :nt], own[codes[b], np.arange(nt)] - lse64(own, 0)))
    print(f"score_numpy B={B} nts={nts} scale={scale}: logprob err {worst_lp:.3e}, logit err {worst_lg:.3e}, vs own logits {worst_self:.3e}")
    tol(f"score_numpy_logprob_B{B}_n{n_max}_x{scale:g}", worst_lp, GATE)
    tol(f"score_numpy_selfconsistent_B{B}_n{n_max}_x{scale:g}", worst_self, GATE)


def test_empty_calls_and_argument_checks(rt):
    from detail_tts_amd.runtime import DttsError
    lat = dev(np.zeros((2, 768, 4)))
    out = rt.gpt_score(lat, [np.zeros(0, np.int32), np.zeros(0, np.int32)])         # B * n_max == 0: a no-op
    assert tuple(out.shape) == (2, 0)
    with pytest.raises(DttsError):
        rt.gpt_score(lat, [np.array([5, 8194]), np.array([1])])                     # target outside V, found on the host
    with pytest.raises(DttsError):
        rt.gpt_score(lat, [np.array([5, -1]), np.array([1])])
    with pytest.raises(DttsError):
        rt.gpt_score(lat, [np.arange(5), np.array([1])])                            # n_max > lat_stride
    with pytest.raises(DttsError):
        rt.gpt_score(lat, [np.array([1])])                                          # one code row per latent row


def test_forced_decode_logits_equal_reference_golden(rt, golden):
    """The decode-time latents of a forced decode, scored over columns 0 .. n with targets codes + [8193]: the kernel's raw logits at
    steps 0, 5 and n are the reference's own (gpt_forced.npz, GPT2InferenceModel's logits), and each log-probability is their log-softmax."""
    g = golden("gpt_forced")
    n = g["codes"].shape[1]
    codes, ncodes, lat = rt.gpt_generate(dev(g["refer"]), None, [g["text"][0]], 1, [0], max_generate_length=n + 1, forced_codes=[g["codes"][0]])
    assert ncodes[0] == n + 1 and codes[0, n] == 8193
    targets = np.concatenate([g["codes"][0], [8193]]).astype(np.int32)
    lp, lg = rt.gpt_score(lat, [targets], want_logits=True)
    lp, lg = host(lp), host(lg)
    steps = [int(s) for s in g["logits_steps"]]
    assert steps == [0, 5, n]
    ref = g["logits"].astype(np.float64)                                # [3, V]
    err_lg = maxabs(lg[0][:, steps].T, ref)
    ref_lp = ref[np.arange(3), targets[steps]] - lse64(ref, 1)
    err_lp = maxabs(lp[0, steps], ref_lp)
    print(f"score_forced: logit err {err_lg:.3e}, logprob err {err_lp:.3e}")
    tol("score_forced_logits", err_lg, GATE)
    tol("score_forced_logprob", err_lp, GATE)


def _score_rows(g, f):
    n = g["codes"].shape[1]
    rl, tl, nc = f["refer_lens"], f["text_lens"], f["ncodes"]
    assert int(nc[0]) == n
    refer = np.zeros((2,) + g["refer"].shape[1:], np.float32)
    text = np.zeros((2, g["text"].shape[1]), np.int64)
    for b in range(2):
        refer[b, :, : rl[b]] = g["refer"][0][:, : rl[b]]
        text[b, : tl[b]] = g["text"][0][: tl[b]]
    codes = [g["codes"][0][: int(nc[b])].astype(np.int32) for b in range(2)]
    return refer, [int(v) for v in rl], text, [int(v) for v in tl], codes


def test_mel_logprobs_vs_reference_golden(rt, golden):
    """UnifiedVoice.mel_logprobs on the ragged 2-row batch against the reference's own forward (gpt_score.npz); the same targets shifted
    by one position miss the gate by more than 10 x (the fixture discriminates); raw logits against the stored reference vectors."""
    from detail_tts_amd.config import load_config
    from detail_tts_amd.gpt.model import UnifiedVoice
    g, f = golden("gpt_forced"), golden("gpt_score")
    refer, rl, text, tl, codes = _score_rows(g, f)
    uv = UnifiedVoice(rt, load_config()["gpt"])
    lps = uv.mel_logprobs(torch.from_numpy(refer).cuda(), rl, text, tl, codes)
    assert [len(v) for v in lps] == [len(c) for c in codes] and all(v.dtype == np.float32 for v in lps)
    err = max(maxabs(lps[b], f["logprob"][b, : len(codes[b])]) for b in range(2))
    print(f"score_fixture: logprob err {err:.3e} (spread {float(f['spread']):.3f})")
    tol("score_fixture_logprob", err, GATE)
    assert GATE < float(f["spread"]) / 100
    shifted = [np.roll(c, 1) for c in codes]
    lps_s = uv.mel_logprobs(torch.from_numpy(refer).cuda(), rl, text, tl, shifted)
    # (teacher forcing: the shifted codes are also other INPUTS, so this is another sequence altogether - it must not look like the fixture)
    miss = max(maxabs(lps_s[b], f["logprob"][b, : len(codes[b])]) for b in range(2))
    assert miss > 10 * GATE, miss
    # the fixture's targets gathered one position late from the RIGHT latents
    lat = rt.gpt_latents(torch.from_numpy(refer).cuda(), rl, [text[b, : tl[b]].astype(np.int32) for b in range(2)], codes)
    late = host(rt.gpt_score(lat, shifted))
    miss2 = max(maxabs(late[b, : len(codes[b])], f["logprob"][b, : len(codes[b])]) for b in range(2))
    assert miss2 > 10 * GATE, miss2
    lp, lg = rt.gpt_score(lat, codes, want_logits=True)
    lg = host(lg)[0].astype(np.float64)
    steps = [int(s) for s in f["logits_steps"]]
    e_full = maxabs(lg[:, 5], f["logits_full"])
    e_tail = maxabs(lg[-4:, steps].T, f["logits_tail"])
    e_lse = maxabs(lse64(lg[:, steps], 0), f["f64_lse"])
    print(f"score_fixture: full logits err {e_full:.3e}, tail {e_tail:.3e}, lse {e_lse:.3e}")
    tol("score_fixture_logits_full", e_full, GATE)
    tol("score_fixture_logits_tail", e_tail, GATE)
    tol("score_fixture_lse", e_lse, GATE)


def test_decode_time_score_equals_teacher_forced(rt, golden):
    """A free-sampled 10-token decode (gpt_generate.npz): the score from the latents the decode left equals the score from the
    teacher-forced pass over the same codes."""
    g = golden("gpt_generate")
    codes, ncodes, lat = rt.gpt_generate(dev(g["refer"]), None, [g["text"][0]], int(g["seed"]), [int(g["sample_id"])], max_generate_length=10)
    assert np.array_equal(codes[0], g["codes"][0])
    c = codes[0, : int(ncodes[0])].astype(np.int32)
    s_dec = host(rt.gpt_score(lat, [c]))[0]
    lat_tf = rt.gpt_latents(dev(g["refer"]), None, [g["text"][0]], [c])
    s_tf = host(rt.gpt_score(lat_tf, [c]))[0]
    err = maxabs(s_dec, s_tf)
    print(f"score_decode_vs_teacher_forced: {err:.3e}  scores {s_dec}")
    assert np.all(s_dec < 0) and np.isfinite(s_dec).all()
    tol("score_decode_vs_teacher_forced", err, GATE)


# ---------------------------------------------------------------------------------------------------------------- infer, best of N
@pytest.fixture(scope="module")
def model(weights):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(weights, folded=True)


@pytest.fixture(scope="module")
def runs(model):
    """B = 2, N = 3, 8 tokens, 2 diffusion steps: the plain call and the candidate calls every infer test shares"""
    rs = np.random.RandomState(77)
    refer = torch.from_numpy((rs.randn(2, 128, 50) * 2 - 5).astype(np.float32))
    rl = [50, 33]
    text = np.zeros((2, 10), np.int64)
    text[0, :10] = np.concatenate([rs.randint(3, 255, 9), [0]])
    text[1, :6] = np.concatenate([rs.randint(3, 255, 5), [0]])
    tl = [10, 6]
    kw = dict(batch=True, seed=4321, sample_ids=[31, 32], max_generate_length=8, diffusion_steps=2)
    a = (torch.from_numpy(text), tl, refer, rl)
    out = dict(args=a, kw=kw, text=text, tl=tl, refer=refer, rl=rl)
    out["plain"] = model.infer(*a, **kw).cpu()
    out["n1"] = model.infer(*a, num_candidates=1, **kw).cpu()
    w, c = model.infer(*a, num_candidates=1, return_candidates=True, **kw)
    out["n1_cand"] = (w.cpu(), c)
    w, c = model.infer(*a, num_candidates=3, choose=[0, 0], return_candidates=True, **kw)
    out["c00"] = (w.cpu(), c)
    w, c = model.infer(*a, num_candidates=3, return_candidates=True, **kw)
    out["auto"] = (w.cpu(), c)
    return out


def test_infer_candidate_zero_is_the_default_call(runs):
    plain = runs["plain"]
    assert torch.isfinite(plain).all() and float(plain.abs().max()) > 0
    assert torch.equal(runs["n1"], plain)
    assert torch.equal(runs["n1_cand"][0], plain) and runs["n1_cand"][1]["chosen"] == [0, 0]
    w, c = runs["c00"]
    assert c["chosen"] == [0, 0] and c["codes"].shape[:2] == (2, 3) and c["scores"].shape == (2, 3)
    assert torch.equal(w, plain)
    # candidate 0 of the 3-candidate decode IS the 1-candidate decode
    assert np.array_equal(c["codes"][:, 0], runs["n1_cand"][1]["codes"][:, 0])
    assert np.array_equal(c["ncodes"][:, 0], runs["n1_cand"][1]["ncodes"][:, 0])


def test_infer_chooses_by_rank_candidates(model, runs):
    from detail_tts_amd.gpt.candidates import expand_sample_ids, rank_candidates
    w, c = runs["auto"]
    refer, rl, text, tl, kw = runs["refer"], runs["rl"], runs["text"], runs["tl"], runs["kw"]
    assert np.array_equal(c["codes"], runs["c00"][1]["codes"]) and np.array_equal(c["scores"], runs["c00"][1]["scores"])
    # the ranking, recomputed on the host from the TEACHER-FORCED log-probabilities of the returned codes
    chosen = []
    for b in range(2):
        rows = [c["codes"][b, k, : int(c["ncodes"][b, k])] for k in range(3)]
        lps = model.gpt.mel_logprobs(refer[b:b + 1].repeat(3, 1, 1).cuda(), [rl[b]] * 3, np.repeat(text[b:b + 1], 3, 0), [tl[b]] * 3, rows)
        best, scores = rank_candidates(lps, c["ncodes"][b], c["stopped"][b])
        assert float(np.abs(scores - c["scores"][b]).max()) < GATE, (scores, c["scores"][b])
        chosen.append(best)
    assert chosen == c["chosen"], (chosen, c)
    w2 = model.infer(*runs["args"], num_candidates=3, choose=c["chosen"], **kw).cpu()
    assert torch.equal(w2, w)
    # the candidates are inference_speech_tortoise's num_return_sequences rows on the expanded noise streams
    ids = expand_sample_ids(kw["sample_ids"], 3)
    from detail_tts_amd.config import REPETITION_PENALTY, TEMPERATURE, TOP_P
    out = model.gpt.inference_speech_tortoise(refer.cuda(), rl, text, text_lengths=tl, num_return_sequences=3, sample_ids=ids, seed=kw["seed"],
                                              max_generate_length=8, top_p=TOP_P, temperature=TEMPERATURE, repetition_penalty=REPETITION_PENALTY,
                                              top_k=50)
    flat = c["codes"].reshape(6, -1)
    assert np.array_equal(out.cpu().numpy(), flat[:, : out.shape[1]]), (out, flat)
