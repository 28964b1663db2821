"""GPU: UnifiedVoice.forward in loss mode (dtts_gpt_forward_losses: the teacher-forced pass of dtts_gpt_latents, gpt_score.hip once per
head - text_head V = 257, mel_head V = 8194 - and a fixed-order mean) against the reference's own forward (tests/golden/gpt_forward.npz,
make_golden_forward.py), and SynthesizerTrn.forward_gpt.

GATE = 2e-3 is the project's gate for this kernel's per-position log-probabilities and logits against the reference
(make_golden_score.py, tests/test_gpu_score.py).  The loss gates follow the 20 x rule on what test 1 measured on the MI355X
(profiles/forward_measured_errors.txt), per case and never looser than 2e-3 (a mean of values each within 2e-3 is within 2e-3):
case A 9.7e-5 (loss_text; loss_mel 7.2e-5) -> 20 x = 1.9e-3 -> 2e-3; case B 9.5e-7 -> 20 x = 1.9e-5 -> 2e-5.  SELF_GATE, the returned
log-probabilities against a float64 log-softmax of the returned logits (no reference involved): measured 1.4e-6 in both cases ->
20 x = 2.8e-5 -> 3e-5.  Measured per-position errors, case A / case B: text log-probabilities 5.6e-4 / 2.9e-6, mel log-probabilities
7.0e-4 / 3.8e-6, sampled mel logits 9.6e-4 / 3.9e-6.

Case A is two orders above case B for a reason that is not the kernels: its row 1 has a 40-frame prompt in a 64-frame batch.  The
reference's MelStyleEncoder runs its two k = 5 temporal convs over the padded frames as well (it masks before its attention and in the
pooling only), so its conditioning vector differs from the one the same prompt gives alone; this project's conditioning encoder
treats frames beyond cond_length as absent, here as everywhere.  The reference against itself (row 1 padded / cut to 40 frames) shows
exactly the measured gap: sampled mel logits 9.62e-4, loss_text 1.9e-4 and loss_mel 1.4e-4 (halved in the B = 2 means)."""
import numpy as np
import pytest
from conftest import tol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GATE = 2e-3
LOSS_GATE = {"a": 2e-3, "b": 2e-5}
SELF_GATE = 3e-5
V = 8194


def host(t):
    return t.detach().cpu().numpy()


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@pytest.fixture(scope="module")
def weights_head(weights):
    """the session's folded weights + the optional gpt.text_head tensors (their own Philox streams: nothing else changes)"""
    from detail_tts_amd.weights import synthetic_state_dict
    P = dict(weights)
    P.update(synthetic_state_dict(0, only_prefixes=("gpt.text_head.",), optional=True))
    assert P["gpt.text_head.weight"].shape == (257, 768)
    return P


@pytest.fixture(scope="module")
def rt(weights_head):
    from detail_tts_amd.runtime import Runtime
    return Runtime(weights_head, folded=True, parts=("gpt",))


@pytest.fixture(scope="module")
def uv(rt):
    from detail_tts_amd.config import load_config
    from detail_tts_amd.gpt.model import UnifiedVoice
    return UnifiedVoice(rt, load_config()["gpt"])


@pytest.fixture(scope="module")
def model(weights_head):
    """the whole model, for forward_gpt alone (it needs the VQ encoder next to the GPT)"""
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(weights_head, folded=True)


def case_inputs(golden, tag):
    f, g = golden("gpt_forward"), golden("gpt_forced")
    B = f[f"{tag}_text"].shape[0]
    refer = np.repeat(g["refer"], B, 0).copy()
    rl = [int(v) for v in f[f"{tag}_refer_lens"]]
    for b in range(B):
        refer[b, :, rl[b]:] = 0.0
    k = lambda name: f[f"{tag}_{name}"]
    return f, (torch.from_numpy(refer).cuda(), rl, torch.from_numpy(k("text").astype(np.int64)), torch.from_numpy(k("text_lens").astype(np.int64)),
               torch.from_numpy(k("codes").astype(np.int64)), torch.from_numpy(k("wav_lens").astype(np.int64)))


@pytest.fixture(scope="module")
def case_a(golden, uv):
    """case A's inputs and ONE forward on them, shared by the tests that compare other calls with it"""
    f, args = case_inputs(golden, "a")
    return f, args, uv.forward(*args)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_losses_logprobs_and_logits_equal_the_reference(rt, uv, golden, case_a, tag):
    """Case A (B = 2: a shorter prompt, a zero-padded text and codes that set_mel_padding rewrites in row 1) and case B (B = 1, 129
    positions per span: one past the score kernel's 128-column tile) through UnifiedVoice.forward: both losses, every per-position
    log-probability of both heads and the sampled mel logits against the reference's own values."""
    from detail_tts_amd.gpt.model import forward_inputs
    from forward_targets import aligned_inputs_and_targets
    if tag == "a":
        f, args, (loss_text, loss_mel, logits) = case_a
    else:
        f, args = case_inputs(golden, tag)
        loss_text, loss_mel, logits = uv.forward(*args)
    k = lambda name: f[f"{tag}_{name}"]
    B, Lt, n = k("text").shape[0], k("text").shape[1], k("codes").shape[1]
    for t in (loss_text, loss_mel):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 0
    assert tuple(logits.shape) == (B, V, n + 2) and logits.dtype == torch.float32
    # the per-position values, from the same entry on the same (preprocessed) inputs
    text, codes = forward_inputs(host(args[2]), host(args[3]), host(args[4]), host(args[5]))
    losses, logits2, tlp, mlp = rt.gpt_forward_losses(args[0], args[1], text, codes, want_logprobs=True)
    assert torch.equal(losses[0], loss_text) and torch.equal(losses[1], loss_mel) and torch.equal(logits2, logits)
    tlp, mlp, lg = host(tlp), host(mlp), host(logits)
    assert tlp.shape == (B, Lt + 2) and mlp.shape == (B, n + 2)
    e_t, e_m = maxabs(tlp, k("text_logprob")), maxabs(mlp, k("mel_logprob"))
    pos, rows = k("logit_pos"), f["logit_rows"]
    e_lg = maxabs(lg[:, rows][:, :, pos].transpose(0, 2, 1), k("logits"))
    e_lt, e_lm = abs(float(loss_text) - float(k("loss")[0])), abs(float(loss_mel) - float(k("loss")[1]))
    # the returned logits carry the returned log-probabilities (float64 log-softmax at the targets)
    _, _, _, mt = aligned_inputs_and_targets(text, codes)
    l64 = lg.astype(np.float64)
    m = l64.max(1, keepdims=True)
    ls = l64 - (m + np.log(np.exp(l64 - m).sum(1, keepdims=True)))
    e_self = maxabs(mlp, np.stack([ls[b, mt[b], np.arange(n + 2)] for b in range(B)]))
    print(f"forward_{tag}: loss_text {float(loss_text):.6f} (err {e_lt:.3e}), loss_mel {float(loss_mel):.6f} (err {e_lm:.3e}), text logprob err "
          f"{e_t:.3e}, mel logprob err {e_m:.3e}, logits err {e_lg:.3e}, vs own logits {e_self:.3e}")
    tol(f"forward_{tag}_text_logprob", e_t, GATE)
    tol(f"forward_{tag}_mel_logprob", e_m, GATE)
    tol(f"forward_{tag}_mel_logits", e_lg, GATE)
    tol(f"forward_{tag}_mel_logprob_vs_own_logits", e_self, SELF_GATE)
    tol(f"forward_{tag}_loss_text", e_lt, LOSS_GATE[tag])
    tol(f"forward_{tag}_loss_mel", e_lm, LOSS_GATE[tag])


def test_batch_of_17_equals_the_mean_of_its_rows(rt):
    """B = 17, Lt = 3, n = 2: the second row group of gpt_score holds one row.  Causal attention and no mask: a row of the rectangle is
    that row alone, and both losses are plain means over all B * positions - so the batched losses are the means of the seventeen B = 1
    losses (an fp32 mean of 17 terms is within 17 * 2^-24 = 1e-6 relative; 1e-5 leaves room for the rows' own rounding)."""
    rs = np.random.RandomState(17)
    B, Lt, n, Tr = 17, 3, 2, 24
    refer = torch.from_numpy((rs.randn(B, 128, Tr) * 2 - 5).astype(np.float32)).cuda()
    rl = [Tr - (b % 3) * 4 for b in range(B)]
    text, codes = rs.randint(1, 255, (B, Lt)), rs.randint(0, 8192, (B, n))
    losses, _, tlp, mlp = rt.gpt_forward_losses(refer, rl, text, codes, want_logits=False, want_logprobs=True)
    losses, tlp, mlp = host(losses).astype(np.float64), host(tlp), host(mlp)
    single = np.zeros((B, 2), np.float64)
    for b in range(B):
        l1, _, t1, m1 = rt.gpt_forward_losses(refer[b:b + 1].contiguous(), rl[b:b + 1], text[b:b + 1], codes[b:b + 1], want_logits=False, want_logprobs=True)
        single[b] = host(l1)
        assert maxabs(host(t1)[0], tlp[b]) < 1e-4 and maxabs(host(m1)[0], mlp[b]) < 1e-4, b       # row 16 (second group) like every other
    rel = np.abs(losses - single.mean(0)) / single.mean(0)
    print(f"forward_b17: batched {losses}, mean of rows {single.mean(0)}, rel {rel}")
    assert rel.max() < 1e-5, (losses, single.mean(0))
    # ... and the plain means of the per-position values the same call returned
    assert abs(-tlp.astype(np.float64).mean() - losses[0]) < 1e-5 * losses[0] and abs(-mlp.astype(np.float64).mean() - losses[1]) < 1e-5 * losses[1]


def test_losses_do_not_depend_on_return_logits_or_the_run(uv, case_a):
    _, args, (lt, lm, logits) = case_a
    lt0, lm0, none = uv.forward(*args, return_logits=False)
    assert none is None
    assert torch.equal(lt0, lt) and torch.equal(lm0, lm)
    lt2, lm2, logits2 = uv.forward(*args)
    assert torch.equal(lt2, lt) and torch.equal(lm2, lm) and torch.equal(logits2, logits)
    lt3, lm3, _ = uv.forward(*args, clip_inputs=True)                    # text_lengths.max() and wav_lengths.max() // 1024 are the full widths here
    assert torch.equal(lt3, lt) and torch.equal(lm3, lm)


def test_a_handle_without_the_head(weights, rt, golden):
    """no gpt.text_head in the blob: loss mode fails naming the tensor, everything else is as before"""
    from detail_tts_amd.config import load_config
    from detail_tts_amd.gpt.model import UnifiedVoice
    from detail_tts_amd.runtime import DttsError, Runtime
    assert "gpt.text_head.weight" not in weights
    rt0 = Runtime(weights, folded=True, parts=("gpt",))
    uv0 = UnifiedVoice(rt0, load_config()["gpt"])
    _, args = case_inputs(golden, "a")
    with pytest.raises(DttsError, match="gpt.text_head.weight"):
        uv0.forward(*args)
    lat = uv0.forward(*args, return_latent=True)
    texts = [host(args[2])[b, : int(args[3][b])].astype(np.int32) for b in range(2)]
    codes = host(args[4]).astype(np.int32).copy()
    codes[1, 6:] = 8193                                                 # set_mel_padding: wav_length 5 * 1024
    ref = rt0.gpt_latents(args[0], args[1], texts, [codes[0], codes[1]])
    assert torch.equal(lat, ref.permute(0, 2, 1).contiguous())
    assert torch.equal(rt.gpt_latents(args[0], args[1], texts, [codes[0], codes[1]]), ref)      # binding the head changes no latent


def test_forward_gpt_is_the_weighted_sum_of_an_explicit_encode_and_forward(model):
    """vqvae/model_24k.py:697-704 on B = 2, T = 64 mel frames (16 codes; row 1's wav_length makes set_mel_padding rewrite its tail)"""
    rs = np.random.RandomState(64)
    data = dict(raw_mel=torch.from_numpy((rs.randn(2, 128, 64) * 2 - 5).astype(np.float32)), raw_spec_length=torch.tensor([64, 48]),
                mel=torch.from_numpy((rs.randn(2, 128, 40) * 2 - 5).astype(np.float32)), spec_length=torch.tensor([40, 33]),
                text=torch.from_numpy(rs.randint(1, 255, (2, 6))), text_length=torch.tensor([6, 4]), raw_wav_length=torch.tensor([64 * 256, 48 * 256]))
    loss = model.forward_gpt(None, None, data)
    assert loss.is_cuda and loss.dtype == torch.float32 and loss.dim() == 0 and bool(torch.isfinite(loss))
    code, _ = model.encode(data["raw_mel"], data["raw_spec_length"])
    assert tuple(code.shape) == (2, 16)
    lt, lm, logits = model.gpt(data["mel"].cuda(), data["spec_length"], data["text"], data["text_length"], code, data["raw_wav_length"])
    assert tuple(logits.shape) == (2, V, 18)
    assert (model.text_loss_weight, model.mel_loss_weight) == (0.01, 1)
    assert torch.equal(loss, lt * 0.01 + lm)
    assert np.log(257) * 0.9 < float(lt) < np.log(257) * 1.2 and np.log(V) * 0.9 < float(lm) < np.log(V) * 1.2      # random init: near uniform


@pytest.mark.parametrize("bad_text,bad_code", [(257, None), (-1, None), (None, 8194), (None, -1)])
def test_out_of_range_ids_are_rejected_on_the_host(rt, uv, bad_text, bad_code):
    from detail_tts_amd.runtime import DttsError
    refer = torch.zeros((1, 128, 16), device="cuda")
    text, codes = np.array([[5, 6, 7]]), np.array([[1, 2]])
    if bad_text is not None:
        text[0, 1] = bad_text
    if bad_code is not None:
        codes[0, 1] = bad_code
    with pytest.raises(DttsError, match="text id outside" if bad_text is not None else "mel code outside"):
        rt.gpt_forward_losses(refer, None, text, codes)
    with pytest.raises(DttsError):
        uv.forward(refer, [16], torch.from_numpy(text), [3], torch.from_numpy(codes), [2048])
