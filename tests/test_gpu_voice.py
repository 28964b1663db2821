"""GPU: reusable voices (detail_tts_amd/voice.py, csrc/voice.hip).  The latents of one or many clips against the REFERENCE's
get_conditioning in float64 (tests/golden/make_golden_voice.py -> voice_latents.npz), the pool kernel against its numpy restatement bit
for bit, `speaker=` / `cond_latents=` against the `refer` form bit for bit on every entry, the latents-in decode against the
reference's compute_embeddings + generate (voice_generate.npz), broadcast and blend.  Measurements: profiles/voice_measured_errors.txt."""
import numpy as np
import pytest

from conftest import tol
from voice_ref import pool

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# device latents vs the reference's float64 values, max |diff| on values of magnitude ~1: 20 x the largest error measured over the four
# cases on the MI355X (profiles/voice_measured_errors.txt: 2.2e-7 for the gpt member, 3.5e-6 for the diffusion member)
GPT_GATE = 4.5e-6
DIFF_GATE = 7e-5
# a voice made ALONE (S = 1, its own T) vs the same clip as one row of a B = 2 rectangle: members, and the waveform of a
# forced-codes infer() with it (relative rms).  Measured 0.0 both (same file): the encoders' launches do not choose a summation order
# by the rectangle.  20 x 0 is 0, so the gate is the smallest figure that still reads as one: anything but equal bits misses it.
ALONE_MEMBER_GATE = 1e-9
ALONE_WAV_GATE = 1e-9
G = 12
KW = dict(batch=True, seed=3, sample_ids=[21, 22], max_generate_length=G, suppress_eos=True, diffusion_steps=4)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def model(weights):
    """the whole model with the optional gpt.text_head (gpt.forward's loss mode needs it)"""
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    from detail_tts_amd.weights import synthetic_state_dict
    P = dict(weights)
    P.update(synthetic_state_dict(0, only_prefixes=("gpt.text_head.",), optional=True))
    return SynthesizerTrn(P, folded=True)


@pytest.fixture(scope="module")
def gl(golden):
    return golden("voice_latents")


@pytest.fixture(scope="module")
def req():
    """B = 2, ragged prompt lengths (odd and even through both stride-2 convs, a masked tail in the MelStyle pool), texts of 6 and 4 ids"""
    rs = np.random.RandomState(21)
    refer = torch.from_numpy((rs.randn(2, 128, 64) * 2 - 5).astype(np.float32))
    text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (2, 5)), [[0], [0]]], 1).astype(np.int64))
    text[1, 3:] = 0
    return dict(text=text, tl=torch.tensor([6, 4]), refer=refer, rl=torch.tensor([50, 37]))


@pytest.fixture(scope="module")
def voice(model, req):
    return model.get_conditioning_latents(req["refer"], req["rl"])


# ------------------------------------------------------------------------------------------------------------ 1. latents vs the reference
@pytest.mark.parametrize("name", ["s2n3_eq", "s2n3_rag", "s1n2_rag", "s1n1_rag"])
def test_latents_against_the_reference(model, gl, name):
    """get_conditioning_latents on [S,n,128,T] vs the reference's two get_conditioning in float64; ragged clips vs the reference's modules
    on each clip cut to its length.  The mirrors' own 4-D get_conditioning are the same launches: the same bits."""
    refer, lens = gl[f"{name}_refer"], gl[f"{name}_lens"]
    ragged = name.endswith("rag")
    v = model.get_conditioning_latents(torch.from_numpy(refer), clip_lengths=lens if ragged else None)
    S, n = refer.shape[:2]
    assert v.S == S and v.dims == dict(gpt=768, diffusion=1536, vq=768)
    eg = float(np.abs(v.gpt.cpu().numpy().astype(np.float64) - gl[f"f64_{name}_gpt"]).max())
    ed = float(np.abs(v.diffusion.cpu().numpy().astype(np.float64) - gl[f"f64_{name}_diffusion"]).max())
    print(f"voice_{name}_gpt_maxabs {eg:.3e}  voice_{name}_diffusion_maxabs {ed:.3e}")
    tol(f"voice_{name}_gpt_maxabs", eg, GPT_GATE)
    tol(f"voice_{name}_diffusion_maxabs", ed, DIFF_GATE)
    assert float(np.abs(gl[f"f64_{name}_gpt"]).max()) > 0.1 and float(np.abs(gl[f"f64_{name}_diffusion"]).max()) > 0.1
    x = dev(refer)
    assert bits(model.gpt.get_conditioning(x, lens if ragged else None), v.gpt)
    assert bits(model.diffusion.get_conditioning(x, lens if ragged else None), v.diffusion)
    if n == 1:      # not pooled: the encoders' own outputs
        assert bits(model.rt.diff_conditioning(x[:, 0].contiguous(), lens.reshape(-1).tolist()), v.diffusion)
        assert bits(model.rt.mel_style("vq_ref_enc", x[:, 0].contiguous(), lens.reshape(-1).tolist()), v.vq)


def test_a_wrong_diffusion_weight_is_caught(model, gl):
    """clips of 37 / 50 / 64 frames: the PLAIN mean of the clips' embedder means is not the reference's mean over the concatenation - it
    misses the float64 value by 0.1, 1400 x DIFF_GATE - and the right weights are the embedder lengths 10 / 13 / 16"""
    name = "s2n3_rag"
    refer, lens = gl[f"{name}_refer"], gl[f"{name}_lens"]
    d = model.rt.diff_conditioning(dev(refer.reshape(6, 128, 64)), lens.reshape(-1).tolist()).view(2, 3, -1)
    want = gl[f"f64_{name}_diffusion"]
    plain = float(np.abs(model.rt.voice_pool(d).cpu().numpy() - want).max())
    by_frames = float(np.abs(model.rt.voice_pool(d, lens.astype(np.float32)).cpu().numpy() - want).max())
    right = float(np.abs(model.rt.voice_pool(d, np.array([[10, 13, 16], [16, 10, 13]], np.float32)).cpu().numpy() - want).max())
    print(f"voice_plain_mean_miss {plain:.3e}  voice_frame_weight_miss {by_frames:.3e}  right {right:.3e}")
    assert plain > 1000 * DIFF_GATE and abs(plain - float(gl[f"f64_{name}_plain_err"])) < 1e-3
    assert by_frames > 10 * DIFF_GATE          # weights l instead of ((l - 1) // 2 + 1 - 1) // 2 + 1: caught as well
    tol("voice_right_weights_maxabs", right, DIFF_GATE)


# ------------------------------------------------------------------------------------------------------------ 2. the pool kernel
def test_pool_kernel_equals_the_restatement_bit_for_bit(model):
    rt = model.rt
    rs = np.random.RandomState(2)
    v = (rs.randn(2, 3, 1536) * 3).astype(np.float32)
    w = np.array([[10, 13, 16], [16, 10, 13]], np.float32)
    for weights in (None, w, rs.rand(2, 3).astype(np.float32), np.array([[0, 2, 5], [1, 0, 0]], np.float32)):
        out = rt.voice_pool(dev(v), weights)
        assert out.cpu().numpy().tobytes() == pool(v, weights).tobytes()
        assert bits(rt.voice_pool(dev(v), weights), out)                    # two calls, the same bits
    # planted: float32 addition does not associate, the kernel adds in ascending j
    p = np.array([[[1e8, 1.0], [1.0, 1e8], [-1e8, -1e8]]], np.float32)
    assert rt.voice_pool(dev(p)).cpu().numpy().tobytes() == pool(p).tobytes() == np.array([[0.0, 0.0]], np.float32).tobytes()
    q = p[:, [0, 2, 1]]
    assert rt.voice_pool(dev(q)).cpu().numpy().tobytes() == pool(q).tobytes() != pool(p).tobytes()
    # D that is no multiple of the block, more speakers, n = 1: the input's bits (a negative zero, a denormal, a NaN payload)
    for S, n, D in ((3, 2, 300), (1, 8, 1), (5, 1, 257)):
        x = rs.randn(S, n, D).astype(np.float32)
        if n == 1:
            x[0, 0, :3] = np.array([-0.0, 1e-40, np.nan], np.float32)
        out = rt.voice_pool(dev(x))
        assert out.cpu().numpy().tobytes() == pool(x).tobytes()
        if n == 1:
            assert out.cpu().numpy().tobytes() == x[:, 0].tobytes()
    for bad in (np.array([[1, -1, 1], [1, 1, 1]], np.float32), np.zeros((2, 3), np.float32)):
        with pytest.raises(ValueError):
            rt.voice_pool(dev(v), bad)
    import ctypes as C
    from detail_tts_amd import _lib
    o = torch.zeros((2, 1536), device="cuda")
    nanw = np.array([[1, np.nan, 1], [1, 1, 1]], np.float32)               # the library checks too, before its launch
    rc = rt.lib.dtts_voice_pool(rt.h, C.c_void_p(dev(v).data_ptr()), nanw.ctypes.data_as(_lib.c_float_p), 2, 3, 1536, C.c_void_p(o.data_ptr()), rt._stream())
    assert rc != 0 and b"finite" in rt.lib.dtts_last_error(rt.h)


# ------------------------------------------------------------------------------------------------------------ 3. reuse, bit for bit
def test_infer_with_a_speaker_equals_infer_with_refer(model, req, voice):
    """the voice is computed by the same launches on the same rectangle, so every entry returns the refer form's bits"""
    a = (req["text"], req["tl"])
    want = model.infer(*a, req["refer"], req["rl"], **KW)
    got = model.infer(*a, None, None, speaker=voice, **KW)
    assert bits(got, want) and float(want.abs().max()) > 1e-4
    w2, c2 = model.infer(*a, req["refer"], req["rl"], return_candidates=True, num_candidates=2, **KW)
    g2, d2 = model.infer(*a, None, None, speaker=voice, return_candidates=True, num_candidates=2, **KW)
    assert bits(g2, w2) and np.array_equal(c2["codes"], d2["codes"]) and np.array_equal(c2["scores"], d2["scores"]) and c2["chosen"] == d2["chosen"]
    prompt = np.random.RandomState(4).randint(0, 8192, (2, 5))
    assert bits(model.infer(*a, None, None, speaker=voice, prompt_codes=prompt, **KW), model.infer(*a, req["refer"], req["rl"], prompt_codes=prompt, **KW))
    forced = [np.arange(5) + 100, np.arange(3) + 7]
    fkw = dict(KW, forced_codes=forced)
    assert bits(model.infer(*a, None, None, speaker=voice, **fkw), model.infer(*a, req["refer"], req["rl"], **fkw))
    skw = dict(KW, stream_vocoder=True, sampler="ddim", trunk_precision="fp32")
    assert bits(model.infer(*a, None, None, speaker=voice, **skw), model.infer(*a, req["refer"], req["rl"], **skw))


def test_beams_and_infer_gpt_with_a_speaker(model, req, voice):
    a = (req["text"], req["tl"])
    bkw = dict(KW, suppress_eos=False, decode_options=dict(num_beams=3, min_new_tokens=3))
    assert bits(model.infer(*a, None, None, speaker=voice, **bkw), model.infer(*a, req["refer"], req["rl"], **bkw))
    gkw = {k: v for k, v in KW.items() if k != "diffusion_steps"}
    want = model.infer_gpt(*a, req["refer"], req["rl"], **gkw)
    assert bits(model.infer_gpt(*a, None, None, speaker=voice, **gkw), want) and float(want.abs().max()) > 1e-4
    gb = dict(gkw, suppress_eos=False, decode_options=dict(num_beams=3, min_new_tokens=3))
    assert bits(model.infer_gpt(*a, None, None, speaker=voice, **gb), model.infer_gpt(*a, req["refer"], req["rl"], **gb))


def test_unified_voice_takes_cond_latents(model, req, voice):
    """inference_speech_tortoise / valle / forward / mel_logprobs with cond_latents= against the prompt-mel form: codes, last_latents,
    both losses and the logits, bit for bit"""
    uv, refer, rl = model.gpt, req["refer"].cuda(), req["rl"]
    text = req["text"].numpy()
    kw = dict(text_lengths=req["tl"], seed=5, sample_ids=[3, 4], max_generate_length=G, suppress_eos=True, top_p=0.8, temperature=0.8,
              repetition_penalty=2.0)
    want = uv.inference_speech_tortoise(refer, rl, text, **kw)
    wlat = uv.last_latents.clone()
    got = uv.inference_speech_tortoise(None, None, text, cond_latents=voice.gpt, **kw)
    assert torch.equal(got, want) and bits(uv.last_latents, wlat)
    prompt = np.random.RandomState(4).randint(0, 8192, (2, 5))
    assert torch.equal(uv.inference_speech_valle(None, None, text, prompt, cond_latents=voice.gpt, **kw),
                       uv.inference_speech_valle(refer, rl, text, prompt, **kw))
    bk = dict(text_lengths=req["tl"], max_generate_length=G, num_beams=3, repetition_penalty=2.0, min_new_tokens=2, return_scores=True)
    s1, sc1 = uv.inference_speech_tortoise(refer, rl, text, **bk)
    s2, sc2 = uv.inference_speech_tortoise(None, None, text, cond_latents=voice.gpt, **bk)
    assert torch.equal(s1, s2) and torch.equal(sc1, sc2)
    codes = np.random.RandomState(6).randint(0, 8192, (2, 7))
    f_ref = uv.forward(refer, rl, text, [6, 6], codes, [7 * 1024] * 2)
    f_lat = uv.forward(None, None, text, [6, 6], codes, [7 * 1024] * 2, cond_latents=voice.gpt)
    for x, y in zip(f_ref, f_lat):
        assert bits(x, y)
    assert bits(uv.forward(None, None, text, req["tl"], codes, [7 * 1024] * 2, return_latent=True, cond_latents=voice.gpt),
                uv.forward(refer, rl, text, req["tl"], codes, [7 * 1024] * 2, return_latent=True))
    lp_ref = uv.mel_logprobs(refer, rl, text, req["tl"], [codes[0], codes[1][:4]])
    lp_lat = uv.mel_logprobs(None, None, text, req["tl"], [codes[0], codes[1][:4]], cond_latents=voice.gpt)
    assert all(np.array_equal(x, y) for x, y in zip(lp_ref, lp_lat))


def test_infer_stream_with_speakers(model, req, voice):
    base = dict(text=req["text"], text_length=req["tl"], sample_ids=[21, 22])
    kw = dict(max_generate_length=G, suppress_eos=True, diffusion_steps=4)
    with_refer = [dict(base, refer=req["refer"], refer_lengths=req["rl"], seed=9 + i) for i in range(2)]
    with_voice = [dict(base, speaker=voice, seed=9 + i) for i in range(2)]
    want = [(w.clone(), list(n)) for w, n in model.infer_stream(iter(with_refer), **kw)]
    got = [(w.clone(), list(n)) for w, n in model.infer_stream(iter(with_voice), **kw)]
    assert len(got) == len(want) == 2
    for (gw, gn), (ww, wn) in zip(got, want):
        assert gn == wn and bits(gw, ww)
    # ... and two requests of one shared session, one naming its speaker by a voice, the other by its prompt mel
    mixed = [with_voice[0], with_refer[1]]
    got = [(w.clone(), list(n)) for w, n in model.infer_stream(iter(mixed), pair_stage_a=True, **kw)]
    pair = [(w.clone(), list(n)) for w, n in model.infer_stream(iter(with_refer), pair_stage_a=True, **kw)]
    for (gw, gn), (ww, wn) in zip(got, pair):
        assert gn == wn and bits(gw, ww)
    with pytest.raises(ValueError, match="both given"):
        list(model.infer_stream(iter([dict(with_refer[0], speaker=voice)]), **kw))


def test_a_timed_out_session_replays_from_the_kept_cond_vector(model, req, voice):
    """the session's replay record keeps the cond vector where it keeps the prompt mel: a session whose token kernel is declared dead
    (the handle's test hook) is replayed on the launch-per-GEMV chain and returns the chain's codes and latents"""
    rt = model.rt
    texts = [req["text"][0].numpy().astype(np.int32), req["text"][1, :4].numpy().astype(np.int32)]

    def gen():
        c, n, lat = rt.gpt_generate(None, None, texts, 5, [3, 4], max_generate_length=G, suppress_eos=True, cond=voice.gpt)
        return np.array(c), lat.clone()

    try:
        rt.set_option("gpt_token_kernel", 0)
        c_chain, l_chain = gen()
        rt.set_option("gpt_token_kernel", 1)
        rt.set_option("gpt_token_fault", 7)
        c1, l1 = gen()                               # 6 good tokens, a dead kernel from the 7th on, then the replay
        assert np.array_equal(c1, c_chain) and bits(l1, l_chain)
    finally:
        rt.set_option("gpt_token_kernel", 1)         # clears the latch
    c_ref, _, l_ref = rt.gpt_generate(req["refer"].cuda(), req["rl"].tolist(), texts, 5, [3, 4], max_generate_length=G, suppress_eos=True)
    c_tok, l_tok = gen()
    assert np.array_equal(c_tok, c_ref) and bits(l_tok, l_ref)


def test_a_voice_made_alone_serves_a_row_of_a_batch(model, req, voice):
    """across rectangles: speaker 1's voice made alone (S = 1, its own T = 37) against the same clip as row 1 of the B = 2 rectangle -
    other launches, so close, not equal: members, and the waveform of a forced-codes infer() with it"""
    alone = model.get_conditioning_latents(req["refer"][1:2, :, :37].contiguous())
    e = max(float((getattr(alone, k)[0] - getattr(voice, k)[1]).abs().max()) for k in ("gpt", "diffusion", "vq"))
    print(f"voice_alone_vs_row_member_maxabs {e:.3e}")
    tol("voice_alone_vs_row_member_maxabs", e, ALONE_MEMBER_GATE)
    a = (req["text"], req["tl"])
    fkw = dict(KW, forced_codes=[np.arange(5) + 100, np.arange(5) + 7])
    want = model.infer(*a, req["refer"], req["rl"], **fkw)
    mixed = type(voice)(torch.cat([voice.gpt[:1], alone.gpt]), torch.cat([voice.diffusion[:1], alone.diffusion]), torch.cat([voice.vq[:1], alone.vq]))
    got = model.infer(*a, None, None, speaker=mixed, **fkw)
    assert bits(got[0], want[0])                      # row 0 carries the rectangle's own latents
    rel = float((got[1] - want[1]).double().pow(2).mean().sqrt() / want[1].double().pow(2).mean().sqrt())
    print(f"voice_alone_vs_row_wav_relrms {rel:.3e}")
    tol("voice_alone_vs_row_wav_relrms", rel, ALONE_WAV_GATE)


# ------------------------------------------------------------------------------------------------------------ 4. latents in vs the reference
def test_latents_in_decode_returns_the_reference_tokens(model, golden):
    """cond_latents = the mean over n = 2 clips -> the tokens the reference's compute_embeddings + inference_model.generate returned"""
    g = golden("voice_generate")
    v = model.get_conditioning_latents(torch.from_numpy(g["refer"]))
    tol("voice_generate_cond_maxabs", float(np.abs(v.gpt.cpu().numpy().astype(np.float64) - g["f64_cond"]).max()), GPT_GATE)
    out = model.gpt.inference_speech_tortoise(None, None, g["text"], cond_latents=v.gpt, seed=int(g["seed"]), sample_ids=[int(g["sample_id"])],
                                              max_generate_length=int(g["G"]), do_sample=True, top_p=float(g["top_p"]),
                                              temperature=float(g["temperature"]), repetition_penalty=float(g["repetition_penalty"]),
                                              length_penalty=float(g["length_penalty"]))
    assert np.array_equal(out.cpu().numpy(), g["codes"]), (out, g["codes"])
    assert bits(model.gpt.get_conditioning(dev(g["refer"])), v.gpt)


# ------------------------------------------------------------------------------------------------------------ 5. broadcast, 6. blend
def test_one_voice_serves_every_row(model, req, voice):
    one = voice.rows(1)
    a = (req["text"], req["tl"])
    assert one.S == 1 and bits(model.infer(*a, None, None, speaker=one, **KW), model.infer(*a, None, None, speaker=voice.rows([1, 1]), **KW))
    gkw = {k: v for k, v in KW.items() if k != "diffusion_steps"}
    assert bits(model.infer_gpt(*a, None, None, speaker=one, **gkw), model.infer_gpt(*a, None, None, speaker=voice.rows([1, 1]), **gkw))
    with pytest.raises(ValueError, match="S has to be 1"):
        model.infer(*a, None, None, speaker=model.get_conditioning_latents(torch.cat([req["refer"], req["refer"][:1]])), **KW)


def test_blend(model, req, voice, tmp_path):
    from detail_tts_amd.voice import Voice
    a, b = voice.rows(0), voice.rows(1)
    only_a = Voice.blend([a, b], [1, 0])
    half = Voice.blend([a, b], [1, 1])
    third = Voice.blend([a, b], [0.5, 1.5])
    for k, t in a.members():
        assert bits(getattr(only_a, k), t), k
        pair = np.stack([t.cpu().numpy(), getattr(b, k).cpu().numpy()], 1)
        assert getattr(half, k).cpu().numpy().tobytes() == pool(pair).tobytes(), k
        assert getattr(third, k).cpu().numpy().tobytes() == pool(pair, np.array([[0.5, 1.5]], np.float32)).tobytes(), k
    args = (req["text"], req["tl"])
    wav = model.infer(*args, None, None, speaker=half, **KW)
    assert wav.shape[0] == 2 and bool(torch.isfinite(wav).all()) and float(wav.abs().max()) > 1e-4
    assert not bits(wav, model.infer(*args, None, None, speaker=a, **KW))
    path = str(tmp_path / "half.npz")
    half.save(path)
    again = Voice.load(path, model)
    assert again.gpt.is_cuda and bits(model.infer(*args, None, None, speaker=again, **KW), wav)
