"""Host side of the reusable voices (detail_tts_amd/voice.py): the pool's restatement, the length weights against the reference's
float64 values, every refusal that has to come before a device call, and the .npz round trip.  No GPU."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from detail_tts_amd import voice as V      # noqa: E402
from detail_tts_amd.config import load_config      # noqa: E402
from voice_ref import pool      # noqa: E402

DIMS = dict(gpt=768, diffusion=1536, vq=768)


def make(S=1, seed=0, dims=DIMS, vq=True):
    rs = np.random.RandomState(seed)
    t = {k: torch.from_numpy(rs.randn(S, w).astype(np.float32)) for k, w in dims.items()}
    return V.Voice(t["gpt"], t["diffusion"], t["vq"] if vq else None)


class _NoDevice:
    """a model whose runtime must never be touched"""
    cfg = load_config()
    device = "cpu"

    @property
    def rt(self):
        raise AssertionError("device work before the arguments were checked")


class _Model:
    """what Voice.load reads of a model: its config, its device and the runtime the voice will launch on (none here)"""
    cfg, device, rt = load_config(), "cpu", None


class _NoRuntime:
    """a runtime nothing may be asked of"""
    def __getattr__(self, name):
        raise AssertionError(f"rt.{name} before the arguments were checked")


class _NoLibrary:
    """a Runtime whose library must never be touched"""
    def __init__(self):
        from detail_tts_amd.runtime import Runtime
        self._pad_text, self._prompt, self.cfg = Runtime._pad_text, Runtime._prompt, load_config()
        self._check_cond = lambda cond: Runtime._check_cond(self, cond)

    @property
    def lib(self):
        raise AssertionError("library call before the arguments were checked")


def test_pool_restatement():
    """the restatement is the weighted mean (against float64), in float32, with the kernel's two special cases"""
    rs = np.random.RandomState(1)
    v = rs.randn(2, 3, 1536).astype(np.float32)
    w = np.array([[9, 13, 16], [16, 9, 13]], np.float32)
    ref = (v.astype(np.float64) * w[:, :, None]).sum(1) / w.sum(1, dtype=np.float64)[:, None]
    out = pool(v, w)
    assert out.dtype == np.float32 and np.abs(out - ref).max() < 1e-6
    assert np.abs(pool(v) - v.astype(np.float64).mean(1)).max() < 1e-6
    # planted values: the order matters in float32 - (1e8 + 1) - 1e8 loses the 1, ascending j is what the kernel does
    p = np.array([[[1e8], [1.0], [-1e8]]], np.float32)
    assert pool(p)[0, 0] == np.float32(0.0) and pool(p[:, [0, 2, 1]])[0, 0] == np.float32(1.0) / np.float32(3.0)
    # n = 1 and "one live clip" copy the bits (w v / w does not: 13 * 0.1f / 13 != 0.1f)
    x = np.array([[[0.1, -0.0, 1e-40]]], np.float32)
    assert pool(x).tobytes() == x[:, 0].tobytes()
    two = np.concatenate([x, np.full_like(x, np.nan)], 1)
    assert pool(two, np.array([[13.0, 0.0]], np.float32)).tobytes() == x[:, 0].tobytes()
    assert (np.float32(13) * np.float32(0.1)) / np.float32(13) != np.float32(0.1)


def test_length_weights_reproduce_the_reference_mean(golden):
    """DiffusionTts.get_conditioning's mean over the concatenated embedder outputs == the mean of the clips' own means weighted by
    ((l - 1) // 2 + 1 - 1) // 2 + 1, on the reference's float64 values; the plain mean of ragged clips misses by ~0.1"""
    g = golden("voice_latents")
    assert [V.embedder_length(l) for l in (1, 2, 3, 4, 5, 37, 50, 64)] == [1, 1, 1, 1, 2, 10, 13, 16]
    for l in range(1, 70):          # conv k 3, stride 2, pad 1, twice
        assert V.embedder_length(l) == ((l + 2 - 3) // 2 + 1 + 2 - 3) // 2 + 1
    for name in g["cases"].tolist():
        lens, dclip, d = g[f"{name}_lens"], g[f"f64_{name}_dclip"], g[f"f64_{name}_diffusion"]
        w = np.vectorize(V.embedder_length)(lens).astype(np.float64)
        weighted = (dclip * w[:, :, None]).sum(1) / w.sum(1)[:, None]
        assert np.abs(weighted - d).max() < 1e-12, name
        plain = float(np.abs(dclip.mean(1) - d).max())
        assert abs(plain - float(g[f"f64_{name}_plain_err"])) < 1e-12
        assert (plain > 0.05) == (name in ("s2n3_rag", "s1n2_rag")), (name, plain)      # equal lengths: the plain mean IS the mean
        assert np.abs(g[f"{name}_gpt"] - g[f"f64_{name}_gpt"]).max() < 1e-6 and np.abs(g[f"{name}_diffusion"] - d).max() < 5e-6
    assert float(g["f64_s2n3_rag_plain_err"]) > 0.05 and float(g["f64_s1n2_rag_plain_err"]) > 0.05
    gg = golden("voice_generate")
    assert bool(gg["f64_agree"]) and gg["codes"].shape == (1, int(gg["G"])) and gg["refer"].shape == (1, 2, 128, 64)


def test_speaker_and_refer_exclude_each_other():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    text, tl, refer = torch.zeros((2, 4), dtype=torch.long), [4, 4], torch.zeros((2, 128, 8))
    me, v = _NoDevice(), make(2)
    for fn in (SynthesizerTrn.infer, SynthesizerTrn.infer_gpt):
        with pytest.raises(ValueError, match="both given"):
            fn(me, text, tl, refer, [8, 8], batch=True, speaker=v)
        with pytest.raises(ValueError, match="both given"):
            fn(me, text, tl, None, [8, 8], batch=True, speaker=v)
        with pytest.raises(ValueError, match="neither"):
            fn(me, text, tl, None, None, batch=True)
        with pytest.raises(ValueError, match="S has to be 1"):
            fn(me, text, tl, None, None, batch=True, speaker=make(3))
        with pytest.raises(ValueError, match="S has to be 1"):          # batch=False keeps one row
            fn(me, text, tl, None, None, speaker=make(2))
        with pytest.raises(ValueError, match="Voice.diffusion is 1024 wide"):
            fn(me, text, tl, None, None, batch=True, speaker=make(2, dims=dict(gpt=768, diffusion=1024, vq=768)))
        with pytest.raises(ValueError, match="has to be a Voice"):
            fn(me, text, tl, None, None, batch=True, speaker=torch.zeros(2, 768))
    with pytest.raises(ValueError, match="no vq member"):
        SynthesizerTrn.infer_gpt(me, text, tl, None, None, batch=True, speaker=make(2, vq=False))
    mel = torch.zeros((2, 128, 8))
    with pytest.raises(ValueError, match="both given"):
        SynthesizerTrn.invert_mel(me, mel, [8, 8], text, tl, refer, [8, 8], speaker=v)
    with pytest.raises(ValueError, match="neither"):
        SynthesizerTrn.invert_mel(me, mel, [8, 8], text, tl)
    with pytest.raises(ValueError, match="both given"):
        SynthesizerTrn.resynthesize(me, dict(codes=np.zeros((2, 2))), text, tl, refer=refer, refer_lengths=[8, 8], speaker=v)
    # a request dict of infer_stream goes through the same check
    from detail_tts_amd.pipeline import normalize_request
    with pytest.raises(ValueError, match="both given"):
        normalize_request(text, tl, refer, [8, 8], speaker=v, dims=DIMS)
    with pytest.raises(ValueError, match="S has to be 1"):
        normalize_request(text, tl, None, None, speaker=make(3), dims=DIMS)
    st = normalize_request(text, tl, None, None, speaker=make(1), dims=DIMS, seed=3)
    assert st.refer is None and st.voice.S == 1 and st.B == 2 and st.rl == [0, 0]


def test_gpt_entries_refuse_bad_cond_latents_before_any_launch():
    from detail_tts_amd.gpt.model import UnifiedVoice
    from detail_tts_amd.runtime import Runtime
    uv = UnifiedVoice(_NoRuntime(), load_config()["gpt"])
    refer, text = torch.zeros((1, 128, 8)), np.zeros((1, 4), np.int64)
    with pytest.raises(ValueError, match="have to be None"):
        uv.inference_speech_tortoise(refer, None, text, cond_latents=torch.zeros(1, 768))
    with pytest.raises(ValueError, match="have to be None"):
        uv.inference_speech_valle(None, [8], text, np.zeros((1, 2), np.int64), cond_latents=torch.zeros(1, 768))
    with pytest.raises(ValueError, match="neither"):
        uv.forward(None, None, text, [4], np.zeros((1, 2), np.int64), [2048])
    with pytest.raises(ValueError, match=r"\[B, 768\]"):
        uv.mel_logprobs(None, None, text, [4], [np.zeros(2, np.int64)], cond_latents=torch.zeros(1, 512))
    args = ([np.arange(4)], 0, [0])
    for fn in (Runtime.gpt_generate, Runtime.gpt_prefill):
        with pytest.raises(ValueError, match="one of the two"):
            fn(_NoLibrary(), refer, None, *args, cond=torch.zeros(1, 768))
        with pytest.raises(ValueError, match="one of the two"):
            fn(_NoLibrary(), None, None, *args)
        with pytest.raises(ValueError, match=r"\[B, 768\]"):
            fn(_NoLibrary(), None, None, *args, cond=torch.zeros(1, 512))
    with pytest.raises(ValueError, match="g_vq"):
        Runtime.vq_decode(_NoLibrary(), [np.arange(3)], refer, None, g_vq=torch.zeros(1, 768))
    with pytest.raises(ValueError, match=r"\[B, 768\]"):
        Runtime.vq_decode(_NoLibrary(), [np.arange(3)], None, None, g_vq=torch.zeros(1, 100))


def test_clip_lengths_are_checked_before_any_device_call():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    me = _NoDevice()
    x4, x3 = torch.zeros((2, 3, 128, 16)), torch.zeros((2, 128, 16))
    bad = [dict(clip_lengths=[[16, 0, 5], [1, 2, 3]]), dict(clip_lengths=[[16, 17, 5], [1, 2, 3]]), dict(clip_lengths=[[16, 16], [1, 2]]),
           dict(clip_lengths=[16, 16, 16]), dict(clip_lengths=[[1.5, 2, 3], [1, 2, 3]]), dict(refer_lengths=[16, 16])]
    for kw in bad:
        with pytest.raises(ValueError):
            SynthesizerTrn.get_conditioning_latents(me, x4, **kw)
    for kw in (dict(refer_lengths=[0, 16]), dict(refer_lengths=[16, 17]), dict(refer_lengths=[16]), dict(refer_lengths=[16, 16], clip_lengths=[[16], [16]])):
        with pytest.raises(ValueError):
            SynthesizerTrn.get_conditioning_latents(me, x3, **kw)
    with pytest.raises(ValueError, match="has to be"):
        SynthesizerTrn.get_conditioning_latents(me, torch.zeros((2, 16)))
    assert V.check_clips(x4, None, [[16, 1, 5], [1, 2, 3]]) == (2, 3, 16, [16, 1, 5, 1, 2, 3])
    assert V.check_clips(x3, [7, 16]) == (2, 1, 16, [7, 16]) and V.check_clips(x3, None, [[7], [16]]) == (2, 1, 16, [7, 16])
    assert V.check_clips(x4) == (2, 3, 16, [16] * 6)


def test_blend_refuses_bad_weights_and_unlike_voices():
    a, b = make(2, 1), make(2, 2)

    class _NoRt:
        def voice_pool(self, *args):
            raise AssertionError("launch before the weights were checked")

    # (3e38 twice: finite, but their float32 sum is not)
    for w in ([1, -1], [0, 0], [1, float("nan")], [1, float("inf")], [1], [1, 2, 3], [3e38, 3e38]):
        with pytest.raises(ValueError):
            V.Voice.blend([a, b], w, rt=_NoRt())
    with pytest.raises(ValueError, match="different shapes"):
        V.Voice.blend([a, make(1, 3)], [1, 1], rt=_NoRt())
    with pytest.raises(ValueError, match="different shapes"):
        V.Voice.blend([a, make(2, 3, vq=False)], [1, 1], rt=_NoRt())
    with pytest.raises(ValueError, match="no voices"):
        V.Voice.blend([], [], rt=_NoRt())
    w = V.check_weights([[1, 0], [2, 2]], 2, 2)
    assert w.dtype == np.float32 and w.tolist() == [[1, 0], [2, 2]]


def test_save_load_round_trips_bits_and_refuses_other_dimensions(tmp_path):
    v = make(2, 5)
    v.gpt[0, 0], v.gpt[0, 1] = -0.0, 1e-40          # a negative zero and a denormal survive
    path = os.path.join(tmp_path, "voice.npz")
    v.save(path)
    assert os.path.exists(path)
    w = V.Voice.load(path, _Model())
    assert w.S == 2 and w.dims == DIMS
    for k, t in v.members():
        assert getattr(w, k).numpy().tobytes() == t.numpy().tobytes(), k
    with pytest.raises(ValueError, match="Voice.diffusion is 1536 wide, the model's is 2048"):
        V.Voice.load(path, dims=dict(gpt=768, diffusion=2048, vq=768))
    with pytest.raises(ValueError, match="Voice.gpt"):
        V.Voice.load(path, dims=dict(gpt=1024, diffusion=1536, vq=768))
    nv = make(1, 6, vq=False)
    nv.save(path)
    w = V.Voice.load(path, _Model())
    assert w.vq is None and w.dims["vq"] is None and w.gpt.numpy().tobytes() == nv.gpt.numpy().tobytes()
    # rows / for_batch
    r = v.rows([1, 0])
    assert torch.equal(r.gpt[0], v.gpt[1]) and r.S == 2 and v.rows(1).S == 1 and v.rows(slice(0, 1)).S == 1
    with pytest.raises(ValueError):
        v.rows([2])
    one = v.rows(0).for_batch(3)
    assert one.S == 3 and torch.equal(one.diffusion[2], v.diffusion[0]) and v.for_batch(2) is v
    with pytest.raises(ValueError, match="S has to be 1 or B"):
        v.for_batch(3)
    assert V.model_dims(load_config()) == DIMS
