"""GPU: the unconditional code-path cache (option "uncond_cache_mb", csrc/uncond_cache.h) is invisible - a call served from it, the
call that filled it and a call with the cache off give the same bits - and its counters say what it did.

Shapes.  The cache serves only where no launch of the pre-pass takes conv split-K or the attention's key split, with every
unconditional row present and with none (Model::integ_unsplit).  The narrowest launch is layer 0's front on the B conditional rows
alone: 6 M tiles x ceil(T / 192) N tiles x B samples must exceed the 128 tiles below which conv_x3 splits K, i.e. B ceil(T / 192) >= 22.
B = 8 with three N tiles per sample (385 <= T <= 576) is the smallest batch of eight past that threshold (24 x 6 = 144 tiles; B = 7
would be 126); every chunk launch is wider and holds more than the two samples up to which the attention splits its keys.  B = 3,
T = 193 (36 tiles) lies inside the split regime.  Five steps of the default schedule: with B + Nu = 9 samples per step the pre-pass
takes J = 4 steps per launch (one full launch, one of a single step), with B + Nu = 16 J = 2 (2 + 2 + 1)."""
import numpy as np
import pytest

from conv_tile_probe import launches_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 8
N_STEPS = 5
MB = 256                                   # dozens of these slabs (5 x 768 x T floats: 5.6 MiB at T = 385)


@pytest.fixture(scope="module")
def rt(weights):
    from detail_tts_amd.runtime import Runtime
    r = Runtime(weights, folded=True, parts=("diffusion",))
    yield r
    r.set_option("uncond_cache_mb", 0)


def code_emb(seed, b, T):
    return torch.from_numpy((np.random.RandomState(seed).randn(b, 768, T) * 0.5).astype(np.float32)).cuda()


def reset(rt, mb=MB):
    """an empty cache of `mb` MiB"""
    rt.set_option("uncond_cache_mb", 0)
    rt.set_option("uncond_cache_mb", mb)


def sample(rt, ce, lens, seed=7, **kw):
    out = rt.diff_sample_ex(ce, seed, list(range(ce.shape[0])), lens=lens, n_steps=kw.pop("n_steps", N_STEPS), **kw).clone()
    assert bool(torch.isfinite(out).all())
    return out


def off(rt, ce, lens, **kw):
    """the reference of a test: the call with the cache off.  (Switching it off drops it: every test takes its references first.)"""
    rt.set_option("uncond_cache_mb", 0)
    return sample(rt, ce, lens, **kw)


def delta(rt, before):
    now = rt.uncond_cache_stats()
    return {k: now[k] - before[k] for k in ("hits", "misses", "bypasses", "evictions")}


# on (384), one past (385) and inside (300, 77) the 192-column conv tile; 193 / 192 / 191 around the first boundary
RAGGED = [385, 384, 383, 300, 193, 192, 191, 77]


@pytest.mark.parametrize("cfg_streams", [1, 2])
@pytest.mark.parametrize("lens", [[384] * B, [385] * B, RAGGED], ids=["Nu1_on_tile", "Nu1_past_tile", "NuB"])
def test_off_cold_warm_are_the_same_bits(rt, lens, cfg_streams):
    """T1: cache off, the call that fills it and the call it serves; the pre-pass of the served call is narrower by Nu rows per step"""
    ce, nu = code_emb(11, B, 385), len(set(lens))
    rt.set_option("cfg_streams", cfg_streams)
    try:
        ref = off(rt, ce, lens)
        reset(rt)
        s0 = rt.uncond_cache_stats()
        cold = sample(rt, ce, lens)
        d = delta(rt, s0)
        assert d == dict(hits=0, misses=nu, bypasses=0, evictions=0), d
        assert rt.uncond_cache_stats()["entries"] == nu and rt.uncond_cache_stats()["bytes"] == nu * N_STEPS * 768 * 385 * 4
        s1 = rt.uncond_cache_stats()
        warm = sample(rt, ce, lens)
        d = delta(rt, s1)
        assert d == dict(hits=nu, misses=0, bypasses=0, evictions=0), d
        assert torch.equal(cold, ref), float((cold - ref).abs().max())
        assert torch.equal(warm, ref), float((warm - ref).abs().max())
    finally:
        rt.set_option("cfg_streams", 0)


def test_one_length_under_two_padded_widths(rt):
    """T2: a length cached where it is the batch's maximum, then used in a wider batch.  The GroupNorm pass sums a row in an order
    that follows the padded width, so the key holds (len, T): the second call must not be served the first one's slab, and equals cache
    off bit for bit."""
    ce, lens = code_emb(13, B, 576), [576, 500, 500, 576, 500, 500, 500, 576]
    ref = off(rt, ce, lens)
    reset(rt)
    sample(rt, code_emb(12, B, 500), [500] * B)
    s0 = rt.uncond_cache_stats()
    out = sample(rt, ce, lens)
    assert delta(rt, s0) == dict(hits=0, misses=2, bypasses=0, evictions=0)
    assert torch.equal(out, ref)
    s1 = rt.uncond_cache_stats()
    assert torch.equal(sample(rt, ce, lens), ref)
    assert delta(rt, s1)["hits"] == 2 and rt.uncond_cache_stats()["entries"] == 3


def test_partial_hit(rt):
    """T3: one length cached, one not: the call evaluates the missing one only, equals cache off, and leaves both cached"""
    ce, lens = code_emb(14, B, 450), [400, 430] * (B // 2)
    ref = off(rt, ce, lens)
    reset(rt)
    sample(rt, ce, [400] * B)
    s0 = rt.uncond_cache_stats()
    out = sample(rt, ce, lens)
    assert delta(rt, s0) == dict(hits=1, misses=1, bypasses=0, evictions=0)
    assert torch.equal(out, ref)
    assert rt.uncond_cache_stats()["entries"] == 2
    s1 = rt.uncond_cache_stats()
    assert torch.equal(sample(rt, ce, lens), ref)
    assert delta(rt, s1) == dict(hits=2, misses=0, bypasses=0, evictions=0)


def test_split_regime_stands_aside(rt):
    """T4: B = 3, T = 193 - 36 tiles per conv launch of layer 0's front, inside split-K: counted as a bypass, nothing stored"""
    ce, lens = code_emb(15, 3, 193), [193, 77, 193]
    ref = off(rt, ce, lens)
    reset(rt)
    s0 = rt.uncond_cache_stats()
    a = sample(rt, ce, lens)
    b = sample(rt, ce, lens)
    assert delta(rt, s0) == dict(hits=0, misses=0, bypasses=2, evictions=0)
    assert rt.uncond_cache_stats()["entries"] == 0
    assert torch.equal(a, ref) and torch.equal(b, ref)


def test_key_and_invalidation(rt, weights):
    """T5: another schedule (step count) or the DPM-Solver++ sampler's schedule is not served the default schedule's rows; a rebind on
    other weights serves nothing of the old binding and equals a runtime that never cached; conv_x3 = 0 and the pinned entry
    diff_reverse_step neither read nor write the cache."""
    from detail_tts_amd.runtime import Runtime
    ce, lens = code_emb(16, B, 400), [400] * B
    sched7 = rt.diff_schedule(list(range(0, 4000, 4000 // 7))[:7])
    dpm = rt.diff_schedule_dpm(6)
    ref, ref7 = off(rt, ce, lens), off(rt, ce, lens, sched=sched7)
    ref_dpm, ref_ddim = off(rt, ce, lens, sched=dpm, sampler=2, n_steps=0), off(rt, ce, lens, sampler=1)
    reset(rt)
    first = sample(rt, ce, lens)
    assert torch.equal(first, ref)
    s0 = rt.uncond_cache_stats()
    assert torch.equal(sample(rt, ce, lens, sched=sched7), ref7)
    assert delta(rt, s0) == dict(hits=0, misses=1, bypasses=0, evictions=0)
    s0 = rt.uncond_cache_stats()
    assert torch.equal(sample(rt, ce, lens, sched=dpm, sampler=2, n_steps=0), ref_dpm)
    assert delta(rt, s0) == dict(hits=0, misses=1, bypasses=0, evictions=0)
    # the DDIM sampler on the default schedule reads the SAME code-path rows as p_sample: served
    s0 = rt.uncond_cache_stats()
    assert torch.equal(sample(rt, ce, lens, sampler=1), ref_ddim)
    assert delta(rt, s0) == dict(hits=1, misses=0, bypasses=0, evictions=0)
    # neither read nor written: the exact fp32 kernels, and a pinned entry
    s0 = rt.uncond_cache_stats()
    rt.set_option("conv_x3", 0)
    try:
        sample(rt, ce, lens)
    finally:
        rt.set_option("conv_x3", 1)
    x = torch.from_numpy(np.random.RandomState(3).randn(B, 128, 400).astype(np.float32)).cuda()
    rt.diff_reverse_step(x, ce, 3, sched7, lens=lens)
    s1 = rt.uncond_cache_stats()
    assert delta(rt, s0) == dict(hits=0, misses=0, bypasses=2, evictions=0) and s1["entries"] == s0["entries"] and s1["bytes"] == s0["bytes"]
    # a rebind on other weights
    fresh = Runtime(weights, folded=True, parts=("diffusion",))
    fresh.set_option("uncond_cache_mb", 0)
    keep = rt.blob.clone()
    try:
        rt.blob.mul_(1.0 + 2.0 ** -10)
        rt.rebind()
        fresh.blob.copy_(rt.blob)
        fresh.rebind()
        s0 = rt.uncond_cache_stats()
        out = sample(rt, ce, lens)
        assert delta(rt, s0) == dict(hits=0, misses=1, bypasses=0, evictions=0)
        assert torch.equal(out, sample(fresh, ce, lens))
        assert not torch.equal(out, first)
        assert torch.equal(sample(rt, ce, lens), out) and delta(rt, s0)["hits"] == 1
    finally:
        rt.blob.copy_(keep)
        rt.rebind()
    assert torch.equal(sample(rt, ce, lens), first)


def test_eviction_and_budget_zero(rt):
    """T6: a budget of one slab (5.64 MiB in 6 MiB) and two lengths alternating: every call equals cache off and every call after the
    first gives the other length's slab up.  Budget 0 launches the uncached sequence (the counts of tests/test_gpu_sampler_preamble.py);
    so do the filling and the served call, whose launches only cover fewer samples."""
    ce = code_emb(17, B, 385)
    lens_a, lens_b = [384] * B, [385] * B
    ref_a, ref_b = off(rt, ce, lens_a), off(rt, ce, lens_b)
    reset(rt, 6)
    s0 = rt.uncond_cache_stats()
    for i in range(3):
        assert torch.equal(sample(rt, ce, lens_a), ref_a), i
        torch.cuda.synchronize()                     # a slab is given up only once the copies out of it have completed
        assert torch.equal(sample(rt, ce, lens_b), ref_b), i
        torch.cuda.synchronize()
    assert delta(rt, s0) == dict(hits=0, misses=6, bypasses=0, evictions=5)
    assert rt.uncond_cache_stats()["entries"] == 1
    rt.set_option("cfg_streams", 2)
    try:
        counts = []
        for i, what in enumerate(("off", "filling", "served")):
            if i < 2:
                reset(rt, 0 if what == "off" else MB)
            _, ran = launches_of(rt, lambda: sample(rt, ce, lens_a), level=2)
            counts.append({k: v for k, v in ran.items() if k.startswith(("conv_", "flash_attn", "gn_", "split_"))})
        assert rt.uncond_cache_stats()["hits"] - s0["hits"] == 1
    finally:
        rt.set_option("cfg_streams", 0)
        reset(rt)
    c = -(-N_STEPS // 4)                             # J = 36 // 9 steps per pre-pass launch
    convs = sum(n for k, n in counts[0].items() if k.startswith("conv_"))
    assert convs == 48 * 2 * N_STEPS + 12 * c + 1
    assert counts[0].get("split_planes_kernel", 0) == N_STEPS + c and counts[0].get("gn_split_planes_kernel", 0) == 37 * 2 * N_STEPS + 8 * c + 1
    assert counts[1] == counts[0] and counts[2] == counts[0], counts


# ---- T7: across streams ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    return SynthesizerTrn(select_inference_params(synthetic_state_dict(0, variant="signal")), folded=True)


def test_infer_stream_cold_then_warm_equals_blocking_infer(synth):
    """Three requests of eight utterances x 100 codes (T = 400) x 5 sampling steps through infer_stream - the first fills the cache on
    stage B's stream, the next two are served from it beside stage A and stage C of their neighbours - against blocking infer()."""
    rs = np.random.RandomState(23)
    reqs = []
    for i in range(3):
        refer = torch.from_numpy((rs.randn(B, 128, 200) * 2 - 5).astype(np.float32)).cuda()
        text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, 20)), np.zeros((B, 1), np.int64)], 1).astype(np.int32))
        reqs.append(dict(text=text, text_length=torch.full((B,), 21), refer=refer, refer_lengths=torch.full((B,), 200), seed=700 + i,
                         sample_ids=[10 * i + b for b in range(B)]))
    rt = synth.rt
    reset(rt)
    s0 = rt.uncond_cache_stats()
    outs = list(synth.infer_stream(iter(reqs), max_generate_length=101, suppress_eos=True, diffusion_steps=5))
    assert delta(rt, s0) == dict(hits=2, misses=1, bypasses=0, evictions=0)
    for i, (r, (wav, lens)) in enumerate(zip(reqs, outs)):
        ref, rlens = synth.infer(r["text"], r["text_length"], r["refer"], r["refer_lengths"], batch=True, seed=r["seed"],
                                 sample_ids=r["sample_ids"], max_generate_length=101, suppress_eos=True, return_lengths=True, diffusion_steps=5)
        assert lens == rlens == [100 * 1024] * B
        assert torch.equal(wav, ref), f"request {i}: max-abs {float((wav - ref).abs().max()):.3e}"
    rt.set_option("uncond_cache_mb", 0)
    ref, _ = synth.infer(reqs[0]["text"], reqs[0]["text_length"], reqs[0]["refer"], reqs[0]["refer_lengths"], batch=True, seed=reqs[0]["seed"],
                         sample_ids=reqs[0]["sample_ids"], max_generate_length=101, suppress_eos=True, return_lengths=True, diffusion_steps=5)
    assert torch.equal(outs[0][0], ref)
