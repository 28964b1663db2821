"""MI355X: the diffusion trunk's fp16 mode (option "trunk_fp16", infer(trunk_precision="fp16")) = the reference's
DiffusionTts.enable_fp16 / config use_fp16 (vqvae/diff_model.py:143-157, 299-309): layers[1:] of the trunk run their convs and
attention products as ONE fp16 product with fp32 accumulation instead of three.

Yardstick (tests/golden/trunk_fp16.npz, make_golden_fp16.py): the reference's OWN enable_fp16 run.  On the CPU its autocast selects
bfloat16, whose unit roundoff is 8 x fp16's; E_ref = |reference enable_fp16 - reference fp32| per case.  Gate: the device's fp16-mode
error against the reference's fp32 result <= E_ref / 4, max-abs and relative RMS both (expected near E_ref / 8 or below, since the device
also keeps every stored activation in fp32; the remaining factor 2 is for the fp16 attention products).  Floor: the mode's result
differs from the default mode's and its error exceeds the default mode's error of the same case, so it cannot be a no-op.  Every
figure goes to $DTTS_TEST_LOG (profiles/fp16_measured_errors.txt)."""
import os

import numpy as np
import pytest

from conftest import tol
from fullsize_inputs import N_CODES, T, e2e_inputs, inputs, sub

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GATE_DIV = 4.0


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def relrms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def record(name, value, limit=float("nan")):
    """a measured figure (and the limit it is held to, if any) -> $DTTS_TEST_LOG, before anything is asserted"""
    print(f"[fp16] {name}\t{value:.3e}\t{limit:.3e}")
    log = os.environ.get("DTTS_TEST_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{name}\t{value:.3e}\t{limit:.3e}\n")


def gate(name, e16, e_def, e_ref):
    """e16 / e_def: (max-abs, relative RMS) of the fp16 / default mode against the reference's fp32 result; e_ref: the reference's own"""
    for what, v16, vd, vr in zip(("maxabs", "relrms"), e16, e_def, e_ref):
        record(f"{name}_{what}_fp16_mode", v16, vr / GATE_DIV)
        record(f"{name}_{what}_default_mode", vd)
        record(f"{name}_{what}_E_ref", vr)
    for v16, vd, vr in zip(e16, e_def, e_ref):
        assert v16 <= vr / GATE_DIV, (name, v16, vr / GATE_DIV)
        assert v16 > vd, (name, "the fp16 mode is no further from the reference than the default mode", v16, vd)


class fp16_mode:
    def __init__(self, rt, on=1):
        self.rt, self.on = rt, on

    def __enter__(self):
        self.rt.set_option("trunk_fp16", self.on)

    def __exit__(self, *a):
        self.rt.set_option("trunk_fp16", 0)


@pytest.fixture(scope="module")
def rt(weights):
    from detail_tts_amd.runtime import Runtime
    return Runtime(weights, folded=True, parts=("diffusion",))


@pytest.fixture(scope="module")
def G(golden):
    return golden("trunk_fp16")


@pytest.fixture(scope="module")
def synth():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    return SynthesizerTrn(select_inference_params(synthetic_state_dict(0, variant="signal")), folded=True)


# ---------------------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("cond_free", [False, True])
@pytest.mark.parametrize("which", [0, 1])
def test_forward_T48_fp16_mode_within_reference_gate(rt, G, golden, which, cond_free):
    F = golden("diff_forward")
    t = int(G["fwd48_timesteps"][which])
    nm = "uncond" if cond_free else "cond"
    y32, e_ref = G[f"fwd48_t{t}_{nm}_y32"], (float(G[f"fwd48_t{t}_{nm}_emax"]), float(G[f"fwd48_t{t}_{nm}_erel"]))
    x, ce = dev(F["x"]), dev(F["code_emb"])
    assert rt.get_option("trunk_fp16") == 0
    d = host(rt.diff_forward_t(x, t, None if cond_free else ce, cond_free=cond_free))
    with fp16_mode(rt):
        assert rt.get_option("trunk_fp16") == 1
        h = host(rt.diff_forward_t(x, t, None if cond_free else ce, cond_free=cond_free))
    assert np.isfinite(h).all() and not np.array_equal(h, d)
    gate(f"fwd48_t{t}_{nm}", (maxabs(h, y32), relrms(h, y32)), (maxabs(d, y32), relrms(d, y32)), e_ref)


@pytest.mark.parametrize("cond_free", [False, True])
@pytest.mark.parametrize("step", [47, 0])
def test_forward_T936_fp16_mode_within_reference_gate(rt, G, step, cond_free):
    I = inputs()
    nm = "uncond" if cond_free else "cond"
    k = f"fwd936_s{step}_{nm}"
    ref = np.concatenate([G[k + "_y32_s"].ravel(), G[k + "_y32_t"].ravel()])
    x, ce = dev(I["x"]), dev(I["code_emb"])

    def run():
        o = host(rt.diff_forward(x, step, None if cond_free else ce, cond_free=cond_free))
        s, t = sub(o[0], G)
        return o, np.concatenate([s.ravel(), t.ravel()])

    d_full, d = run()
    with fp16_mode(rt):
        h_full, h = run()
    assert np.isfinite(h_full).all() and not np.array_equal(h_full, d_full)
    gate(k, (maxabs(h, ref), relrms(h, ref)), (maxabs(d, ref), relrms(d, ref)), (float(G[k + "_emax"]), float(G[k + "_erel"])))


# ---------------------------------------------------------------------------------------------------------------- 2. layer scope
def test_layer_zero_and_the_integrator_keep_the_three_product_kernels(rt):
    """With the mode on, layers[0] (ResBlock and AttentionBlock) and the conditioning integrator give the default mode's bits; layers[1],
    a later layer and the trailing ResBlocks do not."""
    rs = np.random.RandomState(5)
    x = dev(rs.randn(2, 768, 200).astype(np.float32))
    lens = [200, 131]
    res = ["diffusion.layers.0.resblk", "diffusion.conditioning_timestep_integrator.1.resblk", "diffusion.layers.1.resblk",
           "diffusion.layers.9.resblk", "diffusion.layers.10", "diffusion.layers.12"]
    att = ["diffusion.layers.0.attn", "diffusion.conditioning_timestep_integrator.2.attn", "diffusion.layers.1.attn", "diffusion.layers.9.attn"]

    def run():
        return [host(rt.op_resblock(p, x, 20, lens)) for p in res], [host(rt.op_attention_block(p, x, lens)) for p in att]

    r0, a0 = run()
    with fp16_mode(rt):
        r1, a1 = run()
    for p, u, v in list(zip(res, r0, r1)) + list(zip(att, a0, a1)):
        covered = not (".layers.0." in p or "integrator" in p)
        assert np.isfinite(v).all()
        assert np.array_equal(u, v) != covered, (p, covered)
        if covered:                                  # a single block under one fp16 product: 2^-11 operands, not garbage
            for b, L in enumerate(lens):
                assert relrms(v[b, :, :L], u[b, :, :L]) < 5e-3, p


# ---------------------------------------------------------------------------------------------------------------- 3. end to end
def _e2e_errors(wav, mel, G, E):
    w = host(wav)[0, 0] if wav.dim() == 3 else host(wav)
    out = {"wav": (maxabs(w, E["wav"]), relrms(w, E["wav"]))}
    if mel is not None:
        s, t = sub(host(mel)[0], E)
        m, m32 = np.concatenate([s.ravel(), t.ravel()]), np.concatenate([E["mel_s"].ravel(), E["mel_t"].ravel()])
        out["mel"] = (maxabs(m, m32), relrms(m, m32))
    return out


def _mel(synth, EI, E, prec):
    """the mel of the request, through the same launches infer() makes (stage B alone)"""
    rt = synth.rt
    refer = dev(EI["refer"])
    lat = rt.gpt_latents(refer, [T], [EI["text"][0]], [EI["codes"][0]])
    code_emb = rt.diff_timestep_independent(lat, rt.diff_conditioning(refer, [T]), [N_CODES])
    from detail_tts_amd.vqvae.model_24k import sampling_args
    sched_ts, sampler_id, eta = sampling_args(None, "p", 0.0)
    sched = rt.sampler_schedule(sched_ts, sampler_id)
    with synth._trunk_precision(prec):
        return rt.diff_sample_ex(code_emb, int(E["seed"]), [int(E["sample_id"])], sched=sched, sampler=sampler_id, eta=eta, lens=[T], denorm=True)


def test_e2e_p50_fp16_mode_within_reference_gate(synth, G, golden):
    """infer(..., trunk_precision="fp16") at the headline size under the "signal" weights, sampler "p", 50 steps: mel and waveform
    against the reference's fp32 infer (e2e_fullsize_signal.npz) within E_ref / 4 of the reference's own enable_fp16 infer."""
    E, EI = golden("e2e_fullsize_signal"), e2e_inputs()
    args = (torch.from_numpy(EI["text"]), torch.tensor([61]), torch.from_numpy(EI["refer"]), torch.tensor([T]))
    kw = dict(seed=int(E["seed"]), sample_ids=[int(E["sample_id"])], forced_codes=[EI["codes"][0]])
    w_def = synth.infer(*args, **kw)
    w_16 = synth.infer(*args, trunk_precision="fp16", **kw)
    assert synth.rt.get_option("trunk_fp16") == 0
    assert bool(torch.isfinite(w_16).all()) and not torch.equal(w_16, w_def)
    e16 = _e2e_errors(w_16, _mel(synth, EI, E, 1), G, E)
    edef = _e2e_errors(w_def, _mel(synth, EI, E, None), G, E)
    for k in ("mel", "wav"):
        gate(f"e2e_p50_{k}", e16[k], edef[k], (float(G[f"e2e_{k}_emax"]), float(G[f"e2e_{k}_erel"])))


def test_dpmsolver_20_steps_runs_in_fp16_mode(synth, golden):
    """the mode reaches the other samplers' schedules: recorded, not gated (no reference fixture exists for this pair)"""
    E, EI = golden("e2e_fullsize_signal"), e2e_inputs()
    args = (torch.from_numpy(EI["text"]), torch.tensor([61]), torch.from_numpy(EI["refer"]), torch.tensor([T]))
    kw = dict(seed=int(E["seed"]), sample_ids=[int(E["sample_id"])], forced_codes=[EI["codes"][0]], sampler="dpmsolver++", diffusion_steps=20)
    w32 = host(synth.infer(*args, trunk_precision="fp32", **kw))[0, 0]
    w16 = host(synth.infer(*args, trunk_precision="fp16", **kw))[0, 0]
    assert np.isfinite(w16).all() and not np.array_equal(w16, w32)
    record("e2e_dpmsolver20_wav_maxabs_fp16_vs_fp32_mode", maxabs(w16, w32))
    record("e2e_dpmsolver20_wav_relrms_fp16_vs_fp32_mode", relrms(w16, w32))
    w16d = host(synth.infer(*args, trunk_precision="fp16", **dict(kw, sampler="ddim", diffusion_steps=25)))[0, 0]
    w32d = host(synth.infer(*args, **dict(kw, sampler="ddim", diffusion_steps=25)))[0, 0]
    assert np.isfinite(w16d).all() and not np.array_equal(w16d, w32d)
    record("e2e_ddim25_wav_relrms_fp16_vs_fp32_mode", relrms(w16d, w32d))


# ---------------------------------------------------------------------------------------------------------------- 4. ragged batch
def test_e2e_fp16_mode_row_of_ragged_B8_within_the_same_gate(synth, G, golden):
    from test_gpu_fullsize import _ragged_batch8
    E, EI = golden("e2e_fullsize_signal"), e2e_inputs()
    refer, rl, text, tl, codes, n = _ragged_batch8(EI)
    kw = dict(batch=True, seed=int(E["seed"]), sample_ids=[100, 101, 102, 103, 104, int(E["sample_id"]), 106, 107], forced_codes=codes,
              return_lengths=True)
    args = (torch.from_numpy(text), torch.tensor(tl), torch.from_numpy(refer), torch.tensor(rl))
    wd, lens = synth.infer(*args, **kw)
    wh, lens_h = synth.infer(*args, trunk_precision="fp16", **kw)
    assert lens == lens_h and bool(torch.isfinite(wh).all())
    e_ref = (float(G["e2e_wav_emax"]), float(G["e2e_wav_erel"]))
    w16, wdef = host(wh)[5, 0, : lens[5]], host(wd)[5, 0, : lens[5]]
    gate("e2e_p50_row5_of_B8_wav", (maxabs(w16, E["wav"]), relrms(w16, E["wav"])), (maxabs(wdef, E["wav"]), relrms(wdef, E["wav"])), e_ref)
    for b in range(8):                               # every row moved, none by more than the gated row's class of error
        a, c = host(wh)[b, 0, : lens[b]], host(wd)[b, 0, : lens[b]]
        assert not np.array_equal(a, c)
        record(f"e2e_p50_B8_row{b}_wav_relrms_fp16_vs_default_mode", relrms(a, c))
        assert relrms(a, c) <= e_ref[1] / GATE_DIV * 2, b      # |fp16 - default| <= |fp16 - ref| + |default - ref|


# ---------------------------------------------------------------------------------------------------------------- 5. option hygiene
def _small_requests():
    rs = np.random.RandomState(19)
    reqs = []
    for i, (B, Tr, Lt) in enumerate([(2, 220, 14), (8, 150, 10), (1, 260, 20)]):
        refer = torch.from_numpy((rs.randn(B, 128, Tr) * 2 - 5).astype(np.float32))
        text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, Lt)), np.zeros((B, 1), np.int64)], 1).astype(np.int32))
        reqs.append(dict(text=text, text_length=torch.full((B,), Lt + 1), refer=refer, refer_lengths=torch.tensor([Tr - 8 * b for b in range(B)]),
                         seed=700 + i, sample_ids=[10 * i + b for b in range(B)]))
    return reqs


def test_a_per_call_fp16_does_not_leak_and_the_pipeline_equals_blocking(synth):
    reqs, G_ = _small_requests(), 24

    def blocking(r, **kw):
        return synth.infer(r["text"], r["text_length"], r["refer"], r["refer_lengths"], batch=True, seed=r["seed"], sample_ids=r["sample_ids"],
                           max_generate_length=G_, suppress_eos=True, return_lengths=True, **kw)

    before, _ = blocking(reqs[0])
    half, _ = blocking(reqs[0], trunk_precision="fp16")
    assert synth.rt.get_option("trunk_fp16") == 0
    after, _ = blocking(reqs[0])
    assert torch.equal(before, after) and not torch.equal(before, half)
    outs = list(synth.infer_stream(iter(reqs), max_generate_length=G_, suppress_eos=True, trunk_precision="fp16"))
    assert synth.rt.get_option("trunk_fp16") == 0 and len(outs) == len(reqs)
    for r, (wav, lens) in zip(reqs, outs):
        ref, rlens = blocking(r, trunk_precision="fp16")
        assert lens == rlens and torch.equal(wav, ref) and bool(torch.isfinite(wav).all())
    again, _ = blocking(reqs[0])
    assert torch.equal(before, again)
    synth.diffusion.enable_fp16 = True                  # the model-level switch, as on the reference's module ...
    try:
        on, _ = blocking(reqs[0])
        off, _ = blocking(reqs[0], trunk_precision="fp32")          # ... and a per-call "fp32" over it, restored afterwards
        assert synth.rt.get_option("trunk_fp16") == 1
    finally:
        synth.diffusion.enable_fp16 = False
    assert torch.equal(on, half) and torch.equal(off, before)


def test_fp16_mode_is_refused_on_the_exact_fp32_kernels(rt):
    rt.set_option("conv_x3", 0)
    try:
        with pytest.raises(Exception, match="trunk_fp16"):
            rt.set_option("trunk_fp16", 1)
        assert rt.get_option("trunk_fp16") == 0
    finally:
        rt.set_option("conv_x3", 1)
    rt.set_option("trunk_fp16", 1)
    try:
        with pytest.raises(Exception, match="trunk_fp16"):
            rt.set_option("conv_x3", 0)
        assert rt.get_option("conv_x3") == 1
    finally:
        rt.set_option("trunk_fp16", 0)


# ---------------------------------------------------------------------------------------------------------------- 6. default path
def test_default_path_unchanged_with_the_option_explicitly_off(rt, golden):
    """test_diffusion_forward_golden's fixture and limit with trunk_fp16 = 0 set explicitly, and the same bits as before the set"""
    g = golden("diff_forward")
    assert int(g["ts"][0]) == 3836
    oc0 = host(rt.diff_forward(dev(g["x"]), 47, dev(g["code_emb"])))
    rt.set_option("trunk_fp16", 0)
    oc = host(rt.diff_forward(dev(g["x"]), 47, dev(g["code_emb"])))
    ou = host(rt.diff_forward(dev(g["x"]), 47, cond_free=True))
    assert np.array_equal(oc, oc0)
    assert maxabs(oc, g["out_cond"]) < 3e-4 and maxabs(ou, g["out_uncond"]) < 3e-4
    tol("fp16_option_off_forward_T48_maxabs", maxabs(oc, g["out_cond"]), 3e-4)
