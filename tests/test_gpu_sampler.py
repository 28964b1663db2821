"""GPU: any diffusion step count and the DDIM sampler (dtts_diff_schedule / dtts_diff_sample_ex / dtts_diff_step / dtts_diff_forward_t)
against the reference's own runs (sampler_chains.npz, sampler_e2e.npz: tests/golden/make_golden_sampler.py)."""
import numpy as np
import pytest

from conftest import tol
from fullsize_inputs import T, e2e_inputs, sub

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REL_WAV = 6e-5          # relative waveform RMS gate under the signal weights (test_gpu_signal.py)


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def rms(a, b=0.0):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def synth(weights):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(weights, folded=True)


@pytest.fixture(scope="module")
def S(golden):
    return golden("sampler_chains")


def _diffuser(n, sampler="p"):
    from detail_tts_amd.vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    return SpacedDiffusion(space_timesteps(4000, [n]), betas=get_named_beta_schedule("linear", 4000), conditioning_free=True,
                           conditioning_free_k=2.0, sampler=sampler)


def test_forward_at_an_off_schedule_timestep_golden(synth, S):
    """DiffusionTts.forward at t = 1234 (not one of the 50 default timesteps) vs the reference model, cond and uncond."""
    x, ce = dev(S["fwd_x"]), dev(S["code_emb"])
    ts = torch.from_numpy(S["fwd_t"])
    assert int(ts[0]) == 1234 and 1234 not in synth.rt.timestep_map
    oc = host(synth.diffusion(x, ts, precomputed_aligned_embeddings=ce))
    ou = host(synth.diffusion(x, ts, precomputed_aligned_embeddings=ce, conditioning_free=True))
    assert maxabs(oc, S["fwd_out_cond"]) < 3e-4, maxabs(oc, S["fwd_out_cond"])      # the diff_forward.npz gate
    assert maxabs(ou, S["fwd_out_uncond"]) < 3e-4, maxabs(ou, S["fwd_out_uncond"])
    # a default-schedule timestep through the same entry equals the step-indexed forward bit for bit
    t47 = synth.rt.timestep_map[47]
    a = host(synth.diffusion(x, torch.tensor([t47]), precomputed_aligned_embeddings=ce))
    assert np.array_equal(a, host(synth.rt.diff_forward(x, 47, ce)))
    with pytest.raises(ValueError):
        synth.diffusion(x, torch.tensor([4000]), precomputed_aligned_embeddings=ce)


def test_do_spectrogram_diffusion_honours_a_10_step_p_diffuser(synth, S, golden):
    """do_spectrogram_diffusion(model, diffuser, ...) runs THE DIFFUSER'S schedule: 10 ancestral steps vs the reference's
    p_sample_loop of a 10-step SpacedDiffusion (Philox noise on the device)."""
    from detail_tts_amd.vqvae.model_24k import do_spectrogram_diffusion
    g = golden("diff_cond")
    mel = do_spectrogram_diffusion(synth.diffusion, _diffuser(10, "p"), dev(g["latent"]), dev(g["cond_latent"]), seed=int(S["seed"]),
                                   sample_ids=[int(S["sample_id"])])
    e = maxabs(host(mel), S["p_final"])
    print(f"\n[10-step p chain via do_spectrogram_diffusion] max-abs {e:.2e}, rms {rms(host(mel), S['p_final']):.2e}")
    tol("sampler_p10_chain_maxabs", e, 3e-4)                        # ~20 x the measured 1.4e-5


@pytest.mark.parametrize("x3", [1, 0])
@pytest.mark.parametrize("name", ["ddim0", "ddim05", "p"])
def test_sampler_steps_teacher_forced_golden(synth, S, name, x3):
    """Single steps of the reference's 10-step chains with x TEACHER-FORCED from the fixture (steps 9, 8 with device Philox noise when
    eta > 0, and the last step 0), then the whole chain from the reference's x_T; both kernel sets."""
    rt = synth.rt
    sampler = 0 if name == "p" else 1
    eta = float(S[f"{name}_eta"])
    sched = rt.diff_schedule(_diffuser(10).timestep_map)
    assert sched != 0
    ce = dev(S["code_emb"])
    seed, sid = int(S["seed"]), [int(S["sample_id"])]
    rt.set_option("conv_x3", x3)
    try:
        for i in (9, 8, 0):
            x1, x0 = rt.diff_step(dev(S[f"{name}_x_before_{i}"]), ce, i, seed, sid, sched=sched, sampler=sampler, eta=eta, return_x0=True)
            e0, e1 = maxabs(host(x0), S[f"{name}_x0_{i}"]), maxabs(host(x1), S[f"{name}_x_after_{i}"])
            assert e0 < 5e-3 and e1 < (2e-4 if i == 0 else 2e-3), (i, e0, e1)    # test_sampler_steps_teacher_forced_golden's gates
        x = rt.diff_sample_ex(ce, seed, sid, sched=sched, sampler=sampler, eta=eta, denorm=False)
    finally:
        rt.set_option("conv_x3", 1)
    e = maxabs(host(x), S[f"{name}_final"])
    print(f"\n[10-step {name} chain, conv_x3={x3}] max-abs {e:.2e}")
    # ~20 x the measured 7.7e-5 / 2.3e-5 / 1.4e-5 (ddim eta 0 / 0.5 / p; profiles/sampler_measured_errors.txt)
    tol(f"sampler_{name}_chain_x3={x3}_maxabs", e, {"ddim0": 2e-3, "ddim05": 5e-4, "p": 3e-4}[name])


@pytest.fixture(scope="module")
def E(golden):
    return golden("sampler_e2e")


def _infer_headline(synth, E, **kw):
    EI = e2e_inputs()
    return synth.infer(torch.from_numpy(EI["text"]), torch.tensor([61]), torch.from_numpy(EI["refer"]), torch.tensor([T]),
                       seed=int(E["seed"]), sample_ids=[int(E["sample_id"])], forced_codes=[EI["codes"][0]], **kw)


def _mel_trap(synth):
    """record the de-normalised mel that infer() hands to stage C"""
    got = {}
    orig = synth.rt.vocoder

    def voc(mel, *a, **k):
        got["mel"] = host(mel)
        return orig(mel, *a, **k)

    synth.rt.vocoder = voc
    return got, lambda: setattr(synth.rt, "vocoder", orig)


@pytest.mark.parametrize("x3", [1, 0])
def test_e2e_234_codes_ddim20_vs_reference(synth, E, x3):
    """infer(forced codes, diffusion_steps=20, sampler="ddim") at the headline configuration vs the reference's SynthesizerTrn.infer with
    a 20-step diffuser driven through ddim_sample_loop: mel and waveform (seed-0 weights)."""
    got, undo = _mel_trap(synth)
    synth.rt.set_option("conv_x3", x3)
    try:
        wav = _infer_headline(synth, E, diffusion_steps=20, sampler="ddim")
    finally:
        synth.rt.set_option("conv_x3", 1)
        undo()
    s, t = sub(got["mel"][0], E)
    em = max(maxabs(s, E["mel_s"]), maxabs(t, E["mel_t"]))
    w = host(wav)[0, 0][:: int(E["wav_stride"])]
    r = rms(w, E["wav_s"])
    print(f"\n[e2e ddim20, conv_x3={x3}] mel max-abs {em:.2e}, waveform rms {r:.2e} (reference rms {float(E['wav_rms']):.2e})")
    # ~20 x the measured 5.3e-4 (mel; DDIM at eta = 0 carries x0's error through sqrt(1/abar - 1) at every step) and 5.9e-9 (waveform)
    tol(f"ddim20_mel_maxabs_x3={x3}", em, 1e-2)
    tol(f"ddim20_wav_rms_x3={x3}", r, 1.2e-7)


def test_e2e_234_codes_ddim20_signal_weights_vs_reference():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    from conftest import load_golden
    E = load_golden("sampler_e2e")
    synth = SynthesizerTrn(select_inference_params(synthetic_state_dict(0, variant="signal")), folded=True)
    wav = _infer_headline(synth, E, diffusion_steps=20, sampler="ddim")
    w = host(wav)[0, 0][:: int(E["wav_stride"])]
    r = rms(w, E["signal_wav_s"]) / float(E["signal_wav_rms"])
    print(f"\n[e2e ddim20, signal weights] relative waveform rms {r:.2e}")
    tol("ddim20_signal_wav_rel_rms", r, REL_WAV)


def test_ragged_batch8_ddim_eta_rows_equal_alone(synth):
    """ddim with eta = 0.5 (per-row Philox noise at every step) on a ragged batch of 8: each row as it is alone - the same noise, so
    up to the summation order of the batch-8 launches (two CFG stream chunks, other tiles) on the de-normalised mel."""
    rt = synth.rt
    rs = np.random.RandomState(44)
    lens = [96, 40, 77, 96, 13, 64, 50, 88]
    B, Tm = len(lens), max(lens)
    ce = rs.randn(B, 768, Tm).astype(np.float32) * 0.5
    sched = rt.diff_schedule(_diffuser(7).timestep_map)
    sids = [20 + b for b in range(B)]
    xb = host(rt.diff_sample_ex(dev(ce), 77, sids, sched=sched, sampler=1, eta=0.5, lens=lens))
    for b, L in enumerate(lens):
        xs = host(rt.diff_sample_ex(dev(ce[b:b + 1, :, :L]), 77, [sids[b]], sched=sched, sampler=1, eta=0.5))
        assert np.isfinite(xs).all()
        tol(f"ddim_ragged_row{b}_vs_alone_maxabs", maxabs(xb[b, :, :L], xs[0]), 1.2e-2)   # ~20 x the measured 0.8 - 5.8e-4 (7 steps, x 7.1 de-normalised)
    # eta > 0 draws noise: the result differs from eta = 0
    x0 = host(rt.diff_sample_ex(dev(ce), 77, sids, sched=sched, sampler=1, eta=0.0, lens=lens))
    assert maxabs(x0[0, :, :lens[0]], xb[0, :, :lens[0]]) > 1e-3


def _requests(n):
    rs = np.random.RandomState(12)
    reqs = []
    for i, (B, Tr, Lt) in enumerate([(2, 200, 12), (3, 160, 9), (1, 220, 14), (2, 120, 8)][:n]):
        refer = torch.from_numpy((rs.randn(B, 128, Tr) * 2 - 5).astype(np.float32))
        text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, Lt)), np.zeros((B, 1), np.int64)], 1).astype(np.int32))
        reqs.append(dict(text=text, text_length=torch.full((B,), Lt + 1), refer=refer, refer_lengths=torch.tensor([Tr - 8 * b for b in range(B)]),
                         seed=500 + i, sample_ids=[10 * i + b for b in range(B)]))
    return reqs


def test_infer_stream_ddim25_equals_infer(synth):
    reqs = _requests(4)
    G = 16
    outs = list(synth.infer_stream(iter(reqs), max_generate_length=G, suppress_eos=True, sampler="ddim", diffusion_steps=25))
    assert len(outs) == 4
    for r, (wav, lens) in zip(reqs, outs):
        ref, rlens = synth.infer(r["text"], r["text_length"], r["refer"], r["refer_lengths"], batch=True, seed=r["seed"],
                                 sample_ids=r["sample_ids"], max_generate_length=G, suppress_eos=True, return_lengths=True,
                                 sampler="ddim", diffusion_steps=25)
        assert lens == rlens
        assert wav.shape == ref.shape and torch.equal(wav, ref)
        assert bool(torch.isfinite(wav).all()) and float(wav.pow(2).mean().sqrt()) > 1e-5


def test_schedule_cache_leaks_no_state_and_default_is_unchanged(synth):
    """(p, 50) -> (ddim, 20) -> (p, 50): first and third bit-identical; no new arguments == (50, "p") bit for bit; more schedules
    than the cache holds (evictions) leave the default untouched."""
    r = _requests(1)[0]
    kw = dict(batch=True, seed=r["seed"], sample_ids=r["sample_ids"], max_generate_length=16, suppress_eos=True)
    args = (r["text"], r["text_length"], r["refer"], r["refer_lengths"])
    a = synth.infer(*args, **kw)
    b = synth.infer(*args, diffusion_steps=20, sampler="ddim", **kw)
    c = synth.infer(*args, diffusion_steps=50, sampler="p", **kw)
    assert torch.equal(a, c) and not torch.equal(a, b)
    for n in (3, 4, 5, 6, 7, 8, 9, 11, 12, 20):                       # 10 schedules: the cache evicts
        synth.infer(*args, diffusion_steps=n, sampler="ddim", **dict(kw, max_generate_length=4))
    assert torch.equal(synth.infer(*args, **kw), a)
    assert torch.equal(synth.infer(*args, diffusion_steps=20, sampler="ddim", **kw), b)
    tm, coefs = synth.rt.diff_schedule_coefs(synth.rt.diff_schedule(_diffuser(20).timestep_map))
    d = _diffuser(20)
    assert tm.tolist() == d.timestep_map
    np.testing.assert_allclose(coefs[:, 0], d.sqrt_recip_alphas_cumprod.astype(np.float32), rtol=0, atol=0)
    np.testing.assert_allclose(coefs[:, 7], d.alphas_cumprod.astype(np.float32), rtol=0, atol=0)
    np.testing.assert_allclose(coefs[:, 8], d.alphas_cumprod_prev.astype(np.float32), rtol=0, atol=0)
