"""GPU: the DPM-Solver++(2M) sampler (dtts_diff_schedule_dpm / dtts_diff_sample_ex sampler 2 / dtts_diff_step_dpm / dtts_diff_forward_tf)
against the reference's own k_diffusion_sample_loop runs (dpm_chains.npz, dpm_e2e.npz: tests/golden/make_golden_dpm.py)."""
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
def D(golden):
    return golden("dpm_chains")


def _diffuser(n, sampler="dpmsolver++"):
    from detail_tts_amd.vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    return SpacedDiffusion(space_timesteps(4000, [n]), betas=get_named_beta_schedule("linear", 4000), conditioning_free=True,
                           conditioning_free_k=2.0, sampler=sampler)


def test_forward_at_a_fractional_time_golden(synth, D):
    """DiffusionTts.forward at the fractional model time of N = 10's second step vs the reference model, cond and uncond; an integer
    time through the fractional entry is the integer entry bit for bit."""
    x, ce = dev(D["fwd_x"]), dev(D["code_emb"])
    ts = torch.from_numpy(D["fwd_t"])
    assert ts.dtype == torch.float32 and float(ts[0]) != round(float(ts[0]))
    oc = host(synth.diffusion(x, ts, precomputed_aligned_embeddings=ce))
    ou = host(synth.diffusion(x, ts, precomputed_aligned_embeddings=ce, conditioning_free=True))
    ec, eu = maxabs(oc, D["fwd_out_cond"]), maxabs(ou, D["fwd_out_uncond"])
    print(f"\n[fractional forward t = {float(ts[0])}] cond {ec:.2e}, uncond {eu:.2e}")
    assert ec < 3e-4 and eu < 3e-4, (ec, eu)                            # the diff_forward.npz gate
    rt = synth.rt
    a = host(rt.diff_forward_tf(x, 1234.0, ce))
    assert np.array_equal(a, host(rt.diff_forward_t(x, 1234, ce)))
    t47 = rt.timestep_map[47]
    assert np.array_equal(host(rt.diff_forward_tf(x, float(t47), ce)), host(rt.diff_forward(x, 47, ce)))
    assert np.array_equal(host(synth.diffusion(x, torch.tensor([float(t47)]), precomputed_aligned_embeddings=ce)),
                          host(rt.diff_forward(x, 47, ce)))
    with pytest.raises(ValueError):
        synth.diffusion(x, torch.tensor([4000.5]), precomputed_aligned_embeddings=ce)


@pytest.mark.parametrize("x3", [1, 0])
@pytest.mark.parametrize("n", [10, 7])
def test_dpm_steps_teacher_forced_golden(synth, D, n, x3):
    """Single steps of the reference's N-step chains with x and x0_prev TEACHER-FORCED from the fixture: the first (first-order) step,
    the first second-order step and the last step (second order at N = 10, first order at N = 7: lower_order_final); both kernel sets."""
    rt = synth.rt
    sched = rt.diff_schedule_dpm(n)
    ce = dev(D["code_emb"])
    rt.set_option("conv_x3", x3)
    try:
        for i in (n - 1, n - 2, 0):
            order = int(D[f"n{n}_order_{i}"])
            assert order == (1 if i == n - 1 or (n < 10 and i == 0) else 2)
            xb = dev(D[f"n{n}_x_before_{i}"])
            hist = dev(D[f"n{n}_x0_prev_{i}"]) if order == 2 else torch.full_like(xb, float("nan"))   # a first-order step never reads it
            x1, h1, x0 = rt.diff_step_dpm(xb, hist, ce, i, sched, return_x0=True)
            assert torch.equal(h1, x0)
            e0, e1 = maxabs(host(x0), D[f"n{n}_x0_{i}"]), maxabs(host(x1), D[f"n{n}_x_after_{i}"])
            print(f"\n[dpm N={n} step {i} (order {order}), conv_x3={x3}] x0 {e0:.2e}, x {e1:.2e}")
            # ~20 x the measured <= 1.9e-5 (x0) / 6.7e-6 (x) (profiles/dpm_measured_errors.txt)
            tol(f"dpm{n}_step{i}_x0_x3={x3}_maxabs", e0, 4e-4)
            tol(f"dpm{n}_step{i}_x_x3={x3}_maxabs", e1, 1.5e-4)
    finally:
        rt.set_option("conv_x3", 1)


@pytest.mark.parametrize("x3", [1, 0])
def test_dpm_chains_golden(synth, D, x3):
    """The whole N = 10 chain through SpacedDiffusion.sample_loop (device Philox x_T) and the N = 7 chain (lower_order_final) through
    k_diffusion_sample_loop from the reference's x_T, against the reference's final samples."""
    ce = dev(D["code_emb"])
    kw = dict(model_kwargs={"precomputed_aligned_embeddings": ce})
    synth.rt.set_option("conv_x3", x3)
    try:
        m10 = host(_diffuser(10).sample_loop(synth.diffusion, tuple(ce.shape[:1]) + (128, ce.shape[2]), seed=int(D["seed"]),
                                             sample_ids=[int(D["sample_id"])], **kw))
        x_T = dev(D["n7_x_init"])
        m7 = host(_diffuser(7).k_diffusion_sample_loop(None, None, synth.diffusion, tuple(x_T.shape), noise=x_T, **kw))
    finally:
        synth.rt.set_option("conv_x3", 1)
    for n, m in ((10, m10), (7, m7)):
        e = maxabs(m, D[f"n{n}_final"])
        print(f"\n[dpm N={n} chain, conv_x3={x3}] max-abs {e:.2e}, rms {rms(m, D[f'n{n}_final']):.2e}")
        tol(f"dpm{n}_chain_x3={x3}_maxabs", e, 3e-4)                   # ~20 x the measured 6.7e-6 - 1.3e-5


@pytest.fixture(scope="module")
def E(golden):
    return golden("dpm_e2e")


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
def test_e2e_234_codes_dpmsolver50_vs_reference(synth, E, x3):
    """infer(forced codes, sampler="dpmsolver++") at the headline configuration vs the reference's SynthesizerTrn.infer with its OWN
    infer_diffuser (50 steps, sampler='dpm++2m') driven through sample_loop: mel and waveform (seed-0 weights)."""
    assert int(E["n_steps"]) == 50
    got, undo = _mel_trap(synth)
    synth.rt.set_option("conv_x3", x3)
    try:
        wav = _infer_headline(synth, E, sampler="dpmsolver++")
    finally:
        synth.rt.set_option("conv_x3", 1)
        undo()
    s, t = sub(got["mel"][0], E)
    em = max(maxabs(s, E["mel_s"]), maxabs(t, E["mel_t"]))
    w = host(wav)[0, 0][:: int(E["wav_stride"])]
    r = rms(w, E["wav_s"])
    print(f"\n[e2e dpmsolver++ 50, conv_x3={x3}] mel max-abs {em:.2e}, waveform rms {r:.2e} (reference rms {float(E['wav_rms']):.2e})")
    # ~20 x the measured 1.3e-4 (mel) and 6.6e-9 (waveform)
    tol(f"dpm50_mel_maxabs_x3={x3}", em, 3e-3)
    tol(f"dpm50_wav_rms_x3={x3}", r, 1.4e-7)


def test_e2e_234_codes_dpmsolver50_signal_weights_vs_reference():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    from conftest import load_golden
    E = load_golden("dpm_e2e")
    synth = SynthesizerTrn(select_inference_params(synthetic_state_dict(0, variant="signal")), folded=True)
    wav = _infer_headline(synth, E, sampler="dpmsolver++")
    w = host(wav)[0, 0][:: int(E["wav_stride"])]
    r = rms(w, E["signal_wav_s"]) / float(E["signal_wav_rms"])
    print(f"\n[e2e dpmsolver++ 50, signal weights] relative waveform rms {r:.2e}")
    tol("dpm50_signal_wav_rel_rms", r, REL_WAV)


def test_ragged_batch8_dpm_rows_equal_alone(synth):
    """dpmsolver++ on a ragged batch of 8: each row as it is alone, up to the summation order of the batch-8 launches, on the
    de-normalised mel"""
    rt = synth.rt
    rs = np.random.RandomState(45)
    lens = [96, 40, 77, 96, 13, 64, 50, 88]
    B, Tm = len(lens), max(lens)
    ce = rs.randn(B, 768, Tm).astype(np.float32) * 0.5
    sched = rt.diff_schedule_dpm(7)
    sids = [30 + b for b in range(B)]
    xb = host(rt.diff_sample_ex(dev(ce), 78, sids, sched=sched, sampler=2, lens=lens))
    for b, L in enumerate(lens):
        xs = host(rt.diff_sample_ex(dev(ce[b:b + 1, :, :L]), 78, [sids[b]], sched=sched, sampler=2))
        assert np.isfinite(xs).all()
        tol(f"dpm_ragged_row{b}_vs_alone_maxabs", maxabs(xb[b, :, :L], xs[0]), 1.2e-3)   # ~20 x the measured 3.4 - 5.3e-5
    # the padded columns stay untouched
    assert np.all(xb[4, :, 13:] == 0)
    from detail_tts_amd.runtime import DttsError
    with pytest.raises(DttsError):
        rt.diff_sample_ex(dev(ce), 78, sids, sched=sched, sampler=2, eta=0.5, lens=lens)
    with pytest.raises(DttsError):
        rt.diff_sample_ex(dev(ce), 78, sids, sched=sched, sampler=1, lens=lens)       # a DPM schedule runs sampler 2 only


def _requests(n):
    rs = np.random.RandomState(12)
    reqs = []
    for i, (B, Tr, Lt) in enumerate([(2, 200, 12), (3, 160, 9), (1, 220, 14), (2, 120, 8)][:n]):
        refer = torch.from_numpy((rs.randn(B, 128, Tr) * 2 - 5).astype(np.float32))
        text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, Lt)), np.zeros((B, 1), np.int64)], 1).astype(np.int32))
        reqs.append(dict(text=text, text_length=torch.full((B,), Lt + 1), refer=refer, refer_lengths=torch.tensor([Tr - 8 * b for b in range(B)]),
                         seed=500 + i, sample_ids=[10 * i + b for b in range(B)]))
    return reqs


def test_infer_stream_dpmsolver_equals_infer(synth):
    reqs = _requests(4)
    G = 16
    outs = list(synth.infer_stream(iter(reqs), max_generate_length=G, suppress_eos=True, sampler="dpmsolver++", diffusion_steps=20))
    assert len(outs) == 4
    for r, (wav, lens) in zip(reqs, outs):
        ref, rlens = synth.infer(r["text"], r["text_length"], r["refer"], r["refer_lengths"], batch=True, seed=r["seed"],
                                 sample_ids=r["sample_ids"], max_generate_length=G, suppress_eos=True, return_lengths=True,
                                 sampler="dpmsolver++", diffusion_steps=20)
        assert lens == rlens
        assert wav.shape == ref.shape and torch.equal(wav, ref)
        assert bool(torch.isfinite(wav).all()) and float(wav.pow(2).mean().sqrt()) > 1e-5


def test_schedule_cache_dpm_and_integer_schedules_stay_apart(synth):
    """(p, 50) -> (dpmsolver++, 20) -> (p, 50): first and third bit-identical; interleaved DPM and integer schedules that overflow the
    cache (evictions) leave both kinds correct."""
    r = _requests(1)[0]
    kw = dict(batch=True, seed=r["seed"], sample_ids=r["sample_ids"], max_generate_length=16, suppress_eos=True)
    args = (r["text"], r["text_length"], r["refer"], r["refer_lengths"])
    a = synth.infer(*args, **kw)
    b = synth.infer(*args, diffusion_steps=20, sampler="dpmsolver++", **kw)
    c = synth.infer(*args, diffusion_steps=50, sampler="p", **kw)
    d = synth.infer(*args, diffusion_steps=20, sampler="ddim", **kw)
    assert torch.equal(a, c) and not torch.equal(a, b) and not torch.equal(b, d)
    for n in (3, 4, 5, 6, 7, 8):                                         # 12 schedules, 6 of each kind, the same step counts: evictions
        for s in ("dpmsolver++", "ddim"):
            synth.infer(*args, diffusion_steps=n, sampler=s, **dict(kw, max_generate_length=4))
    assert torch.equal(synth.infer(*args, **kw), a)
    assert torch.equal(synth.infer(*args, diffusion_steps=20, sampler="dpmsolver++", **kw), b)
    assert torch.equal(synth.infer(*args, diffusion_steps=20, sampler="ddim", **kw), d)
    rt = synth.rt
    assert rt.diff_schedule_dpm(20) != rt.diff_schedule(_diffuser(20).timestep_map)
