#!/usr/bin/env python3
"""Golden vectors of the sampler options (any step count, DDIM) FROM THE REFERENCE ITSELF.

Same recipe as make_golden.py (reference imported under its shim, seed-0 synthetic weights, Philox noise at the reference's RNG sites),
with the diffusion step counter of the noise hook starting at N - 1 for an N-step schedule.  Stored (data only):

  sampler_tables.npz   timestep_map and the float64 tables of the reference's SpacedDiffusion for N = 10, 25, 200 and "ddim25"
                       (N = 1: timestep_map only - the reference's constructor cannot build a 1-step schedule)
  sampler_chains.npz   at the T = 48 shape of diff_cond.npz: ddim_sample_loop (N = 10, eta = 0 and 0.5) and p_sample_loop (N = 10);
                       x before / after and pred_xstart of steps 9, 8 and 0, and the final sample; DiffusionTts.forward at the
                       off-schedule timestep t = 1234, cond and uncond
  sampler_e2e.npz      the reference's SynthesizerTrn.infer at the headline configuration (234 forced codes, 936-frame prompt)
                       with a 20-step diffuser driven through ddim_sample_loop (eta = 0), seed-0 weights and the "signal" variant:
                       mel subsampled as make_golden_e2e_fullsize.py does, the waveform every 8th sample

    python tests/golden/make_golden_sampler.py      # ~2 min on 8 cores
"""
import contextlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
from make_golden import build_reference_model, install_shim, save  # noqa: E402

TABLES = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "alphas_cumprod_next", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
          "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
          "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")
CH_STRIDE, T_STRIDE, TAIL, WAV_STRIDE = 4, 13, 8, 8


def diffuser(n, sampler="p"):
    from vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(4000, n if isinstance(n, str) else [n]), model_mean_type="epsilon",
                           model_var_type="learned_range", loss_type="mse", betas=get_named_beta_schedule("linear", 4000),
                           conditioning_free=True, conditioning_free_k=2.0, sampler=sampler)


@contextlib.contextmanager
def philox_rng_n(n_steps, sample_id=0):
    """make_golden.philox_rng with the step counter of the initial-noise hook at n_steps - 1 instead of 49"""
    import torch
    with MG.philox_rng(sample_id=sample_id) as st:
        inner = torch.randn

        def randn(*a, **k):
            z = inner(*a, **k)
            st["diff_step"] = n_steps - 1
            return z

        torch.randn = randn
        try:
            yield st
        finally:
            torch.randn = inner


def sub(a):
    a = np.asarray(a.detach().numpy() if hasattr(a, "detach") else a)[0]
    return a[::CH_STRIDE, ::T_STRIDE].copy(), a[:, -TAIL:].copy()


def tables():
    from vqvae.utils.diffusion import space_timesteps
    out = {"tmap_1": np.array(sorted(space_timesteps(4000, [1])))}
    for key, n in (("10", 10), ("25", 25), ("200", 200), ("ddim25", "ddim25")):
        d = diffuser(n)
        out[f"tmap_{key}"] = np.array(d.timestep_map)
        for t in TABLES:
            out[f"f64_{key}_{t}"] = np.asarray(getattr(d, t), np.float64)
    save("sampler_tables", **out)


def chains(m):
    import torch
    g = dict(np.load(os.path.join(HERE, "diff_cond.npz")))
    code_emb = torch.from_numpy(g["code_emb"])
    T = code_emb.shape[2]
    N, KEEP = 10, (9, 8, 0)
    out = {"code_emb": code_emb, "seed": np.array(MG.SEED_N), "sample_id": np.array(0), "n_steps": np.array(N)}
    for name, sampler, eta in (("ddim0", "ddim", 0.0), ("ddim05", "ddim", 0.5), ("p", "p", 0.0)):
        d = diffuser(N, sampler)
        step_fn = "ddim_sample" if sampler == "ddim" else "p_sample"
        orig = getattr(d, step_fn)

        def rec(model, x, t, *a, _orig=orig, _name=name, **k):
            r = _orig(model, x, t, *a, **k)
            i = int(t[0])
            if i in KEEP:
                out[f"{_name}_x_before_{i}"] = x.clone()
                out[f"{_name}_x_after_{i}"] = r["sample"]
                out[f"{_name}_x0_{i}"] = r["pred_xstart"]
            return r

        setattr(d, step_fn, rec)
        with philox_rng_n(N, sample_id=0):
            x_init = torch.randn((1, 128, T))
            kw = dict(noise=x_init, model_kwargs={"precomputed_aligned_embeddings": code_emb}, progress=False)
            if sampler == "ddim":
                final = d.ddim_sample_loop(m.diffusion, (1, 128, T), eta=eta, **kw)
            else:
                final = d.p_sample_loop(m.diffusion, (1, 128, T), **kw)
        out[f"{name}_x_init"] = x_init
        out[f"{name}_final"] = final
        out[f"{name}_eta"] = np.array(eta, np.float32)
    rs = np.random.RandomState(1234)
    x = rs.randn(1, 128, T).astype(np.float32)
    ts = torch.tensor([1234])
    out["fwd_x"], out["fwd_t"] = x, ts
    out["fwd_out_cond"] = m.diffusion(torch.from_numpy(x), ts, precomputed_aligned_embeddings=code_emb)
    out["fwd_out_uncond"] = m.diffusion(torch.from_numpy(x), ts, precomputed_aligned_embeddings=code_emb, conditioning_free=True)
    save("sampler_chains", **out)


def e2e(variant, sample_id):
    import torch
    from fullsize_inputs import N_CODES, T, e2e_inputs
    m = build_reference_model(variant)
    g = m.gpt
    I = e2e_inputs()
    N = 20
    d = diffuser(N, "ddim")
    d.p_sample_loop = d.ddim_sample_loop             # do_spectrogram_diffusion (vqvae/model_24k.py:479-492) through DDIM, eta = 0
    m.infer_diffuser = d
    out = {"seed_inputs": np.array(I["seed_inputs"]), "seed": np.array(MG.SEED_N), "sample_id": np.array(sample_id),
           "n_steps": np.array(N), "ch_stride": np.array(CH_STRIDE), "t_stride": np.array(T_STRIDE), "tail": np.array(TAIL),
           "wav_stride": np.array(WAV_STRIDE)}
    o_fv = m.infer_flowvae

    def infer_flowvae(mel, yl, *a, **k):
        assert mel.shape == (1, 128, T), mel.shape
        out["mel_s"], out["mel_t"] = sub(mel)
        return o_fv(mel, yl, *a, **k)

    m.infer_flowvae = infer_flowvae
    codes_t = torch.from_numpy(I["codes"])
    g.inference_speech_tortoise = lambda *a, **k: torch.cat([codes_t, torch.tensor([[g.stop_mel_token]])], 1)
    t0 = time.time()
    with philox_rng_n(N, sample_id=sample_id):
        wav = m.infer(torch.from_numpy(I["text"]), torch.tensor([I["text"].shape[1]]), torch.from_numpy(I["refer"]),
                      torch.tensor([I["refer"].shape[2]]))
    w = wav.numpy()[0, 0]
    assert w.shape == (1024 * N_CODES,)
    out["wav_s"] = w[::WAV_STRIDE].astype(np.float32)
    out["wav_rms"] = np.array(float(np.sqrt(np.mean(w.astype(np.float64) ** 2))))
    print(f"e2e {variant}: {time.time() - t0:.0f} s, wav rms {float(out['wav_rms']):.3e}", flush=True)
    return out


def main():
    install_shim()
    import torch
    torch.set_grad_enabled(False)
    tables()
    chains(build_reference_model())
    a, b = e2e(None, 5), e2e("signal", 5)
    save("sampler_e2e", **a, **{"signal_" + k: v for k, v in b.items() if k in ("mel_s", "mel_t", "wav_s", "wav_rms")})


if __name__ == "__main__":
    main()
