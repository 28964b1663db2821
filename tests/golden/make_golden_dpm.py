#!/usr/bin/env python3
"""Golden vectors of the DPM-Solver++(2M) sampler FROM THE REFERENCE ITSELF.

Same recipe as make_golden_sampler.py (reference imported under its shim, seed-0 synthetic weights, Philox noise at the reference's
RNG sites).  The path is SpacedDiffusion.k_diffusion_sample_loop (vqvae/utils/diffusion.py:487-581), which runs the bundled DPM_Solver
(vqvae/utils/dpm_solver.py) with algorithm_type="dpmsolver++", order 2, multistep, time_uniform: it draws no noise after x_T.
Stored (data only):

  dpm_tables.npz   for N = 2, 7, 10, 20, 50: the solver's fp32 times t_0..t_N and model times (t * 1000) of the N model evaluations;
                   alpha, sigma, lambda at every time, as NoiseScheduleVP("linear", 0.025, 5.0) computes them (:108-154); and the
                   per-step scalars of the N updates in the solver's order (step k: t_k -> t_{k+1}): sigma_t / sigma_s, alpha_t * phi_1,
                   1 / r0 (0 for a first-order step) and the order (:547-580, 796-831, 1195-1201)
  dpm_chains.npz   at the T = 48 shape of diff_cond.npz, N = 10 and N = 7 (lower_order_final): x_T; x before / after, x0 and x0_prev of
                   the first step, the first second-order step and the last step (keyed by the device's step index i = N - 1 - k); the
                   final sample; DiffusionTts.forward at the fractional model time of N = 10's second evaluation, cond and uncond
  dpm_e2e.npz      the reference's SynthesizerTrn.infer at the headline configuration (234 forced codes, 936-frame prompt) with its
                   OWN infer_diffuser (50 steps, sampler='dpm++2m') driven through sample_loop, seed-0 weights and the "signal" variant:
                   mel subsampled as make_golden_e2e_fullsize.py does, the waveform every 8th sample

    python tests/golden/make_golden_dpm.py      # ~4 min on 8 cores
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
from make_golden import build_reference_model, install_shim, save  # noqa: E402

CH_STRIDE, T_STRIDE, TAIL, WAV_STRIDE = 4, 13, 8, 8
TABLE_N = (2, 7, 10, 20, 50)


def diffuser(n):
    from vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(4000, [n]), model_mean_type="epsilon", model_var_type="learned_range",
                           loss_type="mse", betas=get_named_beta_schedule("linear", 4000), conditioning_free=True,
                           conditioning_free_k=2.0, sampler="dpm++2m")


class _Pbar:
    def update(self, n=1):
        pass


def sub(a):
    a = np.asarray(a.detach().numpy() if hasattr(a, "detach") else a)[0]
    return a[::CH_STRIDE, ::T_STRIDE].copy(), a[:, -TAIL:].copy()


def tables():
    """The solver's own schedule arithmetic, on the 0-d fp32 tensors it uses (DPM_Solver.sample: timesteps[step] is 0-d)."""
    import torch
    from vqvae.utils.dpm_solver import DPM_Solver, NoiseScheduleVP
    ns = NoiseScheduleVP(schedule="linear", continuous_beta_0=0.1 / 4, continuous_beta_1=20.0 / 4)
    solver = DPM_Solver(lambda x, t: x, ns, algorithm_type="dpmsolver++")
    out = {}
    for N in TABLE_N:
        ts = solver.get_time_steps(skip_type="time_uniform", t_T=ns.T, t_0=1.0 / ns.total_N, N=N, device="cpu")
        assert ts.dtype == torch.float32 and ts.shape == (N + 1,)
        tl = [ts[i] for i in range(N + 1)]
        out[f"times_{N}"] = ts
        out[f"model_times_{N}"] = torch.stack([(t.reshape(1) * 1000)[0] for t in tl[:N]])
        out[f"alpha_{N}"] = torch.stack([ns.marginal_alpha(t) for t in tl])
        out[f"sigma_{N}"] = torch.stack([ns.marginal_std(t) for t in tl])
        out[f"lambda_{N}"] = torch.stack([ns.marginal_lambda(t) for t in tl])
        ratio, c1, inv_r0, order = [], [], [], []
        for k in range(N):
            s, t = tl[k], tl[k + 1]
            o = 1 if k == 0 or (N < 10 and k == N - 1) else 2
            lam_s, lam_t = ns.marginal_lambda(s), ns.marginal_lambda(t)
            h = lam_t - lam_s
            ratio.append(ns.marginal_std(t) / ns.marginal_std(s))
            c1.append(torch.exp(ns.marginal_log_mean_coeff(t)) * torch.expm1(-h))
            if o == 2:
                h_0 = lam_s - ns.marginal_lambda(tl[k - 1])
                inv_r0.append(1.0 / (h_0 / h))
            else:
                inv_r0.append(torch.zeros((), dtype=torch.float32))
            order.append(o)
        out[f"ratio_{N}"] = torch.stack(ratio)
        out[f"alpha_phi1_{N}"] = torch.stack(c1)
        out[f"inv_r0_{N}"] = torch.stack(inv_r0)
        out[f"order_{N}"] = np.array(order, np.int32)
    save("dpm_tables", **out)


def chains(m):
    import torch
    from vqvae.utils.dpm_solver import DPM_Solver
    g = dict(np.load(os.path.join(HERE, "diff_cond.npz")))
    code_emb = torch.from_numpy(g["code_emb"])
    T = code_emb.shape[2]
    out = {"code_emb": code_emb, "seed": np.array(MG.SEED_N), "sample_id": np.array(0)}
    orig = DPM_Solver.multistep_dpm_solver_update
    for N in (10, 7):
        keep = {1: N - 1, 2: N - 2, N: 0}          # the reference's step -> the device's step index

        def rec(self, x, model_prev_list, t_prev_list, t, order, *a, _N=N, _keep=keep, **k):
            r = orig(self, x, model_prev_list, t_prev_list, t, order, *a, **k)
            step = len(rec.seen) + 1
            rec.seen.append(order)
            if step in _keep:
                i = _keep[step]
                out[f"n{_N}_x_before_{i}"] = x.clone()
                out[f"n{_N}_x_after_{i}"] = r.clone()
                out[f"n{_N}_x0_{i}"] = model_prev_list[-1].clone()
                if order == 2:
                    out[f"n{_N}_x0_prev_{i}"] = model_prev_list[-2].clone()
                out[f"n{_N}_order_{i}"] = np.array(order, np.int32)
            return r

        rec.seen = []
        DPM_Solver.multistep_dpm_solver_update = rec
        try:
            d = diffuser(N)
            with MG.philox_rng(sample_id=0):
                x_init = torch.randn((1, 128, T))
            final = d.k_diffusion_sample_loop(None, _Pbar(), m.diffusion, (1, 128, T), noise=x_init,
                                              model_kwargs={"precomputed_aligned_embeddings": code_emb})
        finally:
            DPM_Solver.multistep_dpm_solver_update = orig
        assert len(rec.seen) == N, rec.seen
        out[f"n{N}_orders"] = np.array(rec.seen, np.int32)
        out[f"n{N}_x_init"] = x_init
        out[f"n{N}_final"] = final
    rs = np.random.RandomState(4321)
    x = rs.randn(1, 128, T).astype(np.float32)
    tt = torch.linspace(1.0, 0.001, 11)[1:2] * 1000           # N = 10's second model time: fractional
    assert float(tt[0]) != round(float(tt[0]))
    out["fwd_x"], out["fwd_t"] = x, tt
    out["fwd_out_cond"] = m.diffusion(torch.from_numpy(x), tt, precomputed_aligned_embeddings=code_emb)
    out["fwd_out_uncond"] = m.diffusion(torch.from_numpy(x), tt, precomputed_aligned_embeddings=code_emb, conditioning_free=True)
    save("dpm_chains", **out)


def e2e(variant, sample_id):
    import torch
    from fullsize_inputs import N_CODES, T, e2e_inputs
    m = build_reference_model(variant)
    g = m.gpt
    I = e2e_inputs()
    d = m.infer_diffuser                            # the reference's own: 50 steps, sampler='dpm++2m' (vqvae/model_24k.py:581-583)
    assert d.sampler == "dpm++2m" and d.num_timesteps == 50
    d.p_sample_loop = d.sample_loop                 # do_spectrogram_diffusion (vqvae/model_24k.py:479-492) through sample_loop
    out = {"seed_inputs": np.array(I["seed_inputs"]), "seed": np.array(MG.SEED_N), "sample_id": np.array(sample_id),
           "n_steps": np.array(50), "ch_stride": np.array(CH_STRIDE), "t_stride": np.array(T_STRIDE), "tail": np.array(TAIL),
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
    with MG.philox_rng(sample_id=sample_id):
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
    if "--no-e2e" not in sys.argv:
        a, b = e2e(None, 5), e2e("signal", 5)
        save("dpm_e2e", **a, **{"signal_" + k: v for k, v in b.items() if k in ("mel_s", "mel_t", "wav_s", "wav_rms")})


if __name__ == "__main__":
    main()
