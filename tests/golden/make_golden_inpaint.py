#!/usr/bin/env python3
"""tests/golden/inpaint.npz: the inpainting loop (RePaint) driven by THE REFERENCE'S OWN steps, on the CPU, in eval mode.

The reference has no inpainting loop, but every step such a loop is made of: GaussianDiffusion.ddim_sample (eta = 0,
vqvae/utils/diffusion.py:744-783) and, for the ancestral sampler, p_mean_variance (:284-386) with p_sample's
mean + (i != 0) exp(0.5 log_variance) noise (:445-485).  This script calls those, and between the calls sits the blend of
tests/inpaint_ref.py in NumPy fp32 - q_sample's formula (:243-260) at alphas_cumprod_prev for the kept frames, a select, one forward
step for a repeat.

Runs only in the build container (needs the reference checkout and transformers), under the shim of make_golden.py with the seed-0
synthetic weights.  Data only.  Inputs come from sampler_chains.npz (code_emb, ddim0_x_init as x_T, ddim0_final as `known`) and are
not stored again, only their checksums; the three noise arrays of a chain are rebuilt by inpaint_inputs.noises (exact integers over
256), only their checksums are stored.

Stored per chain c in (ddim1, ddim2, p1, p2) - (sampler, U):
  <c>_x_after_7 / _4 / _0   x after the last repeat of steps 7 and 4 and the final x, every invert_inputs.CH_STRIDE-th channel
  f64_gap_<c>               max-abs over those three of the fp32 chain against the same chain with the blend evaluated in float64 (the
                            reference's steps are fp32 either way): no gate may sit below it
  f64_sum_noise_<c>         checksums of the three noise arrays
The script prints and asserts
  (a) each chain's float64 gap (< 2e-5) and what a 1e-6 perturbation of x_T arrives as at the final x (printed; < 1e-3);
  (b) kept frames of every stored tensor are the blend of known alone - at the final x, known's bits; with nothing kept and U = 1 the
      ddim chain is sampler_chains' ddim0_final bit for bit;
  (c) at least 10 % of the span of every stored tensor is unsaturated (|x| < 1): the final x is pred_xstart, clamped to +-1;
  (d) each planted mistake (inpaint_ref.MISTAKES) moves EVERY stored tensor by more than 20 x the gate of its GPU test
      (inpaint_inputs.CHAIN_GATE; no_blend is measured inside the span); renoise_beta exists only where U = 2.

    python tests/golden/make_golden_inpaint.py       # ~1 min on 8 cores
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/inpaint_ref.py, tests/inpaint_inputs.py, tests/diff_loss_inputs.py

import make_golden as MG  # noqa: E402
import make_golden_sampler as MGS  # noqa: E402
import inpaint_ref as IR  # noqa: E402
import inpaint_inputs as PI  # noqa: E402
from diff_loss_inputs import checksum  # noqa: E402

INPUT_KEYS = ("code_emb", "ddim0_final", "ddim0_x_init")


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def main():
    MG.install_shim()
    import torch
    torch.set_grad_enabled(False)
    m = MG.build_reference_model()
    assert not m.diffusion.training
    d = MGS.diffuser(PI.N_STEPS, "ddim")
    N = d.num_timesteps
    S = dict(np.load(os.path.join(HERE, "sampler_chains.npz")))
    kw = {"precomputed_aligned_embeddings": torch.from_numpy(S["code_emb"])}
    tt = lambda i: torch.tensor([i])  # noqa: E731
    x_T, known, keep = S["ddim0_x_init"], S["ddim0_final"], PI.keep_mask()

    def stepper(sampler, step_noise):
        def step(x, i, e):
            xt = torch.from_numpy(np.ascontiguousarray(x, np.float32))
            if sampler == "ddim":
                return d.ddim_sample(m.diffusion, xt, tt(i), model_kwargs=kw, eta=0.0)["sample"].numpy()
            r = d.p_mean_variance(m.diffusion, xt, tt(i), model_kwargs=kw)
            return (r["mean"] + float(i != 0) * torch.exp(0.5 * r["log_variance"]) * torch.from_numpy(step_noise[e])).numpy()
        return step

    def run(sampler, U, x0=x_T, keep=keep, dtype=np.float32, mistake=None):
        sn, kn, rn = PI.noises(sampler, U)
        got = {}

        def record(e, i, r, u, x):
            if i in PI.STORED_AFTER and r == (0 if i == 0 else U - 1):
                got[i] = np.asarray(x).copy()
        IR.chain(d, stepper(sampler, sn), x0, known, keep, U, kn, rn, dtype=dtype, mistake=mistake, record=record)
        return got

    out = {"ch_stride": np.array(PI.CH_STRIDE)}
    out.update({"f64_sum_" + k: checksum(S[k]) for k in INPUT_KEYS})

    # (b) nothing kept, U = 1: the plain chain
    plain = run("ddim", 1, keep=np.zeros((1, PI.T), bool))
    assert np.array_equal(plain[0], S["ddim0_final"])

    for sampler, U in PI.CHAINS:
        c = PI.name(sampler, U)
        sn, kn, rn = PI.noises(sampler, U)
        out["f64_sum_noise_" + c] = np.stack([checksum(a) for a in (sn, kn, rn)])
        x32 = run(sampler, U)
        x64 = run(sampler, U, dtype=np.float64)
        gap = max(maxabs(x32[i], x64[i]) for i in PI.STORED_AFTER)
        pert = run(sampler, U, x0=(x_T.astype(np.float64) + 1e-6 * np.sign(x_T)).astype(np.float32))
        arrive = maxabs(pert[0], x32[0])
        print(f"{c}: (a) fp32 against the float64 blend {gap:.2e}; a 1e-6 perturbation of x_T arrives as {arrive:.2e}")
        assert gap < 2e-5 and arrive < 1e-3, (c, gap, arrive)
        assert PI.CHAIN_GATE[c] >= gap, (c, gap)                              # no gate below the reference's own gap
        out["f64_gap_" + c] = np.array(gap)
        ev = {i: e for e, i, r, reps in IR.evaluations(N - 1, U) if r == reps - 1}
        for i in PI.STORED_AFTER:
            x = x32[i]
            assert x.dtype == np.float32 and np.isfinite(x).all()
            # (b) kept frames: the blend of known alone
            kept = IR.blend(x, known, keep, IR.coefs(d, i), step0=i == 0, zk=kn[ev[i]])
            assert np.array_equal(kept, x), (c, i)
            if i == 0:
                assert np.array_equal(x[:, :, keep[0]], known[:, :, keep[0]])
            # (c) saturation inside the span
            unsat = float(np.mean(np.abs(x[:, :, PI.SPAN]) < 1.0))
            print(f"    x after step {i}: {100 * unsat:.0f} % of the span unsaturated, differs from the plain chain by "
                  f"{maxabs(x[:, :, PI.SPAN], plain[i][:, :, PI.SPAN]):.2f} there")
            assert unsat >= 0.10, (c, i, unsat)
            out[f"{c}_x_after_{i}"] = PI.sub(x)
        # (d) planted mistakes
        for mk in IR.MISTAKES:
            if mk == "renoise_beta" and U == 1:
                continue
            wrong = run(sampler, U, mistake=mk)
            where = PI.SPAN if mk == "no_blend" else slice(None)
            for i in PI.STORED_AFTER:
                move = maxabs(PI.sub(wrong[i])[:, where], PI.sub(x32[i])[:, where])
                ratio = move / PI.CHAIN_GATE[c]
                print(f"    (d) {mk:13s} x after step {i}: moves {move:.2e} = {ratio:9.1f} x the gate")
                assert ratio > 20.0, (c, mk, i, ratio)

    MG.save("inpaint", **out)
    size = os.path.getsize(os.path.join(HERE, "inpaint.npz"))
    print("inpaint.npz:", size, "bytes")
    assert size <= 128 * 1024, size


if __name__ == "__main__":
    main()
