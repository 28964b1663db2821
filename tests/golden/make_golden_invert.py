#!/usr/bin/env python3
"""tests/golden/ddim_reverse.npz FROM THE REFERENCE ITSELF: GaussianDiffusion.ddim_reverse_sample
(vqvae/utils/diffusion.py:785-817), p_mean_variance (:284-386) and ddim_sample (:744-783), on the CPU, in eval mode.

Runs only in the build container (needs the reference checkout and transformers), under the shim of make_golden.py with the seed-0
synthetic weights.  Data only.  Its inputs are regenerated from sampler_chains.npz (code_emb, ddim0_final, ddim0_x_init, p_x_before_9 / _0);
nothing already committed is stored again, only checksums of what was read.  The diffuser is make_golden_sampler.diffuser(10, "ddim").

Tensors that a test feeds back, whole [1,128,48]:
  rev_x_before_4 / _9   x at the level of steps 4 and 9 of the reference's free inversion chain from x_start = ddim0_final (step 0 is fed
                        ddim0_final itself)
  split_x5              x at the level of step 5 of the reference's ddim_sample_loop (eta = 0) from ddim0_x_init - its final result is
                        asserted to be sampler_chains' ddim0_final bit for bit
  f64_gap [10]          max-abs of the reference's fp32 `sample` against tests/ddim_ref.py's float64 restatement on the reference's own
                        pred_xstart, per step: no step gate may be tighter
  f64_sum_*             checksums of the inputs read from sampler_chains.npz
Compared outputs, every invert_inputs.CH_STRIDE-th channel (p_mean_variance every PMV_CH_STRIDE-th):
  chain_x [10], chain_x0 [3]   the free chain: x after steps 0 .. 9 (= depth 1 .. 10), pred_xstart of steps 0, 4, 9.  Step t's teacher-forced
                        `sample` is chain_x[t]: the chain IS the reference's step fed its own output
  pmv_<t>_<key>         the p_mean_variance dict at t = 9 and t = 0 on p_x_before_9 / p_x_before_0
  rt_final              the round trip: inversion to depth 5, then ddim_sample (eta = 0) for t = 5 .. 0
  rt_miss               max-abs of rt_final against x_start (the round trip is not the identity)

The script prints and asserts
  (a) the reference's own fp32-against-float64 gap per step (stored as f64_gap);
  (b) the share of clamped pred_xstart elements per step - steps 0 and 4 have >= 10 % on either side of the clamp;
  (c) that each planted mistake (tests/ddim_ref.MISTAKES) moves a stored `sample` by more than 20 x the gate its GPU test uses
      (tests/invert_inputs.py): on the teacher-forced steps 0 and 4 from the recorded model outputs (at step 9, 99 % clamped, only the
      two clamp mistakes are required to show; the rest is printed), and on the free chain by running the reference's model under the
      mistaken update to every compared depth.

    python tests/golden/make_golden_invert.py       # ~1 min on 8 cores
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/ddim_ref.py, tests/invert_inputs.py, tests/diff_loss_inputs.py

import make_golden as MG  # noqa: E402
import make_golden_sampler as MGS  # noqa: E402
import ddim_ref as DR  # noqa: E402
import invert_inputs as II  # noqa: E402
from diff_loss_inputs import checksum  # noqa: E402

INPUT_KEYS = ("code_emb", "ddim0_final", "ddim0_x_init", "p_x_before_9", "p_x_before_0")


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def main():
    MG.install_shim()
    import torch
    torch.set_grad_enabled(False)
    m = MG.build_reference_model()
    assert not m.diffusion.training
    d = MGS.diffuser(II.N_STEPS, "ddim")
    N = d.num_timesteps
    S = dict(np.load(os.path.join(HERE, "sampler_chains.npz")))
    assert np.array_equal(S["code_emb"], np.load(os.path.join(HERE, "diff_cond.npz"))["code_emb"])
    code_emb = torch.from_numpy(S["code_emb"])
    kw = {"precomputed_aligned_embeddings": code_emb}
    tt = lambda i: torch.tensor([i])  # noqa: E731

    # the two model outputs of every step, recorded in call order (cond, then conditioning_free)
    rec = []
    hook = m.diffusion.register_forward_hook(lambda mod, a, k, out: rec.append((bool(k.get("conditioning_free")), out.numpy().copy())),
                                             with_kwargs=True)

    def outputs():
        (f0, c), (f1, u) = rec[-2:]
        assert not f0 and f1
        return c[:, :128], u[:, :128], c, u

    fed = {"f64_sum_" + k: checksum(S[k]) for k in INPUT_KEYS}
    out = {"ch_stride": np.array(II.CH_STRIDE), "pmv_ch_stride": np.array(II.PMV_CH_STRIDE)}

    # ---- the free chain from x_start = ddim0_final, t = 0 .. 9
    x_start = torch.from_numpy(S["ddim0_final"])
    x, chain = x_start, []
    for t in range(N):
        r = d.ddim_reverse_sample(m.diffusion, x, tt(t), model_kwargs=kw)
        c, u, _, _ = outputs()
        chain.append(dict(x=x.numpy().copy(), sample=r["sample"].numpy().copy(), x0=r["pred_xstart"].numpy().copy(), c=c, u=u))
        x = r["sample"]
    gap = np.zeros(N)
    print("(a) reference fp32 against the float64 restatement, (b) clamped share of pred_xstart:")
    for t, s in enumerate(chain):
        gap[t] = maxabs(s["sample"], DR.reverse_update(d, s["x"], s["x0"], t))
        s["clamped"] = float(np.mean(np.abs(s["x0"]) == 1.0))
        full = DR.reverse_step(d, s["x"], s["c"], s["u"], t)
        print(f"  t = {t}: sample gap {gap[t]:.2e} (from the model outputs: sample {maxabs(s['sample'], full[0]):.2e}, pred_xstart "
              f"{maxabs(s['x0'], full[1]):.2e}), clamped {100 * s['clamped']:.0f} %, |sample| max {np.abs(s['sample']).max():.2f}")
    assert gap[0] < 2e-5 and gap[1:].max() < 3e-6, gap
    assert all(0.1 <= chain[t]["clamped"] <= 0.9 for t in (0, 4)), [s["clamped"] for s in chain]
    fed["f64_gap"] = gap
    fed["rev_x_before_4"], fed["rev_x_before_9"] = chain[4]["x"], chain[9]["x"]
    out["chain_x"] = np.stack([II.sub(s["sample"]) for s in chain])
    out["chain_x0"] = np.stack([II.sub(chain[t]["x0"]) for t in II.STEPS])

    # ---- p_mean_variance at t = 9 and t = 0 on the stored p_x_before_*
    for t in II.PMV_STEPS:
        xb = torch.from_numpy(S[f"p_x_before_{t}"])
        r = d.p_mean_variance(m.diffusion, xb, tt(t), model_kwargs=kw)
        _, _, oc, ou = outputs()
        f = DR.mean_variance(d, xb.numpy(), oc, ou, t)
        for k in II.PMV_KEYS:
            out[f"pmv_{t}_{k}"] = II.sub(r[k], II.PMV_CH_STRIDE)
            print(f"  p_mean_variance t = {t} {k:13s}: reference fp32 against float64 {maxabs(r[k].numpy(), f[k]):.2e}")
            assert maxabs(r[k].numpy(), f[k]) < 2e-5, (t, k)

    # ---- the round trip: inversion to depth 5, then ddim_sample (eta = 0) for t = 5 .. 0
    D = II.ROUND_TRIP_DEPTH
    x = torch.from_numpy(chain[D - 1]["sample"])
    for t in range(D, -1, -1):
        x = d.ddim_sample(m.diffusion, x, tt(t), model_kwargs=kw, eta=0.0)["sample"]
    miss = maxabs(x.numpy(), S["ddim0_final"])
    print(f"round trip from depth {D}: misses x_start by {miss:.2f} max-abs")
    assert miss > 0.1
    out["rt_final"], out["rt_miss"] = II.sub(x), np.array(miss)

    # ---- the reference's own ddim_sample_loop (eta = 0) from ddim0_x_init: x at the level of step 5
    x = torch.from_numpy(S["ddim0_x_init"])
    for t in range(N - 1, -1, -1):
        if t == II.SPLIT_LEVEL:
            fed["split_x5"] = x.numpy().copy()
        x = d.ddim_sample(m.diffusion, x, tt(t), model_kwargs=kw, eta=0.0)["sample"]
    assert np.array_equal(x.numpy(), S["ddim0_final"])

    # ---- (c) the mistakes the fixture must see
    print("(c) planted mistakes: change of a stored `sample` over the gate of tests/test_gpu_invert.py")
    for mk in DR.MISTAKES:
        for t in II.STEPS:
            s = chain[t]
            wrong, _ = DR.reverse_step(d, s["x"], s["c"], s["u"], t, mk)
            ratio = maxabs(II.sub(wrong), II.sub(s["sample"])) / II.STEP_SAMPLE_GATE[t]
            required = t != N - 1 or mk in ("no_clamp", "eps_of_model")
            print(f"  {mk:18s} step t = {t}: {ratio:12.1f} x the gate" + ("" if required else "  (not required: nearly all clamped)"))
            assert ratio > 20.0 or not required, (mk, t, ratio)
    hook.remove()
    ts = lambda t: torch.tensor([d.timestep_map[t]])  # noqa: E731
    for mk in (None,) + DR.MISTAKES:
        x = S["ddim0_final"]
        for t in range(max(II.CHAIN_DEPTHS)):
            xt = torch.from_numpy(x)
            c = m.diffusion(xt, ts(t), precomputed_aligned_embeddings=code_emb).numpy()[:, :128]
            u = m.diffusion(xt, ts(t), precomputed_aligned_embeddings=code_emb, conditioning_free=True).numpy()[:, :128]
            x = DR.reverse_step(d, x, c, u, t, mk)[0].astype(np.float32)
            if t + 1 in II.CHAIN_DEPTHS:
                e = maxabs(II.sub(x), out["chain_x"][t])
                if mk is None:
                    print(f"  free chain, depth {t + 1}: the float64 update rounded per step is {e:.2e} off the reference's fp32 chain")
                    assert e <= II.CHAIN_GATE[t + 1], (t + 1, e)          # no chain gate below the reference's own gap
                else:
                    ratio = e / II.CHAIN_GATE[t + 1]
                    print(f"  {mk:18s} chain depth {t + 1}: {ratio:12.1f} x the gate")
                    assert ratio > 20.0, (mk, t + 1, ratio)
    for t in II.STEPS:
        assert II.STEP_SAMPLE_GATE[t] >= gap[t], (t, gap[t])              # no step gate below the reference's own gap

    MG.save("ddim_reverse", **fed, **out)
    size = os.path.getsize(os.path.join(HERE, "ddim_reverse.npz"))
    assert size <= 128 * 1024, size


if __name__ == "__main__":
    main()
