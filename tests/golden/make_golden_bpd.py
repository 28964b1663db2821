#!/usr/bin/env python3
"""tests/golden/diff_bpd.npz FROM THE REFERENCE ITSELF: GaussianDiffusion.calc_bpd_loop with _vb_terms_bpd and _prior_bpd beneath it
(vqvae/utils/diffusion.py:903-928, 1098-1169), on the CPU, in eval mode.

Runs only in the build container (needs the reference checkout and transformers), under the shim of make_golden.py with the seed-0
synthetic weights.  Data only.  The inputs are drawn by tests/bpd_inputs.py from fixed seeds; the fixture stores their checksums.

Loops (keys <loop>_vb / _xstart_mse / _mse fp32 [2, S], <loop>_prior_bpd / _total_bpd fp32 [2]): calc_bpd_loop at B = 2, T = 36 on rows
0 - 1 of diff_loss_inputs.case_a, aligned_conditioning + conditioning_latent in model_kwargs.  torch.randn_like is patched to hand out
bpd_inputs.loop_noise(loop)[t] at timestep t and is counted (S calls).
  s5:   SpacedDiffusion(space_timesteps(4000, [5]), conditioning_free=False), the cheap loop
  s200: m.diffuser itself (200 of the 4000 trained steps)
  tr:   SpacedDiffusion(set(range(0, 1000, 5))): a TRUNCATED schedule whose last alphas_cumprod (f64_tr_last_alphas_cumprod) is far from 0,
        so its prior_bpd is O(1); on the other two the prior cancels to ~1e-5 bits
Terms (keys a_vb / a_xstart_mse / a_mse fp32 [3]): the reference's _vb_terms_bpd, mean_flat and _predict_eps_from_xstart at
t = (0, 1, 199) on case A of diff_losses.npz with its STORED model output standing in for the model: what tests/bpd_ref.py must
reproduce without a trunk.

The script prints how far the reference's fp32 results lie from the float64 restatement tests/bpd_ref.py (on the model outputs recorded
during each loop): no gate of tests/test_gpu_bpd.py may be tighter than that gap.  It asserts that the fixture can see the mistakes this
feature can make - each must move a stored value by more than 20 x the gate the GPU test uses (bpd_inputs.LOOP_GATE, relative to
max(1, |value|)) - and prints the margins:
  - noise indexed in draw order instead of by timestep (noise[S - 1 - t] at t): the reference's loop on the flipped noise, s5
  - t off by one ((t + 1) mod S in q_sample, the trunk and the terms): the reference's pieces called by hand, s5 (the same hand-written
    loop without the shift is asserted to equal calc_bpd_loop bit for bit)
  - an unclamped pred_xstart; mse taken from the model's eps instead of eps'; the t == 0 branch dropped: tests/bpd_ref.py's switches on
    the recorded outputs, s5 and s200
  - columns stacked in ascending t: the stored arrays reversed, s5 and s200
  - the prior left out of total_bpd: shows ONLY on the truncated schedule (tr), where the prior is O(1); on s5 and s200 it is ~1e-5 bits,
    below the gate, and no fixture on a full schedule could show it

    python tests/golden/make_golden_bpd.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/bpd_ref.py, tests/bpd_inputs.py, tests/diff_loss_inputs.py

import make_golden as MG  # noqa: E402
import bpd_inputs as BI  # noqa: E402
import bpd_ref as BR  # noqa: E402
import diff_loss_inputs as DI  # noqa: E402

OUT_KEYS = BI.KEYS + ("prior_bpd", "total_bpd")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def run_loop(m, torch, d, inp, noise):
    """the reference's calc_bpd_loop with noise[t] handed out at timestep t -> (its dict as float64 arrays, model outputs by timestep)"""
    S = d.num_timesteps
    seen = {"calls": 0}
    outs = {}
    o_rl = torch.randn_like

    def randn_like(x, **kw):
        t = S - 1 - seen["calls"]
        seen["calls"] += 1
        assert tuple(x.shape) == noise[t].shape
        return torch.from_numpy(noise[t])

    hook = m.diffusion.register_forward_hook(lambda mod, a, out: outs.__setitem__(S - seen["calls"], out.detach().numpy().copy()))
    torch.randn_like = randn_like
    try:
        r = d.calc_bpd_loop(m.diffusion, torch.from_numpy(inp["x_start"]), clip_denoised=True,
                            model_kwargs={"aligned_conditioning": torch.from_numpy(inp["aligned"]),
                                          "conditioning_latent": torch.from_numpy(inp["cond"])})
    finally:
        torch.randn_like = o_rl
        hook.remove()
    assert seen["calls"] == S and sorted(outs) == list(range(S)), (seen, len(outs))
    return {k: r[k].numpy().astype(np.float64) for k in OUT_KEYS}, outs


def hand_loop(m, torch, d, inp, noise, shift):
    """calc_bpd_loop's body from the reference's own pieces, with every timestep moved to (t + shift) mod S"""
    S = d.num_timesteps
    x0 = torch.from_numpy(inp["x_start"])
    kw = {"aligned_conditioning": torch.from_numpy(inp["aligned"]), "conditioning_latent": torch.from_numpy(inp["cond"])}
    cols = {k: [] for k in BI.KEYS}
    for t in range(S - 1, -1, -1):
        tb = torch.tensor([(t + shift) % S] * x0.shape[0])
        z = torch.from_numpy(noise[t])
        x_t = d.q_sample(x_start=x0, t=tb, noise=z)
        out = d._vb_terms_bpd(m.diffusion, x_start=x0, x_t=x_t, t=tb, clip_denoised=True, model_kwargs=kw)
        cols["vb"].append(out["output"])
        cols["xstart_mse"].append(((out["pred_xstart"] - x0) ** 2).mean(dim=(1, 2)))
        cols["mse"].append(((d._predict_eps_from_xstart(x_t, tb, out["pred_xstart"]) - z) ** 2).mean(dim=(1, 2)))
    return {k: torch.stack(v, dim=1).numpy().astype(np.float64) for k, v in cols.items()}


def margins(name, wrong, right, keys, min_ratio=20.0):
    for k in keys:
        ratio = float(rel(wrong[k], right[k]).max() / BI.LOOP_GATE[k])
        print(f"  {name:34s} {k:10s} moves by {ratio:10.1f} x the gate")
        assert ratio > min_ratio, (name, k, ratio)


def main():
    MG.install_shim()
    import torch
    torch.set_grad_enabled(False)
    from vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    m = MG.build_reference_model()
    assert not m.training and not m.diffusion.training
    assert m.diffuser.num_timesteps == 200 and not m.diffuser.conditioning_free

    def diffuser(loop):
        use = BI.use_timesteps(loop, space_timesteps)
        if loop == "s200":
            assert set(m.diffuser.use_timesteps) == set(use)
            return m.diffuser
        return SpacedDiffusion(use_timesteps=use, model_mean_type="epsilon", model_var_type="learned_range", loss_type="mse",
                               betas=get_named_beta_schedule("linear", 4000), conditioning_free=False)

    diff_cond = dict(np.load(os.path.join(HERE, "diff_cond.npz")))
    inp = BI.loop_inputs(diff_cond)
    out = {"f64_sum_" + k: DI.checksum(v) for k, v in inp.items()}
    res, outs, ds, noises = {}, {}, {}, {}
    for loop in BI.LOOPS:
        d = ds[loop] = diffuser(loop)
        S = d.num_timesteps
        noises[loop] = BI.loop_noise(loop, S)
        res[loop], outs[loop] = run_loop(m, torch, d, inp, noises[loop])
        r = res[loop]
        out["f64_sum_noise_" + loop] = DI.checksum(noises[loop])
        out[loop + "_timestep_map"] = np.array(d.timestep_map, np.int32)
        for k in OUT_KEYS:
            out[f"{loop}_{k}"] = r[k].astype(np.float32)
        print(f"{loop}: S = {S}, total_bpd {r['total_bpd']}, prior_bpd {r['prior_bpd']}, vb {r['vb'][0, 0]:.3e} (t = {S - 1}) .. "
              f"{r['vb'][0, -2]:.3e} (t = 1) .. {r['vb'][0, -1]:.3e} (t = 0), mse {r['mse'].min():.3e} .. {r['mse'].max():.3e}, "
              f"xstart_mse {r['xstart_mse'].min():.3e} .. {r['xstart_mse'].max():.3e}")
        # the float64 restatement on the recorded outputs: the gap no gate may go below
        f64 = BR.loop(d, outs[loop], inp["x_start"], noises[loop])
        for k in OUT_KEYS:
            small = np.abs(r[k]) < 1e-3
            print(f"  {loop} {k:10s}: reference fp32 vs float64 restatement: rel-to-max(1,|v|) {rel(r[k], f64[k]).max():.3e}"
                  + (f", abs over the {int(small.sum())} values below 1e-3: {np.abs(r[k] - f64[k])[small].max():.3e}" if small.any() else ""))
            assert rel(r[k], f64[k]).max() < 2e-6, (loop, k)
    out["f64_tr_last_alphas_cumprod"] = np.array(ds["tr"].alphas_cumprod[-1], np.float64)
    assert 0.3 < ds["tr"].alphas_cumprod[-1] < 0.9 and res["tr"]["prior_bpd"].min() > 0.05
    assert res["s200"]["prior_bpd"].max() < 1e-4

    # ---- the per-row terms on case A's stored model output (diff_losses.npz), through the reference's own functions
    g = dict(np.load(os.path.join(HERE, "diff_losses.npz")))
    a = DI.case_a(diff_cond)
    d = m.diffuser
    x0, t, z = torch.from_numpy(a["x_start"]), torch.from_numpy(a["t"]), torch.from_numpy(a["noise"])
    x_t = d.q_sample(x_start=x0, t=t, noise=z)
    o = d._vb_terms_bpd(lambda x, ts, **kw: torch.from_numpy(g["a_model_output"]), x_start=x0, x_t=x_t, t=t, clip_denoised=True, model_kwargs={})
    a_ref = dict(vb=o["output"].numpy(), xstart_mse=((o["pred_xstart"] - x0) ** 2).mean(dim=(1, 2)).numpy(),
                 mse=((d._predict_eps_from_xstart(x_t, t, o["pred_xstart"]) - z) ** 2).mean(dim=(1, 2)).numpy())
    assert np.abs(a_ref["vb"] - g["a_vb"]).max() < 1e-6                      # the same term training_losses returned
    a64 = BR.terms(d, g["a_model_output"], a["x_start"], x_t.numpy(), a["noise"], a["t"])
    for k in BI.KEYS:
        out["a_" + k] = a_ref[k].astype(np.float32)
        print(f"  case A {k:10s}: reference {a_ref[k]}, float64 restatement off by {rel(a_ref[k], a64[k]).max():.3e}")
        assert rel(a_ref[k], a64[k]).max() < 2e-6, k

    # ---- the mistakes the fixture must see
    print("sensitivity margins (change of a stored value relative to max(1, |value|), over the gate of tests/test_gpu_bpd.py):")
    d5, n5 = ds["s5"], noises["s5"]
    flipped, _ = run_loop(m, torch, d5, inp, np.ascontiguousarray(n5[::-1]))
    margins("noise in draw order (s5)", flipped, res["s5"], BI.KEYS + ("total_bpd",))
    same = hand_loop(m, torch, d5, inp, n5, 0)
    assert all(np.array_equal(same[k].astype(np.float32), res["s5"][k].astype(np.float32)) for k in BI.KEYS)
    margins("t off by one (s5)", hand_loop(m, torch, d5, inp, n5, 1), res["s5"], BI.KEYS)
    for loop in ("s5", "s200"):
        f64 = BR.loop(ds[loop], outs[loop], inp["x_start"], noises[loop])
        wrong = BR.loop(ds[loop], outs[loop], inp["x_start"], noises[loop], unclamped=True)
        margins(f"unclamped pred_xstart ({loop})", wrong, f64, ("xstart_mse", "mse"))
        wrong = BR.loop(ds[loop], outs[loop], inp["x_start"], noises[loop], mse_of_model_eps=True)
        margins(f"mse of the model's eps ({loop})", wrong, f64, ("mse",))
        wrong = BR.loop(ds[loop], outs[loop], inp["x_start"], noises[loop], drop_t0=True)
        margins(f"no t == 0 branch ({loop})", wrong, f64, ("vb", "total_bpd"))
        margins(f"columns in ascending t ({loop})", {k: res[loop][k][:, ::-1] for k in BI.KEYS}, res[loop], BI.KEYS)
    no_prior = {"total_bpd": res["tr"]["total_bpd"] - res["tr"]["prior_bpd"]}
    margins("prior left out of total_bpd (tr)", no_prior, res["tr"], ("total_bpd",))
    for loop in ("s5", "s200"):
        ratio = float(rel(res[loop]["total_bpd"] - res[loop]["prior_bpd"], res[loop]["total_bpd"]).max() / BI.LOOP_GATE["total_bpd"])
        print(f"  prior left out of total_bpd ({loop}): {ratio:.2e} x the gate - invisible on a full schedule, as stated above")

    MG.save("diff_bpd", **out)
    size = os.path.getsize(os.path.join(HERE, "diff_bpd.npz"))
    assert size <= 128 * 1024, size


if __name__ == "__main__":
    main()
