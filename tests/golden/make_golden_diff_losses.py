#!/usr/bin/env python3
"""tests/golden/diff_losses.npz FROM THE REFERENCE ITSELF: GaussianDiffusion.training_losses (vqvae/utils/diffusion.py:930-1012) and
SynthesizerTrn.forward_diff / forward_vq (vqvae/model_24k.py:654-696), on the CPU, in eval mode.

Runs only in the build container (needs the reference checkout and transformers), under the shim of make_golden.py with the seed-0
synthetic weights.  Data only.  The inputs are drawn by tests/diff_loss_inputs.py from fixed seeds (stored in full they would not fit
the 128 KiB this file may take next to the reference's model output); the fixture stores their checksums.

Case A (keys a_*): m.diffuser.training_losses at B = 3, T = 36, t = (0, 1, 199), given noise, aligned_conditioning +
conditioning_latent in model_kwargs.  Stored: a_t, a_mse / a_vb / a_loss fp32 [3], a_model_output fp32 [3, 256, 36] (what the
reference's DiffusionTts returned: the loss kernel is tested on it without the trunk), a_pred_stride and a_pred = x_start_predicted
[:, ::4, ::3], a_branch_counts = entries of the t = 0 row below -0.999 / above 0.999.
Case B (keys b_*): m.forward_diff on two rows (64-frame prompt, full-width texts, raw_mel of 36 frames).  m.diffuser.training_losses
is wrapped: the t the reference drew is recorded (b_t); the noise it draws comes from torch.randn_like, which is patched to hand out
diff_loss_inputs.case_b_noise() and counted (exactly one call).  Stored: b_t, b_loss (the returned scalar), b_row_loss fp32 [2],
b_codes (the reference's encode of raw_mel, int32 [2, 9]).
Case C (keys c_*): m.forward_vq on two rows of 36 frames, y_lengths = (36, 28).  Stored: c_loss.
Tables of m.diffuser (float64): f64_sqrt_alphas_cumprod, f64_sqrt_one_minus_alphas_cumprod, f64_log_betas, timestep_map.

The script asserts that the fixture can see the mistakes this feature can make; each must move the stored per-row value by more than
20 x the gate the GPU test uses (diff_loss_inputs.GATES, the numbers tests/test_gpu_diff_losses.py asserts), and the margins are printed:
  - exchanging two rows' t (each of the three pairs), and using t + 1 (mod 200): through the reference's whole training_losses (the
    trunk evaluated at the wrong timestep, q_sample with the wrong coefficients): mse, vb and loss of EVERY row whose t changed
  - dropping the t == 0 branch (the t = 0 row), and taking log_variance at frac = 0 (the t = 0 and t = 1 rows; at t = 199 the two ends
    of the learned range coincide to 1e-11, so no fixture could show it there): through tests/diff_loss_ref.py on the stored output

    python tests/golden/make_golden_diff_losses.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/diff_loss_ref.py, tests/diff_loss_inputs.py

import make_golden as MG  # noqa: E402
import diff_loss_inputs as DI  # noqa: E402
import diff_loss_ref as DR  # noqa: E402

GATES = DI.GATES            # the gates of tests/test_gpu_diff_losses.py for the end-to-end losses against the reference
PRED_STRIDE = (4, 3)


def run_a(m, torch, a, t):
    grabbed = {}
    hook = m.diffusion.register_forward_hook(lambda mod, inp, out: grabbed.__setitem__("out", out.detach().clone()))
    try:
        terms = m.diffuser.training_losses(m.diffusion, torch.from_numpy(a["x_start"]), torch.from_numpy(np.asarray(t, np.int64)),
                                           model_kwargs={"aligned_conditioning": torch.from_numpy(a["aligned"]),
                                                         "conditioning_latent": torch.from_numpy(a["cond"])},
                                           noise=torch.from_numpy(a["noise"]))
    finally:
        hook.remove()
    return {k: terms[k].numpy().astype(np.float64) for k in ("mse", "vb", "loss")}, terms["x_start_predicted"].numpy(), grabbed["out"].numpy()


def main():
    MG.install_shim()
    import torch
    torch.set_grad_enabled(False)
    m = MG.build_reference_model()
    assert not m.training and not m.diffusion.training
    d = m.diffuser
    assert d.num_timesteps == 200 and not d.conditioning_free
    out = dict(timestep_map=np.array(d.timestep_map, np.int32), f64_sqrt_alphas_cumprod=d.sqrt_alphas_cumprod,
               f64_sqrt_one_minus_alphas_cumprod=d.sqrt_one_minus_alphas_cumprod, f64_log_betas=np.log(d.betas))

    # ---- case A
    a = DI.case_a(dict(np.load(os.path.join(HERE, "diff_cond.npz"))))
    t = a["t"]
    terms, pred, mo = run_a(m, torch, a, t)
    assert mo.shape == (DI.B_A, 256, DI.T_A)
    lo, hi = int((a["x_start"][0] < -0.999).sum()), int((a["x_start"][0] > 0.999).sum())
    assert lo >= 8 and hi >= 8 and lo + hi < 128 * DI.T_A // 100, (lo, hi)
    out.update(a_t=t.astype(np.int32), a_mse=terms["mse"], a_vb=terms["vb"], a_loss=terms["loss"], a_model_output=mo.astype(np.float32),
               a_pred_stride=np.array(PRED_STRIDE, np.int32), a_pred=pred[:, ::PRED_STRIDE[0], ::PRED_STRIDE[1]],
               a_branch_counts=np.array([lo, hi], np.int32))
    for k in ("x_start", "noise", "aligned", "cond"):
        out["f64_sum_a_" + k] = DI.checksum(a[k])
    # the float64 restatement on the stored output is the reference's arithmetic
    x_t = DR.q_sample(d, a["x_start"], t, a["noise"])
    ref = DR.loss_terms(d, mo, a["x_start"], x_t, a["noise"], t)
    for k in ("mse", "vb", "loss"):
        gap = np.abs(ref[k] - terms[k]).max()
        print(f"  case A {k}: reference {terms[k]}, float64 restatement off by {gap:.3e}")
        assert gap < 1e-6, (k, gap)             # two fp32 ulps of the largest value (7.1): the reference's result is fp32
    # ---- the mistakes the fixture must see
    print("sensitivity margins (per-row change / gate):")
    for name, t2 in (("rows 0 <-> 1", t[[1, 0, 2]]), ("rows 1 <-> 2", t[[0, 2, 1]]), ("rows 0 <-> 2", t[[2, 1, 0]]), ("t + 1", (t + 1) % 200)):
        wrong, _, _ = run_a(m, torch, a, t2)
        moved = np.nonzero(t2 != t)[0]
        for k in ("mse", "vb", "loss"):
            ratio = np.abs(wrong[k] - terms[k])[moved] / GATES[k]
            print(f"  {name:16s} {k:5s} rows {moved.tolist()}: {np.array2string(ratio, precision=1)}")
            # (under the seed-0 weights the predicted eps is near zero at every t, so mse = mean (noise - eps)^2 sees the timestep least:
            # 1.5e-4 .. 3e-3; vb and the loss move by 1.5 .. 6)
            assert ratio.min() > 20, (name, k, ratio)
    for name, kw, rows in (("no t == 0 branch", dict(drop_t0=True), [0]), ("frac = 0", dict(frac_zero=True), [0, 1])):
        wrong = DR.loss_terms(d, mo, a["x_start"], x_t, a["noise"], t, **kw)
        for k in ("vb", "loss"):
            ratio = np.abs(wrong[k] - ref[k]) / GATES[k]
            print(f"  {name:16s} {k:5s} rows {rows}: {np.array2string(ratio[rows], precision=1)}   (all rows: {np.array2string(ratio, precision=1)})")
            # frac = 0 cannot show in the t = 199 row: there the two ends of the learned range coincide to 1e-11 (posterior variance ->
            # beta); the t = 0 and t = 1 rows see it
            assert ratio[rows].min() > 20, (name, k, ratio)

    # ---- case B
    b = DI.case_b(dict(np.load(os.path.join(HERE, "gpt_forced.npz"))))
    seen = {"randn_like": 0}
    o_tl, o_rl, o_enc = d.training_losses, torch.randn_like, m.encode

    def training_losses(model, x_start, t, model_kwargs=None, noise=None):
        assert noise is None
        seen["t"] = t.numpy().copy()
        terms = o_tl(model=model, x_start=x_start, t=t, model_kwargs=model_kwargs)
        seen["row_loss"] = terms["loss"].numpy().copy()
        return terms

    def randn_like(x, **kw):
        seen["randn_like"] += 1
        z = DI.case_b_noise()
        assert tuple(x.shape) == z.shape
        return torch.from_numpy(z)

    def encode(*a_, **k_):
        r = o_enc(*a_, **k_)
        seen["codes"] = r[0].numpy().copy()
        return r

    d.training_losses, torch.randn_like, m.encode = training_losses, randn_like, encode
    try:
        torch.manual_seed(7)
        data = dict(raw_mel=torch.from_numpy(b["raw_mel"]), raw_spec_length=torch.from_numpy(b["raw_spec_length"]),
                    text=torch.from_numpy(b["text"]), text_length=torch.from_numpy(b["text_length"]),
                    raw_wav_length=torch.from_numpy(b["raw_wav_length"]))
        lb = m.forward_diff(torch.from_numpy(b["y"]), torch.from_numpy(b["y_lengths"]), data)
    finally:
        d.training_losses, torch.randn_like, m.encode = o_tl, o_rl, o_enc
    assert seen["randn_like"] == 1 and seen["t"].shape == (2,) and seen["codes"].shape == (2, 9)
    assert abs(float(lb) - seen["row_loss"].astype(np.float64).mean()) < 1e-6
    out.update(b_t=seen["t"].astype(np.int32), b_loss=np.array(float(lb), np.float32), b_row_loss=seen["row_loss"].astype(np.float32),
               b_codes=seen["codes"].astype(np.int32), f64_sum_b_noise=DI.checksum(DI.case_b_noise()))
    for k in ("y", "raw_mel", "text"):
        out["f64_sum_b_" + k] = DI.checksum(b[k])
    print(f"  case B: t {seen['t'].tolist()}, rows {seen['row_loss']}, forward_diff {float(lb):.6f}")

    # ---- case C
    c = DI.case_c()
    lc = m.forward_vq(torch.from_numpy(c["y"]), torch.from_numpy(c["y_lengths"]), None)
    out.update(c_loss=np.array(float(lc), np.float32), f64_sum_c_y=DI.checksum(c["y"]))
    print(f"  case C: forward_vq {float(lc):.6f}")

    MG.save("diff_losses", **out)
    size = os.path.getsize(os.path.join(HERE, "diff_losses.npz"))
    assert size <= 128 * 1024, size


if __name__ == "__main__":
    main()
