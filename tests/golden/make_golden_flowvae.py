#!/usr/bin/env python3
"""tests/golden/flowvae.npz FROM THE REFERENCE ITSELF: SynthesizerTrn.forward_flowvae (vqvae/model_24k.py:706-737) and kl_loss
(vqvae/modules/losses.py:43-58), on the CPU, in eval mode.

Runs only in the build container (needs the reference checkout and transformers), under the shim of make_golden.py with the seed-0
synthetic weights; enc_q gets synthetic_state_dict(0, only_prefixes=["enc_q."], posterior=True).  Data only.  The inputs are drawn
by tests/flowvae_inputs.py from fixed seeds; the fixture stores their checksums.

Case A: m.forward_flowvae at B = 2, T = 48, y_lengths = (48, 44).  torch.randn_like is patched to hand out flowvae_inputs' noise
(exactly one call, of shape [2, 192, 48]) and torch.rand to hand out the fractions that give ids_slice = (8, 0).  Stored: ids_slice,
y_mask, kl = kl_loss(z_p, logs_q, m_p, logs_p, y_mask), kl_q = kl_loss(z_p, logs_q, m_q, logs_q / 2, y_mask) (the same function on
tensors the host restatement can rebuild: enc_p's are not restated), g = ref_enc's output in full, strided samples (s_*) and float64
(sum, sum of squares) (f64_mom_*) of the six latents, quantized and o.
Case B: m.flow on flowvae_inputs.flow_case(), a latent with non-zero tails, with case A's g and mask: samples and moments
(s_flow, f64_mom_flow).

The script asserts that the fixture can see the mistakes this feature can make; each must move a stored sample by more than 20 x the
gate the GPU test uses (flowvae_inputs.GATES), and the margins are printed.  Through tests/flowvae_ref.py (float64, first checked
against the reference's own numbers here): only the first 4 WaveNet layers of enc_q; the cond offset of layer l taken modulo 4; the
last Flip dropped; x1 * mask omitted (case B: enc_q's z has zero tails already, so case A cannot show it); noise_scale 0.667 on the
posterior; the KL divided by C * sum(len).  Through the reference's own dec: the slice taken at ids + 1.

    python tests/golden/make_golden_flowvae.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/flowvae_inputs.py, tests/flowvae_ref.py

import make_golden as MG  # noqa: E402
import flowvae_inputs as FI  # noqa: E402
import flowvae_ref as FR  # noqa: E402

GATES = FI.GATES


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def main():
    MG.install_shim()
    import torch
    torch.set_grad_enabled(False)
    import vqvae.modules.commons as commons
    import vqvae.modules.losses as losses
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    m = MG.build_reference_model()
    sd = synthetic_state_dict(MG.SEED_W, only_prefixes=["enc_q."], posterior=True)
    m.enc_q.load_state_dict({k[len("enc_q."):]: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not m.training and not m.enc_q.training and m.segment_size == FI.SEG
    P = select_inference_params(synthetic_state_dict(MG.SEED_W, posterior=True))

    c = FI.case()
    y, yl, spec = torch.from_numpy(c["y"]), torch.from_numpy(c["y_lengths"]), torch.from_numpy(c["spec"])
    seen = {"randn_like": 0, "rand": 0}
    o_randn_like, o_rand = torch.randn_like, torch.rand

    def randn_like(x, **kw):
        seen["randn_like"] += 1
        assert tuple(x.shape) == (FI.B, FI.INTER, FI.T), tuple(x.shape)
        return torch.from_numpy(c["noise"])

    def rand(*shape, **kw):
        seen["rand"] += 1
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else tuple(shape)
        assert shape == (FI.B,), shape
        return torch.tensor(FI.RAND_FRACTIONS, dtype=torch.float32)

    torch.randn_like, torch.rand = randn_like, rand
    try:
        o, l_diff, loss_gpt, vq_loss, ids, y_mask, lat, quantized = m.forward_flowvae(y, yl, {"spec": spec})
    finally:
        torch.randn_like, torch.rand = o_randn_like, o_rand
    assert seen == {"randn_like": 1, "rand": 1}, seen
    assert (l_diff, loss_gpt, vq_loss) == (0, 0, 0)
    assert ids.tolist() == list(FI.IDS_SLICE) and ids.dtype == torch.int64, ids
    assert tuple(o.shape) == (FI.B, 1, FI.SEG * 256) and tuple(y_mask.shape) == (FI.B, 1, FI.T)
    z, z_p, m_p, logs_p, m_q, logs_q = lat
    kl = losses.kl_loss(z_p, logs_q, m_p, logs_p, y_mask)
    kl_q = losses.kl_loss(z_p, logs_q, m_q, 0.5 * logs_q, y_mask)
    g = m.ref_enc(y * y_mask, y_mask)
    zf = FI.flow_case()
    zpf = m.flow(torch.from_numpy(zf), y_mask, g=g)
    for name, a in zip(FI.LATENTS, lat):            # the reference multiplies all six by the mask
        assert float(a[1, :, FI.LENGTHS[1]:].abs().max()) == 0.0, name
    assert float(zpf[1, :, FI.LENGTHS[1]:].abs().max()) == 0.0
    # quantized = out_proj's output, which the reference does NOT mask: beyond the length it holds the bias
    assert maxabs(quantized[1, :, FI.LENGTHS[1]:].numpy(), np.broadcast_to(P["enc_p.out_proj.bias"][:, None], (FI.INTER, FI.T - FI.LENGTHS[1]))) < 1e-6

    tensors = dict(zip(FI.LATENTS, (a.numpy() for a in lat)), quantized=quantized.numpy(), o=o.numpy(), flow=zpf.numpy())
    out = dict(ids_slice=ids.numpy(), y_mask=y_mask.numpy(), kl=np.array(float(kl), np.float32), kl_q=np.array(float(kl_q), np.float32),
               g=g.numpy().reshape(FI.B, -1), latent_stride=np.array(FI.LATENT_STRIDE, np.int32), wav_stride=np.array(FI.WAV_STRIDE, np.int32))
    for k, a in tensors.items():
        out["s_" + k] = FI.sample(a)
        out["f64_mom_" + k] = FI.moments(a)
    for k in ("y", "spec", "noise"):
        out["f64_sum_" + k] = FI.checksum(c[k])
    out["f64_sum_flow_in"] = FI.checksum(zf)
    print(f"  ids_slice {ids.tolist()}, kl {float(kl):.6f}, kl_q {float(kl_q):.6f}, |o| max {float(o.abs().max()):.4f}")

    # ---- the float64 restatement is the reference's arithmetic (its own fp32 rounding apart)
    gq = out["g"]
    rz, rm, rl = FR.posterior_encoder(P, c["spec"], FI.LENGTHS, gq, c["noise"])
    rzp = FR.flow_forward(P, rz, FI.LENGTHS, gq)
    rflow = FR.flow_forward(P, zf, FI.LENGTHS, gq)
    rkl = FR.kl_loss(z_p.numpy(), logs_q.numpy(), m_p.numpy(), logs_p.numpy(), FI.LENGTHS)
    for name, r, t in (("z", rz, z), ("m_q", rm, m_q), ("logs_q", rl, logs_q), ("z_p", rzp, z_p), ("flow", rflow, zpf)):
        e = maxabs(r, t.numpy())
        print(f"  float64 restatement {name}: off the reference's fp32 by {e:.3e}")
        assert e < 2e-5, (name, e)
    print(f"  float64 restatement kl: {rkl:.6f} against {float(kl):.6f}")
    assert abs(rkl - float(kl)) < 1e-6 * max(1.0, abs(rkl))

    # ---- the mistakes the fixture must see: |stored sample - the value with the mistake| / gate
    print("sensitivity margins (change of a stored value / gate):")

    def margin(name, key, wrong, right):
        ratio = maxabs(FI.sample(wrong), FI.sample(right)) / GATES[key]
        print(f"  {name:34s} {key:7s}: {ratio:.1f}")
        assert ratio > 20, (name, key, ratio)

    for name, kw in (("first 4 WaveNet layers only", dict(layers_run=4)), ("cond offset of layer l modulo 4", dict(cond_mod=4))):
        wz, wm, wl = FR.posterior_encoder(P, c["spec"], FI.LENGTHS, gq, c["noise"], **kw)
        for key, w, r in (("z", wz, rz), ("m_q", wm, rm), ("logs_q", wl, rl)):
            margin(name, key, w, r)
    margin("last Flip dropped", "z_p", FR.flow_forward(P, rz, FI.LENGTHS, gq, drop_last_flip=True), rzp)
    margin("last Flip dropped", "flow", FR.flow_forward(P, zf, FI.LENGTHS, gq, drop_last_flip=True), rflow)
    margin("x1 * mask omitted (ragged row)", "flow", FR.flow_forward(P, zf, FI.LENGTHS, gq, no_x1_mask=True)[1:], rflow[1:])
    margin("noise_scale 0.667 on the posterior", "z", FR.posterior_encoder(P, c["spec"], FI.LENGTHS, gq, c["noise"], noise_scale=0.667)[0], rz)
    wkl = FR.kl_loss(z_p.numpy(), logs_q.numpy(), m_p.numpy(), logs_p.numpy(), FI.LENGTHS, per_channel=True)
    ratio = abs(wkl - rkl) / GATES["kl"]
    print(f"  {'KL divided by C * sum(len)':34s} {'kl':7s}: {ratio:.1f}")
    assert ratio > 20, ratio
    o_shift = m.dec(commons.slice_segments(torch.nn.functional.pad(z, (0, 1)), ids + 1, FI.SEG), g=g)
    margin("slice taken at ids + 1", "o", o_shift.numpy(), o.numpy())

    MG.save("flowvae", **out)
    size = os.path.getsize(os.path.join(HERE, "flowvae.npz"))
    assert size <= 128 * 1024, size


if __name__ == "__main__":
    main()
