#!/usr/bin/env python3
"""tests/golden/disc_losses.npz FROM THE REFERENCE ITSELF: MultiPeriodDiscriminator (vqvae/model_24k.py:298-431), feature_loss /
discriminator_loss / generator_loss (vqvae/modules/losses.py:4-40) and the loss_mel of train.py:268-307, on the CPU, in eval mode, grads
off.

Runs only in the build container (needs the reference checkout and transformers), under the shim of make_golden.py.  The discriminator
gets synthetic_state_dict(0, only_prefixes=["discriminators."], discriminator=True); librosa is stubbed, so the mel filterbank handed
to the reference's functions is detail_tts_amd.frontend.mel_filterbank, as for the front-end fixture.  Data only.  The inputs are drawn
by tests/disc_inputs.py from fixed seeds; the fixture stores their checksums.

Case A (B = 2, t = 10240) stores the reference's fp32 scalars (loss_fm, loss_disc, loss_gen, the three lists), float64 recomputations of
them and of the 37 per-map mean |r - g| (from the reference's fp32 maps), about 64 strided samples and the float64 (sum, sum of
squares, sum of magnitudes) of every score and feature map of both sides.  Case B (B = 3, t = 97) stores the same scalars and every
tensor in full when it has at most 256 elements, about 128 strided samples otherwise.  Case C: loss_mel on flowvae_inputs.case() with
the waveform disc_inputs.wav_c(), the reference's forward_flowvae driven as make_golden_flowvae.py drives it; also spec_to_mel's
samples.  `names` / `shapes`: the reference's D.state_dict().

The script fails unless every feature map of cases A and B has an rms in [1e-2, 1e2], real and generated maps differ by more than
1e3 x the gate (as the gate is taken: relative to the map's largest magnitude), tests/disc_ref.py (float64) agrees with the reference, and each mistake the feature can make moves a stored value by
more than 20 x the gate the GPU test uses (disc_inputs.GATES); the margins are printed.

    python tests/golden/make_golden_disc.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import disc_inputs as DI  # noqa: E402
import disc_ref as DR  # noqa: E402
import flowvae_inputs as FI  # noqa: E402


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def scalars(y_d_rs, y_d_gs, fmap_rs, fmap_gs):
    """float64 view of everything the loss functions return, from given scores / maps"""
    ld, lr, lg = DR.discriminator_loss(y_d_rs, y_d_gs)
    lgen, lgens = DR.generator_loss(y_d_gs)
    return dict(map_means=DR.map_means(fmap_rs, fmap_gs), loss_fm=DR.feature_loss(fmap_rs, fmap_gs), loss_disc=ld, losses_r=np.array(lr),
                losses_g=np.array(lg), loss_gen=lgen, losses_gen=np.array(lgens))


def main():
    MG.install_shim()
    import torch
    torch.set_grad_enabled(False)
    import vqvae.modules.commons as commons
    import vqvae.modules.losses as losses
    import vqvae.utils.data_utils as du
    from vqvae.model_24k import MultiPeriodDiscriminator
    from detail_tts_amd.frontend import mel_filterbank
    from detail_tts_amd.weights import discriminator_param_spec, select_discriminator_params, select_inference_params, synthetic_state_dict
    du.librosa_mel_fn = lambda sr, n_fft, n_mels, fmin, fmax: mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    G = DI.GATES

    D = MultiPeriodDiscriminator().eval()
    sd = synthetic_state_dict(MG.SEED_W, only_prefixes=["discriminators."], discriminator=True)
    ref_sd = D.state_dict()
    spec = discriminator_param_spec()
    assert list(ref_sd.keys()) == list(spec.keys()), "the spec must list the reference's names in its order"
    assert all(tuple(ref_sd[k].shape) == tuple(spec[k][0]) for k in spec)
    D.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    P = select_discriminator_params(sd)
    out = dict(names=np.array(list(ref_sd.keys())), shapes=np.array([",".join(str(n) for n in ref_sd[k].shape) for k in ref_sd]))

    def run(case, tag, sampler):
        y, y_hat = torch.from_numpy(case["y"]), torch.from_numpy(case["y_hat"])
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = D(y, y_hat)
        loss_fm = losses.feature_loss(fmap_rs, fmap_gs)
        loss_disc, r_losses, g_losses = losses.discriminator_loss(y_d_rs, y_d_gs)
        loss_gen, gen_losses = losses.generator_loss(y_d_gs)
        n = lambda ts: [t.numpy() for t in ts]
        sr, sg = n(y_d_rs), n(y_d_gs)
        fr, fg = [n(d) for d in fmap_rs], [n(d) for d in fmap_gs]
        assert [len(d) for d in fr] == [7, 6, 6, 6, 6, 6]
        out.update({f"{tag}_loss_fm": np.float32(float(loss_fm)), f"{tag}_loss_disc": np.float32(float(loss_disc)),
                    f"{tag}_loss_gen": np.float32(float(loss_gen)), f"{tag}_losses_r": np.array(r_losses, np.float32),
                    f"{tag}_losses_g": np.array(g_losses, np.float32), f"{tag}_losses_gen": np.array([float(v) for v in gen_losses], np.float32)})
        s64 = scalars(sr, sg, fr, fg)
        for k, v in s64.items():
            out[f"f64_{tag}_{k}"] = np.asarray(v, np.float64)
        samples, moms = [], []
        for side, scores, maps in (("r", sr, fr), ("g", sg, fg)):
            for kind, ts in (("score", scores), ("map", DI.flat_maps(maps))):
                for i, a in enumerate(ts):
                    assert len(samples) == DI.slot(kind, side, i)
                    samples.append(sampler(a))
                    moms.append(DI.moments(a))
                    rms = float(np.sqrt(np.mean(np.square(a.astype(np.float64)))))
                    assert kind == "score" or 1e-2 <= rms <= 1e2, (tag, side, i, rms)
        out[f"{tag}_samples"] = np.concatenate(samples).astype(np.float32)
        out[f"{tag}_sample_off"] = np.cumsum([0] + [len(v) for v in samples]).astype(np.int32)
        out[f"f64_{tag}_mom"] = np.array(moms, np.float64)
        out[f"{tag}_map_shapes"] = np.array([",".join(str(v) for v in a.shape) for a in DI.flat_maps(fr)])
        for k in ("y", "y_hat"):
            out[f"f64_sum_{tag}_{k}"] = DI.checksum(case[k])
        rms = [float(np.sqrt(np.mean(np.square(a.astype(np.float64))))) for a in DI.flat_maps(fr)]
        print(f"  case {tag}: loss_fm {float(loss_fm):.6f} loss_disc {float(loss_disc):.6f} loss_gen {float(loss_gen):.6f}; map rms {min(rms):.3f} .. {max(rms):.3f}")
        # real and generated differ, map by map and score by score
        diff = min(DI.relerr(a, b) for a, b in zip(DI.flat_maps(fr) + sr, DI.flat_maps(fg) + sg))
        print(f"  case {tag}: real and generated differ by at least {diff:.3e} of the map's largest magnitude in every map ({diff / G['map']:.0f} x the gate)")
        assert diff > 1e3 * G["map"], diff
        # ---- the float64 restatement is the reference's arithmetic (its own fp32 rounding apart)
        rr, rg, rfr, rfg = DR.mpd(P, case["y"], case["y_hat"])
        e = max(max(maxabs(a, b) for a, b in zip(DI.flat_maps(rfr) + rr, DI.flat_maps(fr) + sr)),
                max(maxabs(a, b) for a, b in zip(DI.flat_maps(rfg) + rg, DI.flat_maps(fg) + sg)))
        print(f"  case {tag}: float64 restatement off the reference's fp32 by {e:.3e} (every element)")
        assert e < 5e-5, e
        r64 = scalars(rr, rg, rfr, rfg)
        assert abs(r64["loss_fm"] - float(loss_fm)) < 1e-5 * max(1.0, abs(float(loss_fm)))
        return r64

    ra = run(DI.case_a(), "a", DI.sample_a)
    rb = run(DI.case_b(), "b", DI.sample_b)

    # ---- the mistakes the fixture must see: change of a stored scalar / its gate (relative gates: the scalars are O(0.1 .. 10))
    print("sensitivity margins (relative change of a stored scalar / gate):")

    def margin(name, wrong, right, keys, gate):
        ratio = max(float(np.max(np.abs(np.asarray(wrong[k]) - np.asarray(right[k])) / np.maximum(1e-30, np.abs(np.asarray(right[k]))))) for k in keys) / gate
        print(f"  {name:44s}: {ratio:.1f}")
        assert ratio > 20, (name, ratio)

    for tag, case, right in (("a", DI.case_a(), ra), ("b", DI.case_b(), rb)):
        def wrong(s_kw=None, p_kw=None):
            return scalars(*DR.mpd(P, case["y"], case["y_hat"], s_kw, p_kw))
        per = ("map_means", "losses_r", "losses_g", "losses_gen")
        margin(f"{tag}: zero pad instead of reflect pad", wrong(p_kw=dict(pad_mode="constant")), right, per, G["map_mean"])
        margin(f"{tag}: the pad applied on the left", wrong(p_kw=dict(left=True)), right, per, G["map_mean"])
        margin(f"{tag}: groups ignored (every group reads group 0)", wrong(s_kw=dict(group_of=lambda g: 0)), right, per, G["map_mean"])
        margin(f"{tag}: groups off by one", wrong(s_kw=dict(group_of=lambda g: max(g - 1, 0))), right, per, G["map_mean"])
        margin(f"{tag}: stride 4 taken as 3", wrong(s_kw=dict(stride=3)), right, per, G["map_mean"])
        margin(f"{tag}: leaky slope 0.01", wrong(s_kw=dict(slope=0.01), p_kw=dict(slope=0.01)), right, per, G["map_mean"])
        rr, rg, rfr, rfg = DR.mpd(P, case["y"], case["y_hat"])
        margin(f"{tag}: feature_loss without the factor 2", dict(loss_fm=DR.feature_loss(rfr, rfg, factor=1.0)), right, ("loss_fm",), G["loss"])
        margin(f"{tag}: conv_post's map left out", dict(loss_fm=DR.feature_loss(rfr, rfg, skip_post=True)), right, ("loss_fm",), G["loss"])
        margin(f"{tag}: mean taken per row", dict(map_means=DR.map_means(rfr, rfg, per_row=True)), right, ("map_means",), G["map_mean"])
        # [p, H] instead of [H, p] flatten order: the means cannot see it, the score's stored samples do - in case A only (at t = 97
        # every DiscriminatorP ends with H = 1, where the two orders are one)
        if tag != "a":
            continue
        sampler = DI.sample_a
        d = 5
        ok, swapped = DR.disc_p(P, d, case["y"])[0], DR.disc_p(P, d, case["y"], flatten_ph=True)[0]
        ratio = DI.relerr(sampler(swapped), sampler(ok)) / G["score"]
        print(f"  {tag + ': [p, H] instead of [H, p] flatten order':44s}: {ratio:.1f}")
        assert ratio > 20, ratio

    # ---- case C: loss_mel of the stage (train.py:268-307) on the flow-VAE fixture's case
    m = MG.build_reference_model()
    sdq = synthetic_state_dict(MG.SEED_W, only_prefixes=["enc_q."], posterior=True)
    m.enc_q.load_state_dict({k[len("enc_q."):]: torch.from_numpy(v) for k, v in sdq.items()}, strict=True)
    c = FI.case()
    y, yl, spec_t = torch.from_numpy(c["y"]), torch.from_numpy(c["y_lengths"]), torch.from_numpy(c["spec"])
    o_randn_like, o_rand = torch.randn_like, torch.rand
    torch.randn_like = lambda x, **kw: torch.from_numpy(c["noise"])
    torch.rand = lambda *a, **kw: torch.tensor(FI.RAND_FRACTIONS, dtype=torch.float32)
    try:
        y_hat, _, _, _, ids, _, _, _ = m.forward_flowvae(y, yl, {"spec": spec_t})
    finally:
        torch.randn_like, torch.rand = o_randn_like, o_rand
    assert ids.tolist() == list(FI.IDS_SLICE)
    mel = du.spec_to_mel_torch(spec_t, 1024, 128, 24000, 0.0, None)
    y_mel = commons.slice_segments(mel, ids, FI.SEG)
    y_hat_mel = du.mel_spectrogram_torch(y_hat.squeeze(1), 1024, 128, 24000, 256, 1024, 0.0, None)
    loss_mel = torch.nn.functional.l1_loss(y_mel, y_hat_mel) * 45
    wav = DI.wav_c()
    y_wav = commons.slice_segments(torch.from_numpy(wav), ids * 256, FI.SEG * 256)
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = D(y_wav, y_hat)
    out.update(c_loss_mel=np.float32(float(loss_mel)), c_spec_to_mel=mel.numpy()[:, ::4, ::3], f64_c_mom_spec_to_mel=DI.moments(mel.numpy()),
               c_loss_fm=np.float32(float(losses.feature_loss(fmap_rs, fmap_gs))),
               c_loss_disc=np.float32(float(losses.discriminator_loss(y_d_rs, y_d_gs)[0])),
               c_loss_gen=np.float32(float(losses.generator_loss(y_d_gs)[0])), f64_sum_c_wav=DI.checksum(wav))
    e = maxabs(DR.spec_to_mel(c["spec"], mel_filterbank(24000, 1024, 128, 0.0, None)), mel.numpy())
    print(f"  case c: loss_mel {float(loss_mel):.6f}; float64 spec_to_mel off the reference by {e:.3e}")
    assert e < 1e-4, e
    ratio = abs(float(loss_mel) / 45 - float(loss_mel)) / max(1.0, abs(float(loss_mel))) / G["loss_mel"]
    print(f"  {'c: loss_mel without the factor 45':44s}: {ratio:.1f}")
    assert ratio > 20, ratio

    MG.save("disc_losses", **out)
    size = os.path.getsize(os.path.join(HERE, "disc_losses.npz"))
    print(f"  {size / 1024:.1f} KiB")
    assert size <= 128 * 1024, size


if __name__ == "__main__":
    main()
