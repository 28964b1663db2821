"""Host side of the flow-VAE stage forward (no GPU): the optional enc_q tensors (weights.posterior_param_spec), their packing, the
host-drawn segment starts, the argument checks that must fail before anything is launched, and the float64 restatement
tests/flowvae_ref.py against the reference's own numbers in tests/golden/flowvae.npz."""
import types

import numpy as np
import pytest

import flowvae_inputs as FI
import flowvae_ref as FR

# |float64 restatement - the reference's own fp32 result| over the stored samples, measured on the CPU by
# tests/golden/make_golden_flowvae.py: z 1.9e-6, m_q 6.2e-7, logs_q 7.1e-7, z_p 2.1e-6, flow case 3.6e-7; x 20.  The KL scalars are
# fp32 values of 70.5 and 7.3: 20 fp32 ulps of the larger.
REF_GATE = {"z": 4e-5, "m_q": 1.3e-5, "logs_q": 1.5e-5, "z_p": 4.3e-5, "flow": 7.2e-6, "kl": 1.6e-4}


@pytest.fixture(scope="module")
def state_post():
    from detail_tts_amd.weights import synthetic_state_dict
    return synthetic_state_dict(0, posterior=True)


@pytest.fixture(scope="module")
def weights_post(state_post):
    from detail_tts_amd.weights import select_inference_params
    return select_inference_params(state_post)


class NoLaunchRt:
    """a runtime on which every call is a test failure: what must be rejected is rejected before the device is used"""

    def __getattr__(self, name):
        raise AssertionError(f"the runtime was reached ({name}) before the arguments were checked")


def test_posterior_param_spec_shapes():
    from detail_tts_amd.weights import inference_param_spec, optional_param_spec, posterior_param_spec
    spec = posterior_param_spec()
    hid, inter, gin = 192, 192, 768
    assert spec["enc_q.pre.weight"][0] == (hid, 1024 // 2 + 1, 1) and spec["enc_q.pre.bias"][0] == (hid,)
    for n, rows in (("bias", (2 * hid * 16,)), ("weight_g", (2 * hid * 16, 1, 1)), ("weight_v", (2 * hid * 16, gin, 1))):
        assert spec["enc_q.enc.cond_layer." + n][0] == rows
    for l in range(16):
        assert spec[f"enc_q.enc.in_layers.{l}.weight_v"][0] == (2 * hid, hid, 5)
        assert spec[f"enc_q.enc.in_layers.{l}.weight_g"][0] == (2 * hid, 1, 1) and spec[f"enc_q.enc.in_layers.{l}.bias"][0] == (2 * hid,)
        rs = 2 * hid if l < 15 else hid
        assert spec[f"enc_q.enc.res_skip_layers.{l}.weight_v"][0] == (rs, hid, 1)
        assert spec[f"enc_q.enc.res_skip_layers.{l}.weight_g"][0] == (rs, 1, 1) and spec[f"enc_q.enc.res_skip_layers.{l}.bias"][0] == (rs,)
    assert spec["enc_q.proj.weight"][0] == (2 * inter, hid, 1) and spec["enc_q.proj.bias"][0] == (2 * inter,)
    assert len(spec) == 2 + 3 + 16 * 3 + 16 * 3 + 2 and all(k.startswith("enc_q.") for k in spec)
    assert not set(spec) & (set(inference_param_spec()) | set(optional_param_spec()))
    # the spectrogram width follows data.filter_length
    from detail_tts_amd.config import load_config
    cfg = load_config(None)
    cfg["data"]["filter_length"] = 512
    assert posterior_param_spec(cfg)["enc_q.pre.weight"][0] == (hid, 257, 1)


def test_posterior_tensors_leave_every_other_tensor_bit_equal(weights, state_post, weights_post):
    from detail_tts_amd.weights import inference_param_spec, posterior_param_spec, synthetic_state_dict
    post = list(posterior_param_spec())
    assert list(state_post) == list(inference_param_spec()) + post
    assert set(weights_post) - set(weights) == {k for k in weights_post if k.startswith("enc_q.")} and len(set(weights_post) - set(weights)) == 70
    for k, v in weights.items():
        assert np.array_equal(v, weights_post[k]), k
    alone = synthetic_state_dict(0, only_prefixes=["enc_q."], posterior=True)
    assert list(alone) == post and all(np.array_equal(alone[k], state_post[k]) for k in post)
    assert not synthetic_state_dict(0, only_prefixes=["enc_q."])
    both = synthetic_state_dict(0, optional=True, posterior=True)
    assert list(both)[-len(post):] == post and np.array_equal(both["gpt.text_head.weight"], synthetic_state_dict(0, optional=True)["gpt.text_head.weight"])
    w = weights_post["enc_q.enc.in_layers.7.weight"]                    # weight-norm folded: a plain [2 hid, hid, 5] weight
    assert w.shape == (384, 192, 5) and w.dtype == np.float32 and float(np.abs(w).max()) > 0


def test_select_keeps_a_full_group_ignores_a_partial_one_and_refuses_a_misshaped_one(weights, state_post, weights_post):
    from detail_tts_amd.weights import select_inference_params
    plain = {k: v for k, v in state_post.items() if not k.startswith("enc_q.")}
    assert set(select_inference_params(plain)) == set(weights)
    lone = dict(plain)
    lone["enc_q.pre.weight"] = np.zeros((4, 4, 1), np.float32)          # a lone, mis-shaped training-only key: ignored as before
    sel = select_inference_params(lone)
    assert set(sel) == set(weights) and all(np.array_equal(sel[k], weights[k]) for k in weights)
    partial = {k: v for k, v in state_post.items() if k != "enc_q.proj.bias"}
    assert set(select_inference_params(partial)) == set(weights)
    bad = dict(state_post)
    bad["enc_q.pre.weight"] = np.zeros((192, 512, 1), np.float32)
    with pytest.raises(ValueError, match="enc_q.pre.weight"):
        select_inference_params(bad)
    bad = dict(state_post)
    bad["enc_q.enc.res_skip_layers.15.weight_v"] = np.ones((384, 192, 1), np.float32)
    bad["enc_q.enc.res_skip_layers.15.weight_g"] = np.ones((384, 1, 1), np.float32)
    with pytest.raises(ValueError, match="enc_q.enc.res_skip_layers.15.weight"):
        select_inference_params(bad)


def test_packed_blob_without_enc_q_is_unchanged_and_the_group_comes_last(weights, weights_post):
    from detail_tts_amd.packing import gate_perm, pack_all
    parts = ("vocoder", "vq")
    base = pack_all(weights, parts=parts)
    full = pack_all(weights_post, parts=parts)
    flat0, names0, off0, num0 = base.blob()
    flat1, names1, off1, num1 = full.blob()
    n = len(names0)
    assert names1[:n] == names0 and not [k for k in names0 if k.startswith("enc_q.")]
    assert all(k.startswith("enc_q.") for k in names1[n:]) and len(names1) > n
    assert np.array_equal(off1[:n], off0) and np.array_equal(num1[:n], num0)
    assert np.array_equal(flat1[:flat0.size], flat0)                      # byte-identical front: the blob without enc_q is today's
    assert not [k for k in pack_all(weights_post, parts=("diffusion",)).entries if k.startswith("enc_q.")]
    e = full.entries
    assert e["enc_q.pre.wp"].shape == (1, 528, 256) and e["enc_q.enc.cond_layer.wp"].shape == (1, 768, 6144)
    assert e["enc_q.proj.wp"].shape == (1, 192, 384) and "enc_q.enc.res_skip_layers.15.res.wp" not in e
    assert e["enc_q.enc.res_skip_layers.14.res.wp"].shape == e["enc_q.enc.res_skip_layers.15.skip.wp"].shape == (1, 192, 256)
    # gate-interleaved rows, as the flow's WaveNet: packed rows (2r, 2r + 1) = (tanh half r, sigmoid half r), per layer in cond_layer
    gp = gate_perm(384)
    w = weights_post["enc_q.enc.in_layers.9.weight"]
    assert np.array_equal(e["enc_q.enc.in_layers.9.wp"][:, :, :384], w[gp].transpose(2, 1, 0))
    wc = weights_post["enc_q.enc.cond_layer.weight"]
    assert np.array_equal(e["enc_q.enc.cond_layer.wp"][0, :, 9 * 384:10 * 384], wc[9 * 384 + gp, :, 0].T)
    rs = weights_post["enc_q.enc.res_skip_layers.3.weight"]
    assert np.array_equal(e["enc_q.enc.res_skip_layers.3.res.wp"][0, :, :192], rs[:192, :, 0].T)
    assert np.array_equal(e["enc_q.enc.res_skip_layers.3.skip.wp"][0, :, :192], rs[192:, :, 0].T)


def test_host_drawn_segment_starts_stay_in_range():
    from detail_tts_amd.vqvae.model_24k import draw_segment_starts
    lens = [40, 41, 44, 48, 400, 40, 1000]
    seen = set()
    for seed in range(200):
        ids = draw_segment_starts(seed, lens, 40)
        assert ids == draw_segment_starts(seed, lens, 40) and len(ids) == len(lens)
        assert all(0 <= i <= n - 40 for i, n in zip(ids, lens)), (seed, ids)
        assert ids[0] == 0 and ids[5] == 0                                  # len == seg: the only start
        seen.add(ids[3])
    assert seen == set(range(9))                                            # every start of a 48-frame row, the last (8) included
    assert draw_segment_starts(1, lens, 40) != draw_segment_starts(2, lens, 40)


def test_bad_arguments_are_rejected_before_any_launch():
    torch = pytest.importorskip("torch")
    from detail_tts_amd.config import load_config
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn, check_flowvae_args
    fake = types.SimpleNamespace(rt=NoLaunchRt(), device="cpu", cfg=load_config(None))
    data = {"spec": torch.zeros(2, 513, 48)}
    with pytest.raises(ValueError, match="divisible by 4"):
        SynthesizerTrn.forward_flowvae(fake, torch.zeros(2, 128, 46), [46, 44], data)
    with pytest.raises(ValueError, match="fewer than the segment"):
        SynthesizerTrn.forward_flowvae(fake, torch.zeros(2, 128, 48), [48, 39], data)
    with pytest.raises(ValueError, match="ids_slice"):
        SynthesizerTrn.forward_flowvae(fake, torch.zeros(2, 128, 48), [48, 44], data, ids_slice=[8, 5])
    with pytest.raises(ValueError, match="ids_slice"):
        SynthesizerTrn.forward_flowvae(fake, torch.zeros(2, 128, 48), [48, 44], data, ids_slice=[-1, 0])
    with pytest.raises(ValueError, match="ids_slice"):
        SynthesizerTrn.forward_flowvae(fake, torch.zeros(2, 128, 48), [48, 44], data, ids_slice=[0])
    with pytest.raises(ValueError, match="lengths"):
        SynthesizerTrn.forward_flowvae(fake, torch.zeros(2, 128, 48), [48], data)
    with pytest.raises(ValueError, match="length 52"):
        SynthesizerTrn.forward_flowvae(fake, torch.zeros(2, 128, 48), [52, 44], data)
    with pytest.raises(ValueError, match="divisible by 4"):                # forward_all checks through forward_flowvae, first
        SynthesizerTrn.forward_all(types.SimpleNamespace(forward_flowvae=lambda *a, **k: SynthesizerTrn.forward_flowvae(fake, *a, **k)),
                                   torch.zeros(2, 128, 46), [46, 44], data)
    assert check_flowvae_args((2, 128, 48), torch.tensor([48, 44]), 40, torch.tensor([8, 4])) == ([48, 44], [8, 4])
    assert check_flowvae_args((2, 128, 48), [48, 40], 40) == ([48, 40], None)


def test_seeded_inputs_are_the_ones_the_fixture_was_made_of(golden):
    g = golden("flowvae")
    c = FI.case()
    for k in ("y", "spec", "noise"):
        assert np.array_equal(FI.checksum(c[k]), g["f64_sum_" + k]), k
    assert np.array_equal(FI.checksum(FI.flow_case()), g["f64_sum_flow_in"])
    assert c["spec"].shape == (2, 513, 48) and float(c["spec"].min()) >= 0 and c["noise"].shape == (2, 192, 48)
    assert g["ids_slice"].tolist() == [8, 0] and g["ids_slice"].dtype == np.int64
    assert [int(np.floor(np.float32(u) * np.float32(n - 40 + 1))) for u, n in zip(FI.RAND_FRACTIONS, FI.LENGTHS)] == [8, 0]
    assert np.array_equal(g["y_mask"], FR.sequence_mask(FI.LENGTHS, 48).astype(np.float32))
    for k in FI.LATENTS + ("quantized", "flow"):
        assert g["s_" + k].shape == (2, 48, 16) and g["f64_mom_" + k].dtype == np.float64
    assert g["s_o"].shape == (2, 1, 1280) and g["g"].shape == (2, 768)
    # the stored samples include a column beyond the ragged row's length (t = 45): zero in the six masked latents and the flow case
    cols = np.arange(48)[::FI.LATENT_STRIDE[1]]
    assert cols[cols >= 44].tolist() == [45]
    for k in FI.LATENTS + ("flow",):
        assert np.all(g["s_" + k][1][:, cols >= 44] == 0) and np.abs(g["s_" + k][1][:, cols < 44]).max() > 0, k
    assert np.abs(g["s_quantized"][1][:, cols >= 44]).max() > 0            # out_proj's bias: the reference does not mask it


def test_float64_restatement_reproduces_the_fixture(golden, weights_post):
    """tests/flowvae_ref.py (enc_q, the forward flow, the KL) on the seeded inputs and the fixture's g gives the reference's stored
    samples, moments and KL within REF_GATE, and every mistake the generator lists is a mistake here too"""
    g = golden("flowvae")
    c = FI.case()
    P, gq = weights_post, g["g"]
    z, m_q, logs_q = FR.posterior_encoder(P, c["spec"], FI.LENGTHS, gq, c["noise"])
    z_p = FR.flow_forward(P, z, FI.LENGTHS, gq)
    flow = FR.flow_forward(P, FI.flow_case(), FI.LENGTHS, gq)
    for k, a in (("z", z), ("m_q", m_q), ("logs_q", logs_q), ("z_p", z_p), ("flow", flow)):
        err = float(np.abs(FI.sample(a) - g["s_" + k]).max())
        mom = np.abs(FI.moments(a) - g["f64_mom_" + k]) / np.maximum(1.0, np.abs(g["f64_mom_" + k]))
        print(f"flowvae_ref {k}: samples off by {err:.3e}, moments by {mom}")
        assert err < REF_GATE[k], (k, err)
        assert mom.max() < 1e-5, (k, mom)
        assert np.all(a[1, :, 44:] == 0)
    kl_q = FR.kl_loss(z_p, logs_q, m_q, 0.5 * logs_q, FI.LENGTHS)
    print(f"flowvae_ref kl_q: {kl_q:.6f} against the reference's {float(g['kl_q']):.6f}")
    assert abs(kl_q - float(g["kl_q"])) < REF_GATE["kl"]
    assert abs(FR.kl_loss(z_p, logs_q, m_q, 0.5 * logs_q, FI.LENGTHS, per_channel=True) * 192 - kl_q) < 1e-9
    # the mistakes
    wrong = FR.posterior_encoder(P, c["spec"], FI.LENGTHS, gq, c["noise"], layers_run=4)[1]
    assert np.abs(FI.sample(wrong) - g["s_m_q"]).max() > 1e-2
    wrong = FR.posterior_encoder(P, c["spec"], FI.LENGTHS, gq, c["noise"], cond_mod=4)[1]
    assert np.abs(FI.sample(wrong) - g["s_m_q"]).max() > 1e-2
    assert np.abs(FI.sample(FR.flow_forward(P, z, FI.LENGTHS, gq, drop_last_flip=True)) - g["s_z_p"]).max() > 1e-1
    assert np.abs(FR.flow_forward(P, FI.flow_case(), FI.LENGTHS, gq, no_x1_mask=True)[1, :, 44:]).max() > 1e-1
    assert np.array_equal(FR.slice_segments(z, (8, 0), 40)[0], z[0, :, 8:48]) and np.array_equal(FR.slice_segments(z, (8, 0), 40)[1], z[1, :, :40])
