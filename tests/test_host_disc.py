"""Host side of the flow-VAE stage's losses: the discriminator's weight spec, the 4-D weight-norm fold, the packer (a blob without the
discriminator is byte-identical to before; the stride-3 convs' two-tap form), the float64 restatement tests/disc_ref.py against the
reference's numbers in tests/golden/disc_losses.npz, the compat module paths and the argument checks that need no device."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import disc_inputs as DI
import disc_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sha256 over the names, offsets, sizes and bytes of the seed-0 blob of all parts, computed on the commit before the discriminator existed
PARENT_BLOB_SHA256 = "c9636637dca1290a834adea948ed9ecfee1452c16673c679a5114c438e73a07a"
# ... and of the seed-0 state dicts with the optional tensors and enc_q (every existing tensor keeps its draw)
PARENT_STATE_SHA256 = "8ee62b4826038f3759160d462a1061bf8550de85d9980c080be4e7e064baf4df"


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@pytest.fixture(scope="module")
def disc_weights():
    from detail_tts_amd.weights import select_discriminator_params, synthetic_state_dict
    return select_discriminator_params(synthetic_state_dict(0, only_prefixes=("discriminators.",), discriminator=True))


def test_param_spec_is_the_references_state_dict(golden):
    from detail_tts_amd.weights import DISC_PERIODS, discriminator_param_spec
    g = golden("disc_losses")
    spec = discriminator_param_spec()
    assert list(spec.keys()) == [str(n) for n in g["names"]]
    assert [",".join(str(v) for v in s) for s, _ in spec.values()] == [str(s) for s in g["shapes"]]
    assert DISC_PERIODS == DI.PERIODS and len(spec) == 3 * (7 + 5 * 6)
    assert spec["discriminators.1.convs.1.weight_v"][0] == (128, 32, 5, 1) and spec["discriminators.0.convs.4.weight_v"][0] == (1024, 4, 41)


def test_weight_norm_fold_of_conv2d_weights():
    from detail_tts_amd.weights import fold_weight_norm
    rs = np.random.RandomState(5)
    v = rs.randn(6, 3, 5, 1).astype(np.float32)
    gg = rs.uniform(0.5, 2.0, size=(6, 1, 1, 1)).astype(np.float32)
    want = gg.astype(np.float64) * v.astype(np.float64) / np.sqrt((v.astype(np.float64) ** 2).sum(axis=(1, 2, 3), keepdims=True))
    for state in ({"d.weight_g": gg, "d.weight_v": v, "d.bias": np.zeros(6, np.float32)},
                  {"d.parametrizations.weight.original0": gg, "d.parametrizations.weight.original1": v}):
        w = fold_weight_norm(state)["d.weight"]
        assert w.shape == (6, 3, 5, 1) and w.dtype == np.float32
        assert maxabs(w, want) <= 2.0 ** -24 * float(np.abs(want).max())          # the float64 result, rounded once
    # every row of the folded weight has the norm g
    assert np.allclose(np.sqrt((w.astype(np.float64) ** 2).sum(axis=(1, 2, 3))), gg.reshape(-1), rtol=1e-6)


def _sha(h, a):
    a = np.ascontiguousarray(a)
    h.update(str(a.shape).encode() + str(a.dtype).encode() + a.tobytes())


def test_blob_without_the_discriminator_is_byte_identical_to_the_parents():
    from detail_tts_amd.packing import pack_all
    from detail_tts_amd.runtime import ALL_PARTS
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    sd = synthetic_state_dict(0, optional=True, posterior=True)
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        _sha(h, v)
    assert h.hexdigest() == PARENT_STATE_SHA256
    assert not any(k.startswith("discriminators.") for k in sd)
    flat, names, offsets, numels = pack_all(select_inference_params(synthetic_state_dict(0)), parts=ALL_PARTS).blob()
    h = hashlib.sha256()
    h.update("\n".join(names).encode())
    for a in (offsets, numels, flat):
        _sha(h, a)
    assert h.hexdigest() == PARENT_BLOB_SHA256
    assert not any(n.startswith("discriminators.") for n in names)
    # drawing the discriminator next to the others changes none of them
    both = synthetic_state_dict(0, only_prefixes=("enc_p.", "discriminators.0.convs.0."), discriminator=True)
    assert all(np.array_equal(both[k], sd[k]) for k in both if k.startswith("enc_p."))
    assert "discriminators.0.convs.0.weight_v" in both


def test_packed_discriminator(disc_weights):
    from detail_tts_amd.packing import pack_discriminator, stride3_as_two_taps
    pk = pack_discriminator(disc_weights)
    flat, names, offsets, numels = pk.blob()
    assert 46.7e6 < flat.size < 52e6          # 46.7 M weights + the zero tap of the two-tap forms and the conv_posts' padding to 32 rows
    assert np.array_equal(pk.entries["discriminators.0.convs.0.weight"], disc_weights["discriminators.0.convs.0.weight"].reshape(-1))
    assert pk.entries["discriminators.2.convs.1.wp"].shape == (2, 96, 128) and pk.entries["discriminators.2.conv_post.wp"].shape == (3, 1024, 32)
    # the two-tap form of a (5, stride 3, pad 2) conv over the input de-interleaved by 3 is that conv: every H mod 3, H = 1 included
    rs = np.random.RandomState(6)
    w, b = rs.randn(4, 3, 5), rs.randn(4)
    for H in (1, 2, 3, 7, 9, 17):
        x = rs.randn(2, 3, H)
        M = -(-H // 3)
        xp = np.zeros((2, 3, 3 * M))
        xp[:, :, :H] = x
        dein = xp.reshape(2, 3, M, 3).transpose(0, 1, 3, 2).reshape(2, 9, M)            # [r][3 c + j][m] = x[r][c][3 m + j]
        weq = stride3_as_two_taps(w.astype(np.float32)).astype(np.float64)
        two = DR.conv1d(np.pad(dein, ((0, 0), (0, 0), (1, 0))), weq, b)                 # left pad 1, 2 taps, stride 1
        assert two.shape == (2, 4, M)
        assert maxabs(two, DR.conv1d(x, w.astype(np.float32), b, stride=3, pad=2)) < 1e-12


def test_float64_restatement_against_the_reference(golden, disc_weights):
    g = golden("disc_losses")
    c = DI.case_b()
    assert np.array_equal(DI.checksum(c["y"]), g["f64_sum_b_y"]) and np.array_equal(DI.checksum(c["y_hat"]), g["f64_sum_b_y_hat"])
    assert np.array_equal(DI.checksum(DI.case_a()["y"]), g["f64_sum_a_y"]) and np.array_equal(DI.checksum(DI.wav_c()), g["f64_sum_c_wav"])
    rr, rg, rfr, rfg = DR.mpd(disc_weights, c["y"], c["y_hat"])
    assert [len(d) for d in rfr] == [7, 6, 6, 6, 6, 6]
    assert [",".join(str(v) for v in a.shape) for a in DI.flat_maps(rfr)] == [str(s) for s in g["b_map_shapes"]]
    for side, scores, maps in (("r", rr, rfr), ("g", rg, rfg)):
        for kind, ts in (("score", scores), ("map", DI.flat_maps(maps))):
            for i, a in enumerate(ts):
                samples, mom = DI.stored(g, "b", kind, side, i)
                assert maxabs(DI.sample_b(a), samples) < 5e-5, (kind, side, i)
                assert np.allclose(DI.moments(a), mom, rtol=1e-4, atol=1e-3)
    assert np.allclose(DR.map_means(rfr, rfg), g["f64_b_map_means"], rtol=1e-4)
    for got, key in ((DR.feature_loss(rfr, rfg), "b_loss_fm"), (DR.discriminator_loss(rr, rg)[0], "b_loss_disc"), (DR.generator_loss(rg)[0], "b_loss_gen")):
        assert abs(got - float(g[key])) < 1e-5 * max(1.0, abs(got)), key
    assert np.allclose(DR.discriminator_loss(rr, rg)[1], g["b_losses_r"], rtol=1e-5) and np.allclose(DR.generator_loss(rg)[1], g["b_losses_gen"], rtol=1e-5)
    # the split itself: reflect on the right, [H, p] order
    x = np.arange(7, dtype=np.float32)[None, None]
    assert DR.period_split(x, 3)[0, 0].tolist() == [[0, 1, 2], [3, 4, 5], [6, 5, 4]]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "disc_losses.npz")) <= 128 * 1024


def test_reference_imports_resolve_through_compat():
    code = ("from vqvae.model_24k import SynthesizerTrn, MultiPeriodDiscriminator\n"
            "from vqvae.modules.losses import generator_loss, discriminator_loss, feature_loss, kl_loss\n"
            "import detail_tts_amd.vqvae.model_24k as M, detail_tts_amd.vqvae.modules.losses as L\n"
            "assert MultiPeriodDiscriminator is M.MultiPeriodDiscriminator and feature_loss is L.feature_loss and kl_loss is L.kl_loss\n"
            "from prepare.load_infer import load_discriminator, load_model\n"
            "import inspect\n"
            "assert list(inspect.signature(load_model).parameters) == ['model_name', 'model_path', 'config_path', 'device']\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=os.path.join(ROOT, "tests"), env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_argument_checks_that_need_no_device(disc_weights, tmp_path):
    torch = pytest.importorskip("torch")
    from detail_tts_amd.prepare.load_infer import load_discriminator
    from detail_tts_amd.runtime import DttsError
    from detail_tts_amd.vqvae.model_24k import MultiPeriodDiscriminator
    from detail_tts_amd.vqvae.modules import losses as L
    from detail_tts_amd.weights import select_discriminator_params
    with pytest.raises(NotImplementedError, match="use_spectral_norm"):
        MultiPeriodDiscriminator(use_spectral_norm=True)
    with pytest.raises(ValueError, match="not both"):
        MultiPeriodDiscriminator(model=object(), device="cuda:0")
    d = MultiPeriodDiscriminator.__new__(MultiPeriodDiscriminator)          # the shape checks come before anything touches the device
    with pytest.raises(ValueError, match="y and y_hat"):
        d.forward(torch.zeros(2, 1, 97), torch.zeros(2, 1, 96))
    with pytest.raises(ValueError, match="y and y_hat"):
        d.forward(torch.zeros(2, 97), torch.zeros(2, 97))
    with pytest.raises(ValueError, match="at least 12"):
        d.forward(torch.zeros(2, 1, 11), torch.zeros(2, 1, 11))
    missing = {k: v for k, v in disc_weights.items() if k != "discriminators.3.conv_post.bias"}
    with pytest.raises(KeyError, match="discriminators.3.conv_post.bias"):
        select_discriminator_params(missing)
    bad = dict(disc_weights)
    bad["discriminators.0.convs.1.weight"] = np.zeros((64, 16, 41), np.float32)       # the ungrouped shape
    with pytest.raises(ValueError, match="discriminators.0.convs.1.weight"):
        select_discriminator_params(bad)
    with pytest.raises(DttsError, match="CUDA"):
        L.feature_loss([[torch.zeros(2, 3)]], [[torch.zeros(2, 3)]])
    with pytest.raises(DttsError, match="CUDA"):
        L.generator_loss([torch.zeros(2, 3)])
    ck = tmp_path / "g_only.pt"
    torch.save({"G": {}}, ck)
    with pytest.raises(KeyError, match="'D'"):
        load_discriminator(str(ck), "cuda:0")
