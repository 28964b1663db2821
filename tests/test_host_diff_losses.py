"""Host side of the diffusion / VQ stage validation losses (no GPU): the float64 restatement tests/diff_loss_ref.py against the
reference's own numbers in tests/golden/diff_losses.npz, the mirror's 200-step schedule tables against the reference's, and the
argument checks that must fail before anything is launched."""
import types

import numpy as np
import pytest

import diff_loss_inputs as DI
import diff_loss_ref as DR

# |float64 restatement on the stored fp32 model output - the reference's own fp32 result|, measured on the CPU by
# tests/golden/make_golden_diff_losses.py: mse 1.5e-7, vb 1.9e-7, loss 1.4e-7; x 20
REF_GATE = {"mse": 3e-6, "vb": 4e-6, "loss": 3e-6}


@pytest.fixture(scope="module")
def diffuser():
    from detail_tts_amd.vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    return SpacedDiffusion(space_timesteps(4000, [200]), betas=get_named_beta_schedule("linear", 4000), conditioning_free=False)


class NoLaunchRt:
    """a runtime on which every call except get_option is a test failure: what must be rejected is rejected before the device is used"""

    def __init__(self, trunk_fp16=0):
        self._fp16 = trunk_fp16

    def get_option(self, key):
        assert key == "trunk_fp16"
        return self._fp16

    def __getattr__(self, name):
        raise AssertionError(f"the runtime was reached ({name}) before the arguments were checked")


def test_seeded_inputs_are_the_ones_the_fixture_was_made_of(golden):
    g = golden("diff_losses")
    a = DI.case_a(golden("diff_cond"))
    for k in ("x_start", "noise", "aligned", "cond"):
        assert np.array_equal(DI.checksum(a[k]), g["f64_sum_a_" + k]), k
    b = DI.case_b(golden("gpt_forced"))
    for k in ("y", "raw_mel", "text"):
        assert np.array_equal(DI.checksum(b[k]), g["f64_sum_b_" + k]), k
    assert np.array_equal(DI.checksum(DI.case_b_noise()), g["f64_sum_b_noise"])
    assert np.array_equal(DI.checksum(DI.case_c()["y"]), g["f64_sum_c_y"])
    lo, hi = g["a_branch_counts"]
    assert (a["x_start"][0] < -0.999).sum() == lo >= 8 and (a["x_start"][0] > 0.999).sum() == hi >= 8     # all three NLL branches
    assert np.abs(a["x_start"][1:]).max() <= 0.95
    assert g["a_t"].tolist() == [0, 1, 199] and g["a_model_output"].shape == (3, 256, 36)
    assert b["text"].shape == (2, 13) and g["b_codes"].shape == (2, 9) and g["b_t"].shape == (2,)


def test_float64_restatement_reproduces_case_a(golden, diffuser):
    """tests/diff_loss_ref.py on the reference's stored model output gives the reference's mse / vb / loss within REF_GATE (the fp32-vs-
    float64 gap measured on the CPU: 1.5e-7 / 1.9e-7 / 1.4e-7, x 20), and its x_start_predicted within fp32 rounding of O(10) values."""
    g = golden("diff_losses")
    a = DI.case_a(golden("diff_cond"))
    x_t = DR.q_sample(diffuser, a["x_start"], a["t"], a["noise"])
    r = DR.loss_terms(diffuser, g["a_model_output"], a["x_start"], x_t, a["noise"], a["t"])
    for k in ("mse", "vb", "loss"):
        err = float(np.abs(r[k] - g["a_" + k].astype(np.float64)).max())
        print(f"diff_loss_ref case A {k}: {r[k]} err {err:.3e}")
        assert err < REF_GATE[k], (k, err)
    s0, s1 = (int(v) for v in g["a_pred_stride"])
    assert np.abs(r["pred_xstart"][:, ::s0, ::s1] - g["a_pred"]).max() < 1e-4
    # the mistakes the generator asserts the fixture can see are mistakes here too
    assert abs(DR.loss_terms(diffuser, g["a_model_output"], a["x_start"], x_t, a["noise"], a["t"], drop_t0=True)["vb"][0] - r["vb"][0]) > 0.1
    assert abs(DR.loss_terms(diffuser, g["a_model_output"], a["x_start"], x_t, a["noise"], a["t"], frac_zero=True)["vb"][1] - r["vb"][1]) > 1.0


def test_mirror_tables_equal_the_reference(golden, diffuser):
    g = golden("diff_losses")
    assert diffuser.num_timesteps == 200 and not diffuser.conditioning_free
    assert list(diffuser.timestep_map) == g["timestep_map"].tolist()
    for mine, key in ((diffuser.sqrt_alphas_cumprod, "f64_sqrt_alphas_cumprod"),
                      (diffuser.sqrt_one_minus_alphas_cumprod, "f64_sqrt_one_minus_alphas_cumprod"), (np.log(diffuser.betas), "f64_log_betas")):
        assert g[key].dtype == np.float64 and g[key].shape == (200,)
        assert np.allclose(mine, g[key], rtol=1e-13, atol=0), key


@pytest.mark.parametrize("t", [[0, 1, 200], [-1, 0, 1], [0, 1], [[0, 1, 2]], [0.5, 1, 2]])
def test_bad_timesteps_are_rejected_before_any_launch(diffuser, t):
    torch = pytest.importorskip("torch")
    from detail_tts_amd.vqvae.utils.diffusion import check_timesteps
    with pytest.raises(ValueError):
        check_timesteps(t, 3, 200)
    model = types.SimpleNamespace(rt=NoLaunchRt())
    x = torch.zeros(3, 128, 8)
    with pytest.raises(ValueError):
        diffuser.training_losses(model, x, torch.tensor(t), model_kwargs={"precomputed_aligned_embeddings": torch.zeros(3, 768, 8)})
    diffuser.rt = NoLaunchRt()
    try:
        with pytest.raises(ValueError):
            diffuser.q_sample(x, t, noise=x)
    finally:
        diffuser.rt = None


def test_check_timesteps_accepts_what_the_reference_passes():
    torch = pytest.importorskip("torch")
    from detail_tts_amd.vqvae.utils.diffusion import check_timesteps
    assert check_timesteps(torch.tensor([0, 1, 199]), 3, 200) == [0, 1, 199]
    assert check_timesteps(np.array([5], np.int32), 1, 200) == [5]
    assert check_timesteps([3.0, 4.0], 2, 200) == [3, 4]


def test_training_losses_refuses_the_fp16_trunk_and_missing_conditioning(diffuser):
    torch = pytest.importorskip("torch")
    x = torch.zeros(2, 128, 8)
    with pytest.raises(NotImplementedError, match="three-product trunk"):
        diffuser.training_losses(types.SimpleNamespace(rt=NoLaunchRt(trunk_fp16=1)), x, [0, 1],
                                 model_kwargs={"precomputed_aligned_embeddings": torch.zeros(2, 768, 8)})
    with pytest.raises(ValueError, match="precomputed_aligned_embeddings"):
        diffuser.training_losses(types.SimpleNamespace(rt=NoLaunchRt()), x, [0, 1], model_kwargs={"aligned_conditioning": x})


def test_forward_vq_needs_a_frame_count_divisible_by_4():
    torch = pytest.importorskip("torch")
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    fake = types.SimpleNamespace(rt=NoLaunchRt(), device="cpu")
    with pytest.raises(ValueError, match="divisible by 4"):
        SynthesizerTrn.forward_vq(fake, torch.zeros(1, 128, 38), [38], None)


@pytest.mark.parametrize("target", ["flowvae", "all", None])
def test_forward_names_enc_q_for_the_targets_it_does_not_have(target):
    from detail_tts_amd.vqvae.model_24k import FORWARD_TARGETS, SynthesizerTrn
    assert FORWARD_TARGETS == {"vqvae": "forward_vq", "gpt": "forward_gpt", "diff": "forward_diff"}
    with pytest.raises(NotImplementedError, match="enc_q"):
        SynthesizerTrn.forward(types.SimpleNamespace(target=target, rt=NoLaunchRt()), None, None, None)


def test_forward_dispatches_on_the_target():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    for target, name in (("vqvae", "forward_vq"), ("gpt", "forward_gpt"), ("diff", "forward_diff")):
        fake = types.SimpleNamespace(target=target, **{name: lambda y, yl, data, name=name: (name, y, yl, data)})
        assert SynthesizerTrn.forward(fake, 1, 2, 3) == (name, 1, 2, 3)


def test_forward_diff_checks_t_and_the_trunk_mode_first():
    torch = pytest.importorskip("torch")
    from detail_tts_amd.vqvae.model_24k import TRAIN_DIFFUSION_STEPS, SynthesizerTrn, draw_timesteps
    d = types.SimpleNamespace(num_timesteps=200)
    data = dict(raw_mel=torch.zeros(2, 128, 8))
    fake = types.SimpleNamespace(rt=NoLaunchRt(), device="cpu", diffuser=d, desired_diffusion_steps=200)
    with pytest.raises(ValueError):
        SynthesizerTrn.forward_diff(fake, None, None, data, t=[0, 200])
    with pytest.raises(ValueError):
        SynthesizerTrn.forward_diff(fake, None, None, data, t=[0])
    fake.rt = NoLaunchRt(trunk_fp16=1)
    with pytest.raises(NotImplementedError, match="three-product trunk"):
        SynthesizerTrn.forward_diff(fake, None, None, data, t=[0, 1])
    ts = draw_timesteps(3, 64)
    assert TRAIN_DIFFUSION_STEPS == 200 and ts == draw_timesteps(3, 64) and ts != draw_timesteps(4, 64)
    assert min(ts) >= 0 and max(ts) < 200 and len(set(ts)) > 20


def test_differing_timesteps_in_diffusion_forward_host_rules():
    """integer timesteps may differ between rows (the per-row entry); fractional ones, conditioning_free=True and the trained range
    are refused before the runtime is reached"""
    torch = pytest.importorskip("torch")
    from detail_tts_amd.vqvae.diff_model import DiffusionTts
    dm = DiffusionTts(NoLaunchRt(), dict(model_channels=768, in_channels=128, out_channels=256, num_heads=16))
    x, emb = torch.zeros(2, 128, 8), torch.zeros(2, 768, 8)
    with pytest.raises(ValueError, match="FRACTIONAL"):
        dm.forward(x, torch.tensor([1.5, 2.0]), precomputed_aligned_embeddings=emb)
    with pytest.raises(ValueError, match="conditioning_free"):
        dm.forward(x, torch.tensor([1, 2]), conditioning_free=True)
    with pytest.raises(ValueError, match="trained range"):
        dm.forward(x, torch.tensor([1, 4000]), precomputed_aligned_embeddings=emb)
    with pytest.raises(AssertionError, match="diff_forward_rows"):       # two integer timesteps: routed to the per-row entry
        dm.forward(x, torch.tensor([1, 2]), precomputed_aligned_embeddings=emb)
