"""CPU: the sampler options' host side - space_timesteps / SpacedDiffusion tables against the reference's own (sampler_tables.npz,
make_golden_sampler.py), and argument checks that must fire before any device work."""
import numpy as np
import pytest

from detail_tts_amd.vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps

TABLES = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "alphas_cumprod_next", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
          "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
          "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")


def diffuser(n, **kw):
    return SpacedDiffusion(space_timesteps(4000, n if isinstance(n, str) else [n]), betas=get_named_beta_schedule("linear", 4000),
                           conditioning_free=kw.pop("conditioning_free", True), conditioning_free_k=2.0, **kw)


@pytest.mark.parametrize("key,n", [("10", 10), ("25", 25), ("200", 200), ("ddim25", "ddim25")])
def test_spaced_diffusion_tables_equal_reference(golden, key, n):
    g = golden("sampler_tables")
    d = diffuser(n)
    assert d.timestep_map == g[f"tmap_{key}"].tolist()
    assert d.num_timesteps == len(g[f"tmap_{key}"])
    for t in TABLES:
        ref = g[f"f64_{key}_{t}"]
        got = getattr(d, t)
        assert got.dtype == np.float64 and got.shape == ref.shape, t
        assert np.max(np.abs(got - ref)) <= 1e-12, t


def test_space_timesteps_string_forms(golden):
    g = golden("sampler_tables")
    assert sorted(space_timesteps(4000, [1])) == g["tmap_1"].tolist()
    assert space_timesteps(4000, "25") == space_timesteps(4000, [25]) == set(g["tmap_25"].tolist())
    assert space_timesteps(4000, "10,15") == space_timesteps(4000, [10, 15])
    assert space_timesteps(4000, "ddim25") == set(range(0, 4000, 160)) == set(g["tmap_ddim25"].tolist())
    with pytest.raises(ValueError):
        space_timesteps(4000, "ddim3999")


def test_one_step_schedule_builds():
    d = diffuser(1)
    assert d.timestep_map == [0] and d.num_timesteps == 1


class _NoDevice:
    """a model whose runtime must never be touched"""
    @property
    def rt(self):
        raise AssertionError("device work before the arguments were checked")


def _loop_kwargs():
    return dict(model_kwargs={"precomputed_aligned_embeddings": object()})


def test_sample_loop_dispatch_errors_before_device_work():
    with pytest.raises(NotImplementedError, match="dpm"):
        diffuser(50, sampler="dpm++2m").sample_loop(_NoDevice(), (1, 128, 8), **_loop_kwargs())
    with pytest.raises(ValueError):
        diffuser(50, sampler="plms").sample_loop(_NoDevice(), (1, 128, 8), **_loop_kwargs())
    with pytest.raises(NotImplementedError, match="conditioning_free"):
        diffuser(50, conditioning_free=False).p_sample_loop(_NoDevice(), (1, 128, 8), **_loop_kwargs())
    with pytest.raises(NotImplementedError, match="rescale_timesteps"):
        diffuser(50, rescale_timesteps=True).ddim_sample_loop(_NoDevice(), (1, 128, 8), **_loop_kwargs())
    with pytest.raises(ValueError, match="eta"):
        diffuser(50).ddim_sample_loop(_NoDevice(), (1, 128, 8), eta=-0.5, **_loop_kwargs())


def test_reference_default_sampler_fields():
    d = diffuser(50)
    assert d.sampler == "ddim"                          # the reference's GaussianDiffusion default
    assert diffuser(50, sampler="p").sampler == "p"


@pytest.mark.parametrize("kw", [dict(diffusion_steps=0), dict(diffusion_steps=4001), dict(diffusion_steps=2.5), dict(diffusion_steps=True),
                                dict(sampler="euler"), dict(eta=-1.0), dict(eta=float("nan")), dict(eta="x")])
def test_infer_arguments_rejected_before_any_launch(kw):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    for fn in (SynthesizerTrn.infer, lambda self, *a, **k: next(SynthesizerTrn.infer_stream(self, [{}], **k))):
        with pytest.raises(ValueError):
            fn(_NoDevice(), None, None, None, None, **kw)


def test_infer_dpm_sampler_not_implemented():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    with pytest.raises(NotImplementedError, match="dpm"):
        SynthesizerTrn.infer(_NoDevice(), None, None, None, None, sampler="dpm++2m")


def test_sampling_args_defaults_are_the_reference_schedule():
    from detail_tts_amd.vqvae.model_24k import sampling_args
    ts, sid, eta = sampling_args()
    assert ts == sorted(space_timesteps(4000, [50])) and sid == 0 and eta == 0.0
    ts, sid, eta = sampling_args(20, "ddim", 0.5)
    assert len(ts) == 20 and sid == 1 and eta == 0.5
    assert sampling_args(np.int64(4000))[0] == list(range(4000))
