"""CPU: the DPM-Solver++(2M) sampler's host side - the host-only schedule table (dtts_dpm_schedule_table) against the reference's own
solver arithmetic (dpm_tables.npz, make_golden_dpm.py), and argument checks that must fire before any device work."""
import os

import numpy as np
import pytest

from detail_tts_amd.vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps

# alpha, sigma, lambda, sigma_t / sigma_s and 1 / r0 are measured bit-identical to the reference here; alpha_t * expm1(-h) within 2 ulps
# (the reference's expm1 / exp of a 0-d tensor against the C library's); the gate allows 4 ulps for another libm
MAX_ULPS = 4


def diffuser(n, **kw):
    return SpacedDiffusion(space_timesteps(4000, [n]), betas=get_named_beta_schedule("linear", 4000),
                           conditioning_free=kw.pop("conditioning_free", True), conditioning_free_k=kw.pop("conditioning_free_k", 2.0), **kw)


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape and np.all(np.sign(a) == np.sign(b))
    if a.size == 0:
        return 0
    return int(np.max(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))))


def _table(n):
    from detail_tts_amd import _lib
    from detail_tts_amd.runtime import Runtime
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdetail_hip.so not built (run __graft_entry__.build())")
    return Runtime.dpm_schedule_table(n)


@pytest.mark.parametrize("n", [2, 7, 10, 20, 50])
def test_dpm_schedule_table_equals_reference(golden, n):
    """times and model times bit for bit (torch's fp32 linspace, t * 1000); alpha, sigma, lambda and the step scalars within MAX_ULPS"""
    g = golden("dpm_tables")
    times, mt, c = _table(n)
    assert np.array_equal(times, g[f"times_{n}"]) and times.dtype == np.float32
    assert np.array_equal(mt, g[f"model_times_{n}"])
    assert np.array_equal(c[:, 6].astype(np.int32), g[f"order_{n}"])
    assert ulps(c[:, 0], g[f"alpha_{n}"][:n]) <= MAX_ULPS
    assert ulps(c[:, 1], g[f"sigma_{n}"][:n]) <= MAX_ULPS
    assert ulps(c[:, 2], g[f"lambda_{n}"][:n]) <= MAX_ULPS
    assert ulps(c[:, 3], g[f"ratio_{n}"]) <= MAX_ULPS
    assert ulps(c[:, 4], g[f"alpha_phi1_{n}"]) <= MAX_ULPS
    second = g[f"order_{n}"] == 2
    assert ulps(c[second, 5], g[f"inv_r0_{n}"][second]) <= MAX_ULPS and np.all(c[~second, 5] == 0)


def test_dpm_schedule_orders_and_range():
    """first step first order; the last step too below 10 steps (lower_order_final); the times run from 1 to 1e-3"""
    for n in (2, 3, 9, 10, 11, 200):
        times, mt, c = _table(n)
        order = c[:, 6].astype(int).tolist()
        assert order[0] == 1 and order[-1] == (1 if n < 10 else 2) and set(order[1:-1]) <= {2}
        assert times[0] == 1.0 and times[-1] == np.float32(0.001) and np.all(np.diff(times) < 0)
        assert np.all(mt > 1.0) and mt[0] == 1000.0
    with pytest.raises(ValueError):
        _table(1)


def test_sampling_args_dpmsolver():
    from detail_tts_amd.vqvae.model_24k import sampling_args
    assert sampling_args(20, "dpmsolver++") == (20, 2, 0.0)
    assert sampling_args(None, "dpmsolver++") == (50, 2, 0.0)          # the reference's infer_diffuser: 50 steps
    assert sampling_args(4000, "dpmsolver++", 0)[0] == 4000


class _NoDevice:
    """a model whose runtime must never be touched"""
    @property
    def rt(self):
        raise AssertionError("device work before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(diffusion_steps=1), dict(diffusion_steps=4001), dict(eta=0.5), dict(diffusion_steps=2.5)])
def test_infer_dpmsolver_arguments_rejected_before_any_launch(kw):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    for fn in (SynthesizerTrn.infer, lambda self, *a, **k: next(SynthesizerTrn.infer_stream(self, [{}], **k))):
        with pytest.raises(ValueError):
            fn(_NoDevice(), None, None, None, None, sampler="dpmsolver++", **kw)


def _loop_kwargs():
    return dict(model_kwargs={"precomputed_aligned_embeddings": object()})


def test_k_diffusion_sample_loop_checks_before_device_work():
    with pytest.raises(ValueError, match="dpmsolver"):
        diffuser(1).k_diffusion_sample_loop(None, None, _NoDevice(), (1, 128, 8), **_loop_kwargs())
    with pytest.raises(ValueError, match="dpmsolver"):
        diffuser(1, sampler="dpmsolver++").sample_loop(_NoDevice(), (1, 128, 8), **_loop_kwargs())
    with pytest.raises(ValueError, match="model_kwargs"):
        diffuser(10).k_diffusion_sample_loop(None, None, _NoDevice(), (1, 128, 8), model_kwargs=None)
    with pytest.raises(ValueError, match="precomputed_aligned_embeddings"):
        diffuser(10).k_diffusion_sample_loop(None, None, _NoDevice(), (1, 128, 8), model_kwargs={})
    with pytest.raises(NotImplementedError, match="conditioning_free"):
        diffuser(10, conditioning_free=False, sampler="dpmsolver++").sample_loop(_NoDevice(), (1, 128, 8), **_loop_kwargs())
    with pytest.raises(NotImplementedError, match="cond_free_k"):
        diffuser(10, conditioning_free_k=3.0).k_diffusion_sample_loop(None, None, _NoDevice(), (1, 128, 8), **_loop_kwargs())


def test_dpm_plus_plus_2m_still_raises_and_names_the_new_key():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn, sampling_args
    with pytest.raises(NotImplementedError, match="dpmsolver\\+\\+"):
        diffuser(50, sampler="dpm++2m").sample_loop(_NoDevice(), (1, 128, 8), **_loop_kwargs())
    with pytest.raises(NotImplementedError, match="dpmsolver\\+\\+"):
        SynthesizerTrn.infer(_NoDevice(), None, None, None, None, sampler="dpm++2m")
    with pytest.raises(NotImplementedError, match="dpmsolver\\+\\+"):
        sampling_args(20, "dpm++2m")
