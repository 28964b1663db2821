"""CPU: the host side of DDIM inversion and partial-depth resampling - the float64 restatement (tests/ddim_ref.py) against the
reference's stored steps (ddim_reverse.npz), the host-only coefficient table (dtts_ddim_reverse_table) against the reference's float64
tables (sampler_tables.npz), every refusal before any launch, the depth / t_start pairing, the fixture's checksums."""
import os

import numpy as np
import pytest

import ddim_ref as DR
import invert_inputs as II
from diff_loss_inputs import checksum


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def _diffuser(n=II.N_STEPS, sampler="ddim", **kw):
    from detail_tts_amd.vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    kw.setdefault("conditioning_free", True)
    return SpacedDiffusion(space_timesteps(4000, n if isinstance(n, str) else [n]), betas=get_named_beta_schedule("linear", 4000),
                           conditioning_free_k=2.0, sampler=sampler, **kw)


@pytest.fixture(scope="module")
def S(golden):
    return golden("sampler_chains")


@pytest.fixture(scope="module")
def R(golden):
    return golden("ddim_reverse")


def test_fixture_checksums_and_shape(S, R):
    for k in ("code_emb", "ddim0_final", "ddim0_x_init", "p_x_before_9", "p_x_before_0"):
        assert np.array_equal(checksum(S[k]), R["f64_sum_" + k]), k
    assert int(R["ch_stride"]) == II.CH_STRIDE and int(R["pmv_ch_stride"]) == II.PMV_CH_STRIDE
    assert R["chain_x"].shape == (II.N_STEPS, 128 // II.CH_STRIDE, 48) and R["chain_x0"].shape == (len(II.STEPS), 128 // II.CH_STRIDE, 48)
    assert float(R["rt_miss"]) > 0.5                                  # the reference's round trip is not the identity
    # both clamp branches at steps 0 and 4
    for j, t in enumerate(II.STEPS[:2]):
        share = float(np.mean(np.abs(R["chain_x0"][j]) == 1.0))
        assert 0.1 <= share <= 0.9, (t, share)
    # the gates respect the reference's own fp32-against-float64 gap
    for t in II.STEPS:
        assert II.STEP_SAMPLE_GATE[t] >= R["f64_gap"][t], t


def test_restatement_reproduces_the_stored_steps(S, R):
    """reverse_update from the stored x and pred_xstart alone gives every stored `sample` within the gap the fixture script printed;
    the posterior mean of p_mean_variance likewise from its x and pred_xstart"""
    d = _diffuser()
    for j, t in enumerate(II.STEPS):
        x = S["ddim0_final"] if t == 0 else R[f"rev_x_before_{t}"]
        got = DR.reverse_update(d, II.sub(x), R["chain_x0"][j], t)
        e = maxabs(got, R["chain_x"][t])
        assert e <= R["f64_gap"][t], (t, e, R["f64_gap"][t])
    for t in II.PMV_STEPS:
        x = II.sub(S[f"p_x_before_{t}"], II.PMV_CH_STRIDE)
        assert maxabs(DR.posterior_mean(d, x, R[f"pmv_{t}_pred_xstart"], t), R[f"pmv_{t}_mean"]) < 1e-6, t
        assert maxabs(np.exp(R[f"pmv_{t}_log_variance"].astype(np.float64)), R[f"pmv_{t}_variance"]) < 1e-6, t
    # the sampling updates from (x, pred_xstart): sampler_chains' eta = 0 DDIM steps and the noise-free last ancestral step
    for i in (9, 8, 0):
        got = DR.ddim_update(d, S[f"ddim0_x_before_{i}"], S[f"ddim0_x0_{i}"], i)
        assert maxabs(got, S[f"ddim0_x_after_{i}"]) < 2e-5, i
    lv = np.zeros_like(S["p_x0_0"])
    assert maxabs(DR.p_update(d, S["p_x_before_0"], S["p_x0_0"], lv, 0), S["p_x_after_0"]) < 2e-6


def test_planted_mistakes_move_the_update():
    """every switch of ddim_ref.reverse_step changes its result (the fixture script measures by how much on the reference's outputs)"""
    d = _diffuser()
    rs = np.random.RandomState(3)
    x, c, u = rs.randn(1, 8, 16) * 0.7, rs.randn(1, 8, 16), rs.randn(1, 8, 16)
    for t in (0, 4):
        right, x0 = DR.reverse_step(d, x, c, u, t)
        assert np.abs(x0).max() == 1.0 and np.abs(x0).min() < 1.0
        assert maxabs(DR.reverse_update(d, x, x0, t), right) == 0.0
        for mk in DR.MISTAKES:
            assert maxabs(DR.reverse_step(d, x, c, u, t, mk)[0], right) > 1e-3, (t, mk)


@pytest.mark.parametrize("key", ["10", "25", "200", "ddim25"])
def test_ddim_reverse_table_equals_reference_tables(golden, key):
    """dtts_ddim_reverse_table (host only) against the reference's float64 tables after the reference's cast order: _extract_into_tensor
    casts to fp32, then sqrt and 1 - . run in fp32.  atol 0."""
    from detail_tts_amd.runtime import Runtime
    T = golden("sampler_tables")
    tmap = T[f"tmap_{key}"]
    n = len(tmap)
    c = Runtime.ddim_reverse_table(tmap)
    assert c.shape == (n, 6) and c.dtype == np.float32
    nxt = T[f"f64_{key}_alphas_cumprod_next"].astype(np.float32)
    assert nxt[-1] == 0.0
    np.testing.assert_array_equal(c[:, 0], nxt)
    np.testing.assert_array_equal(c[:, 1], T[f"f64_{key}_sqrt_recip_alphas_cumprod"].astype(np.float32))
    np.testing.assert_array_equal(c[:, 2], T[f"f64_{key}_sqrt_recipm1_alphas_cumprod"].astype(np.float32))
    np.testing.assert_array_equal(c[:, 3], np.sqrt(nxt))
    np.testing.assert_array_equal(c[:, 4], np.sqrt(np.float32(1.0) - nxt))
    assert c[-1, 3] == 0.0 and c[-1, 4] == 1.0                      # the last step ends at alphas_cumprod_next = 0: pure eps'
    np.testing.assert_array_equal(c[:, 5], (2.0 * (1.0 - np.arange(n) / n)).astype(np.float32))
    # the mirror's own float64 table is the reference's
    np.testing.assert_array_equal(_diffuser(key if key == "ddim25" else int(key)).alphas_cumprod_next, T[f"f64_{key}_alphas_cumprod_next"])


class _NoLaunch:
    def __getattr__(self, name):
        raise AssertionError(f"the runtime was reached ({name}): a refusal must come before any launch")


class _Model:
    rt = _NoLaunch()


X = np.zeros((2, 128, 8), np.float32)
KW = {"precomputed_aligned_embeddings": np.zeros((2, 768, 8), np.float32)}
T3 = np.array([3, 3])


def test_pairing_of_depth_and_t_start():
    d = _diffuser()
    assert d.invert_depth(None) == (10, None) and d.invert_depth(10) == (10, None)
    for depth in range(1, 10):
        assert d.invert_depth(depth) == (depth, depth) and II.pairing(10, depth) == depth
    assert II.pairing(10, 10) is None
    for bad in (0, 11, -1, True, 2.5, "5"):
        with pytest.raises(ValueError):
            d.invert_depth(bad)
        with pytest.raises(ValueError):
            d.ddim_reverse_sample_loop(_Model(), X, KW, depth=bad)
    # step index t of the inversion reads alphas_cumprod_next[t] = alphas_cumprod[t + 1]: depth d ends at the level t_start = d starts from
    np.testing.assert_array_equal(d.alphas_cumprod_next[:-1], d.alphas_cumprod[1:])
    np.testing.assert_array_equal(d.alphas_cumprod_prev[1:], d.alphas_cumprod[:-1])


def test_refusals_come_before_any_launch():
    d, m = _diffuser(), _Model()
    with pytest.raises(ValueError, match="Reverse ODE only for deterministic path"):
        d.ddim_reverse_sample(m, X, T3, model_kwargs=KW, eta=0.5)
    steps = (d.ddim_reverse_sample, d.p_mean_variance, d.p_sample, d.ddim_sample)
    for fn in steps:
        with pytest.raises(ValueError, match="clip_denoised"):
            fn(m, X, T3, clip_denoised=False, model_kwargs=KW)
        with pytest.raises(ValueError, match="denoised_fn"):
            fn(m, X, T3, denoised_fn=lambda x: x, model_kwargs=KW)
        with pytest.raises(ValueError, match="same t"):
            fn(m, X, np.array([3, 4]), model_kwargs=KW)
        for bad in (np.array([10, 10]), np.array([-1, -1]), np.array([3]), np.array([2.5, 2.5])):
            with pytest.raises(ValueError):
                fn(m, X, bad, model_kwargs=KW)
        with pytest.raises(ValueError, match="precomputed_aligned_embeddings"):
            fn(m, X, T3)
    for fn in (d.p_sample, d.ddim_sample):
        with pytest.raises(ValueError, match="cond_fn"):
            fn(m, X, T3, cond_fn=lambda *a, **k: 0, model_kwargs=KW)
    with pytest.raises(ValueError):
        d.ddim_sample(m, X, T3, model_kwargs=KW, eta=-0.1)
    for gen in (d.p_sample_loop_progressive, d.ddim_sample_loop_progressive):
        with pytest.raises(ValueError, match="cond_fn"):
            next(gen(m, X.shape, noise=X, cond_fn=lambda *a, **k: 0, model_kwargs=KW))
        with pytest.raises(ValueError, match="noise"):
            next(gen(m, X.shape, model_kwargs=KW))
    # t_start
    for loop in (d.p_sample_loop, d.ddim_sample_loop):
        for bad in (10, -1, True, 2.5):
            with pytest.raises(ValueError, match="t_start"):
                loop(m, X.shape, noise=X, model_kwargs=KW, t_start=bad)
        with pytest.raises(ValueError, match="noise"):
            loop(m, X.shape, model_kwargs=KW, t_start=5)
        with pytest.raises(ValueError, match="precomputed_aligned_embeddings"):
            loop(m, X.shape, noise=X, t_start=5)
    with pytest.raises(ValueError, match="eta"):
        d.ddim_sample_loop(m, X.shape, noise=X, model_kwargs=KW, t_start=5, eta=-1.0)
    dp = _diffuser(sampler="dpmsolver++")
    with pytest.raises(ValueError, match="dpmsolver"):
        dp.k_diffusion_sample_loop(None, None, m, X.shape, noise=X, model_kwargs=KW, t_start=5)
    with pytest.raises(ValueError, match="dpmsolver"):
        dp.sample_loop(m, X.shape, noise=X, model_kwargs=KW, t_start=5)
    # today's _check refusals, unchanged, on every new entry
    for bad, exc in ((_diffuser(conditioning_free=False), NotImplementedError), (_diffuser(rescale_timesteps=True), NotImplementedError)):
        for fn in (bad.ddim_reverse_sample, bad.p_mean_variance, bad.p_sample, bad.ddim_sample):
            with pytest.raises(exc):
                fn(m, X, T3, model_kwargs=KW)
        with pytest.raises(exc):
            bad.ddim_reverse_sample_loop(m, X, KW)
        with pytest.raises(exc):
            bad.ddim_sample_loop(m, X.shape, noise=X, model_kwargs=KW, t_start=5)


def test_new_entries_are_exported():
    from detail_tts_amd import _lib
    for name in ("dtts_diff_invert", "dtts_diff_sample_from", "dtts_diff_reverse_step", "dtts_diff_mean_variance", "dtts_ddim_reverse_table"):
        assert name in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "detail_hip.h")).read()
    for name in ("dtts_diff_invert", "dtts_diff_sample_from", "dtts_diff_reverse_step", "dtts_diff_mean_variance", "dtts_ddim_reverse_table"):
        assert f"int {name}(" in header
