"""Float64 numpy restatement of the diffuser's three single-step updates - p_sample, ddim_sample and ddim_reverse_sample
(vqvae/utils/diffusion.py:445-485, 744-783, 785-817) - from (x, pred_xstart, the diffuser's float64 tables), and of p_mean_variance's
front (:284-386) from the two model outputs.  No torch, no GPU: the yardstick of tests/golden/make_golden_invert.py (the reference's own
fp32 against it is the gap no gate may go below) and of tests/test_host_invert.py.

`d` is any object with the reference's table attributes (the reference's SpacedDiffusion, or detail_tts_amd's).  The keyword switches
plant the mistakes the fixture must be able to see; all default to the reference's arithmetic."""
import numpy as np


def f64(a):
    return np.asarray(a, np.float64)


def cfk(d, t, k=2.0):
    """the ramped guidance scale of step t (:352)"""
    return k * (1.0 - t / d.num_timesteps)


def guided(cond, uncond, k):
    """(1 + cfk) cond - cfk uncond on the eps halves (:355)"""
    return (1.0 + k) * f64(cond) - k * f64(uncond)


def pred_xstart(d, x, eps, t, clamp=True):
    """_predict_xstart_from_eps (:388-393), clamped to [-1, 1] (:362)"""
    x0 = d.sqrt_recip_alphas_cumprod[t] * f64(x) - d.sqrt_recipm1_alphas_cumprod[t] * f64(eps)
    return np.clip(x0, -1.0, 1.0) if clamp else x0


def eps_from_xstart(d, x, x0, t):
    """_predict_eps_from_xstart (:402-405)"""
    return (d.sqrt_recip_alphas_cumprod[t] * f64(x) - f64(x0)) / d.sqrt_recipm1_alphas_cumprod[t]


def log_variance(d, var_values, t):
    """the learned-range log variance (:327-331)"""
    frac = (f64(var_values) + 1.0) / 2.0
    return frac * np.log(d.betas[t]) + (1.0 - frac) * d.posterior_log_variance_clipped[t]


def posterior_mean(d, x, x0, t):
    """q_posterior_mean_variance's mean (:262-282)"""
    return d.posterior_mean_coef1[t] * f64(x0) + d.posterior_mean_coef2[t] * f64(x)


def p_update(d, x, x0, log_var, t, noise=None):
    """p_sample (:480-485) from (x, pred_xstart, log_variance)"""
    out = posterior_mean(d, x, x0, t)
    if t != 0 and noise is not None:
        out = out + np.exp(0.5 * f64(log_var)) * f64(noise)
    return out


def ddim_update(d, x, x0, t, eta=0.0, noise=None):
    """ddim_sample (:773-783) from (x, pred_xstart)"""
    eps = eps_from_xstart(d, x, x0, t)
    ab, abp = d.alphas_cumprod[t], d.alphas_cumprod_prev[t]
    sigma = eta * np.sqrt((1.0 - abp) / (1.0 - ab)) * np.sqrt(1.0 - ab / abp)
    out = f64(x0) * np.sqrt(abp) + np.sqrt(1.0 - abp - sigma ** 2) * eps
    if t != 0 and noise is not None:
        out = out + sigma * f64(noise)
    return out


def reverse_update(d, x, x0, t, next_table="alphas_cumprod_next", eps=None):
    """ddim_reverse_sample (:809-815): a function of x and pred_xstart alone.  next_table: another table in the place of
    alphas_cumprod_next; eps: an eps in the place of the one re-derived from the clamped pred_xstart (planted mistakes)."""
    e = eps_from_xstart(d, x, x0, t) if eps is None else f64(eps)
    abn = getattr(d, next_table)[t]
    return f64(x0) * np.sqrt(abn) + np.sqrt(1.0 - abn) * e


MISTAKES = ("ab_t_for_next", "ab_prev_for_next", "no_clamp", "eps_of_model", "cfk_mirrored", "cond_only")


def reverse_step(d, x, cond, uncond, t, mistake=None, k=2.0):
    """ddim_reverse_sample from the two model outputs' eps halves -> (sample, pred_xstart), with one of MISTAKES planted:
    alphas_cumprod[t] / alphas_cumprod_prev[t] in the place of alphas_cumprod_next[t]; no clamp; eps taken from the guided output
    instead of re-derived from the clamped x0; the guidance scale of step n - 1 - t; the conditional output alone (no guidance)."""
    assert mistake is None or mistake in MISTAKES, mistake
    kk = cfk(d, d.num_timesteps - 1 - t if mistake == "cfk_mirrored" else t, k)
    eps = f64(cond) if mistake == "cond_only" else guided(cond, uncond, kk)
    x0 = pred_xstart(d, x, eps, t, clamp=mistake != "no_clamp")
    table = {"ab_t_for_next": "alphas_cumprod", "ab_prev_for_next": "alphas_cumprod_prev"}.get(mistake, "alphas_cumprod_next")
    return reverse_update(d, x, x0, t, table, eps if mistake == "eps_of_model" else None), x0


def mean_variance(d, x, out_cond, out_uncond, t, k=2.0):
    """p_mean_variance from the two [.., 256, T] model outputs -> dict of its four tensors"""
    C = np.asarray(x).shape[-2]
    oc, ou = f64(out_cond), f64(out_uncond)
    lv = log_variance(d, oc[..., C:, :], t)
    x0 = pred_xstart(d, x, guided(oc[..., :C, :], ou[..., :C, :], cfk(d, t, k)), t)
    return {"mean": posterior_mean(d, x, x0, t), "variance": np.exp(lv), "log_variance": lv, "pred_xstart": x0}
