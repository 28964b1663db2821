"""float64 numpy restatement of the loss arithmetic of GaussianDiffusion.training_losses for the epsilon / learned_range / mse
configuration (vqvae/utils/diffusion.py:930-1012, _vb_terms_bpd :903-928, normal_kl :17-35, discretized_gaussian_log_likelihood :38-73,
q_sample :243-260).  Test infrastructure: the yardstick of tests/test_host_diff_losses.py and tests/test_gpu_diff_losses.py, and of the
sensitivity margins tests/golden/make_golden_diff_losses.py asserts.  `d` is any object with the float64 schedule tables of
GaussianDiffusion (the reference's diffuser or detail_tts_amd's SpacedDiffusion mirror); tables may be given in fp32 (`fp32_tables`),
which is what both the reference (_extract_into_tensor casts to float) and the device use.

The keyword switches of loss_terms restate the MISTAKES the fixture must be able to see, never anything the product does."""
import numpy as np

MEL_MIN, TORCH_MEL_MAX = -11.512925465, 2.7


def normalize_mel(mel):
    return 2 * ((np.asarray(mel, np.float64) - MEL_MIN) / (TORCH_MEL_MAX - MEL_MIN)) - 1


def _table(d, name, t, fp32_tables):
    if name == "log_betas":
        a = np.log(np.asarray(d.betas, np.float64))
    else:
        a = np.asarray(getattr(d, name), np.float64)
    if fp32_tables:
        a = a.astype(np.float32).astype(np.float64)
    return a[np.asarray(t)][:, None, None]


def q_sample(d, x_start, t, noise, fp32_tables=True):
    x_start, noise = np.asarray(x_start, np.float64), np.asarray(noise, np.float64)
    return _table(d, "sqrt_alphas_cumprod", t, fp32_tables) * x_start + _table(d, "sqrt_one_minus_alphas_cumprod", t, fp32_tables) * noise


def _cdf(x):
    return 0.5 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def loss_terms(d, model_out, x_start, x_t, noise, t, fp32_tables=True, t_plus_one=False, drop_t0=False, frac_zero=False):
    """-> dict(mse [B], vb [B], loss [B], pred_xstart [B,C,T]) in float64"""
    mo, x0, xt, nz = (np.asarray(a, np.float64) for a in (model_out, x_start, x_t, noise))
    t = np.asarray(t).astype(np.int64)
    C = x0.shape[1]
    assert mo.shape == (x0.shape[0], 2 * C, x0.shape[2]) and t.shape == (x0.shape[0],)
    eps, v = mo[:, :C], mo[:, C:]
    tt = np.minimum(t + 1, len(d.betas) - 1) if t_plus_one else t
    k = lambda name: _table(d, name, tt, fp32_tables)
    pred = k("sqrt_recip_alphas_cumprod") * xt - k("sqrt_recipm1_alphas_cumprod") * eps
    x0c = np.clip(pred, -1.0, 1.0)
    mean = k("posterior_mean_coef1") * x0c + k("posterior_mean_coef2") * xt
    true_mean = k("posterior_mean_coef1") * x0 + k("posterior_mean_coef2") * xt
    min_log, max_log = k("posterior_log_variance_clipped"), k("log_betas")
    frac = np.zeros_like(v) if frac_zero else (v + 1) / 2
    logvar = frac * max_log + (1 - frac) * min_log
    kl = 0.5 * (-1.0 + logvar - min_log + np.exp(min_log - logvar) + (true_mean - mean) ** 2 * np.exp(-logvar))
    centered = x0 - mean
    inv_stdv = np.exp(-0.5 * logvar)
    cdf_plus, cdf_min = _cdf(inv_stdv * (centered + 1.0 / 255.0)), _cdf(inv_stdv * (centered - 1.0 / 255.0))
    log_probs = np.where(x0 < -0.999, np.log(np.maximum(cdf_plus, 1e-12)),
                         np.where(x0 > 0.999, np.log(np.maximum(1.0 - cdf_min, 1e-12)), np.log(np.maximum(cdf_plus - cdf_min, 1e-12))))
    flat = lambda a: a.reshape(a.shape[0], -1).mean(1)
    kl_b, nll_b = flat(kl) / np.log(2.0), flat(-log_probs) / np.log(2.0)
    vb = kl_b if drop_t0 else np.where(tt == 0, nll_b, kl_b)
    mse = flat((nz - eps) ** 2)
    return dict(mse=mse, vb=vb, loss=mse + vb, pred_xstart=pred)
