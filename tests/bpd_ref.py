"""float64 numpy restatement of GaussianDiffusion.calc_bpd_loop's arithmetic around a given model output
(vqvae/utils/diffusion.py:1114-1169, _vb_terms_bpd :903-928, _prior_bpd :1098-1112, _predict_eps_from_xstart :402-405).  Test
infrastructure: the yardstick of tests/test_host_bpd.py and tests/test_gpu_bpd.py, and of the sensitivity margins
tests/golden/make_golden_bpd.py asserts.  `d` is any object with the float64 schedule tables of GaussianDiffusion.  The vb term is
diff_loss_ref.loss_terms' (the same lines of the reference).

The keyword switches restate the MISTAKES the fixture must be able to see, never anything the product does."""
import numpy as np

import diff_loss_ref as DR


def terms(d, model_out, x_start, x_t, noise, t, fp32_tables=True, unclamped=False, mse_of_model_eps=False, drop_t0=False, t_plus_one=False):
    """one timestep per row -> dict(vb, xstart_mse, mse: [R]; pred_xstart [R,C,T], clamped) in float64"""
    r = DR.loss_terms(d, model_out, x_start, x_t, noise, t, fp32_tables=fp32_tables, drop_t0=drop_t0, t_plus_one=t_plus_one)
    x0, xt, nz = (np.asarray(a, np.float64) for a in (x_start, x_t, noise))
    t = np.asarray(t).astype(np.int64)
    tt = np.minimum(t + 1, len(d.betas) - 1) if t_plus_one else t
    pred = r["pred_xstart"] if unclamped else np.clip(r["pred_xstart"], -1.0, 1.0)
    flat = lambda a: a.reshape(a.shape[0], -1).mean(1)
    eps = (DR._table(d, "sqrt_recip_alphas_cumprod", tt, fp32_tables) * xt - pred) / DR._table(d, "sqrt_recipm1_alphas_cumprod", tt, fp32_tables)
    if mse_of_model_eps:
        eps = np.asarray(model_out, np.float64)[:, : x0.shape[1]]
    return dict(vb=r["vb"], xstart_mse=flat((pred - x0) ** 2), mse=flat((eps - nz) ** 2), pred_xstart=pred)


def prior_bpd(d, x_start, fp32_tables=True):
    x0 = np.asarray(x_start, np.float64)
    last = [len(d.betas) - 1] * x0.shape[0]
    mean = DR._table(d, "sqrt_alphas_cumprod", last, fp32_tables) * x0
    lv = DR._table(d, "log_one_minus_alphas_cumprod", last, fp32_tables)
    kl = 0.5 * (-1.0 - lv + np.exp(lv) + mean ** 2)
    return kl.reshape(kl.shape[0], -1).mean(1) / np.log(2.0)


def loop(d, model_outs, x_start, noise, **mistakes):
    """the whole loop on recorded model outputs: model_outs[t] [B,2C,T] and noise[t] [B,C,T] for every timestep t ->
    dict(vb, xstart_mse, mse: [B, S] with column j = timestep S - 1 - j; prior_bpd, total_bpd: [B]) in float64"""
    S, B = len(d.betas), np.asarray(x_start).shape[0]
    cols = {k: [] for k in ("vb", "xstart_mse", "mse")}
    for t in range(S - 1, -1, -1):
        tb = [t] * B
        r = terms(d, model_outs[t], x_start, DR.q_sample(d, x_start, tb, noise[t]), noise[t], tb, **mistakes)
        for k in cols:
            cols[k].append(r[k])
    out = {k: np.stack(v, 1) for k, v in cols.items()}
    out["prior_bpd"] = prior_bpd(d, x_start)
    out["total_bpd"] = out["vb"].sum(1) + out["prior_bpd"]
    return out
