"""float64 numpy restatement of the flow-VAE stage forward's new pieces (TEST INFRASTRUCTURE): enc_q / PosteriorEncoder
(vqvae/model_24k.py:172-218), modules.WN at any depth (vqvae/modules/modules.py:204-229), the flow in its forward direction
(vqvae/model_24k.py:162-165, vqvae/modules/modules.py:456-471), slice_segments (vqvae/modules/commons.py:67-73) and kl_loss
(vqvae/modules/losses.py:43-58).  P is the folded weight dict (detail_tts_amd.weights.select_inference_params).

The keyword switches restate the mistakes tests/golden/make_golden_flowvae.py asserts the fixture can see; all off = the reference."""
import numpy as np

F64 = np.float64


def conv1d(x, w, b, padding=0):
    """x [B, Cin, T], w [Cout, Cin, k] -> [B, Cout, T + 2 padding - k + 1], float64"""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    k = w.shape[2]
    xp = np.pad(x, ((0, 0), (0, 0), (padding, padding)))
    n = xp.shape[2] - k + 1
    y = np.zeros((x.shape[0], w.shape[0], n), F64)
    for j in range(k):
        y += np.einsum("oc,bct->bot", w[:, :, j], xp[:, :, j:j + n])
    return y + np.asarray(b, F64)[None, :, None]


def sequence_mask(lengths, T):
    return (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(F64)[:, None, :]


def wn(P, p, x, mask, g, n_layers, hidden=192, layers_run=None, cond_mod=None):
    """modules.WN.forward: x [B, hidden, T], mask [B, 1, T], g [B, gin] -> the summed skips * mask.
    layers_run: only that many layers (the mistake "first 4 layers"); cond_mod: layer l reads the cond rows of layer l % cond_mod"""
    x = np.asarray(x, F64)
    out = np.zeros_like(x)
    G = conv1d(np.asarray(g, F64)[:, :, None], P[p + ".cond_layer.weight"], P[p + ".cond_layer.bias"])
    run = n_layers if layers_run is None else layers_run
    for i in range(run):
        a = conv1d(x, P[p + f".in_layers.{i}.weight"], P[p + f".in_layers.{i}.bias"], padding=2)
        ci = i if cond_mod is None else i % cond_mod
        a = a + G[:, ci * 2 * hidden:(ci + 1) * 2 * hidden]
        acts = np.tanh(a[:, :hidden]) / (1.0 + np.exp(-a[:, hidden:]))
        rs = conv1d(acts, P[p + f".res_skip_layers.{i}.weight"], P[p + f".res_skip_layers.{i}.bias"])
        if i < n_layers - 1:
            x = (x + rs[:, :hidden]) * mask
            out = out + rs[:, hidden:]
        else:
            out = out + rs
    return out * mask


def posterior_encoder(P, spec, lengths, g, noise, noise_scale=1.0, **wn_kw):
    """enc_q.forward -> (z, m_q, logs_q), float64"""
    T = spec.shape[2]
    mask = sequence_mask(lengths, T)
    h = conv1d(spec, P["enc_q.pre.weight"], P["enc_q.pre.bias"]) * mask
    h = wn(P, "enc_q.enc", h, mask, g, 16, **wn_kw)
    stats = conv1d(h, P["enc_q.proj.weight"], P["enc_q.proj.bias"]) * mask
    C = stats.shape[1] // 2
    m, logs = stats[:, :C], stats[:, C:]
    z = (m + np.asarray(noise, F64) * np.exp(logs) * noise_scale) * mask
    return z, m, logs


def flow_forward(P, z, lengths, g, drop_last_flip=False, no_x1_mask=False, n_flows=4):
    """ResidualCouplingBlock.forward(reverse=False): (coupling, Flip) x 4, mean_only couplings"""
    x = np.asarray(z, F64)
    mask = sequence_mask(lengths, x.shape[2])
    half = x.shape[1] // 2
    for f in range(n_flows):
        p = f"flow.flows.{2 * f}"
        x0, x1 = x[:, :half], x[:, half:]
        h = conv1d(x0, P[p + ".pre.weight"], P[p + ".pre.bias"]) * mask
        h = wn(P, p + ".enc", h, mask, g, 4)
        m = conv1d(h, P[p + ".post.weight"], P[p + ".post.bias"]) * mask
        x1 = m + (x1 if no_x1_mask else x1 * mask)
        x = np.concatenate([x0, x1], 1)
        if not (drop_last_flip and f == n_flows - 1):
            x = x[:, ::-1]
    return np.ascontiguousarray(x)


def slice_segments(x, ids, seg):
    return np.stack([x[b, :, int(i):int(i) + seg] for b, i in enumerate(ids)])


def kl_loss(z_p, logs_q, m_p, logs_p, lengths, per_channel=False):
    z_p, logs_q, m_p, logs_p = (np.asarray(a, F64) for a in (z_p, logs_q, m_p, logs_p))
    mask = sequence_mask(lengths, z_p.shape[2])
    kl = logs_p - logs_q - 0.5 + 0.5 * (z_p - m_p) ** 2 * np.exp(-2.0 * logs_p)
    den = mask.sum() * (z_p.shape[1] if per_channel else 1)
    return float((kl * mask).sum() / den)
