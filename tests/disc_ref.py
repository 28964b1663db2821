"""float64 numpy restatement of MultiPeriodDiscriminator.forward (reference: vqvae/model_24k.py:298-431) and of feature_loss /
discriminator_loss / generator_loss (vqvae/modules/losses.py:4-40), on the FOLDED weights (weights.select_discriminator_params).
tests/golden/make_golden_disc.py checks it against the reference's own numbers before it trusts it; tests/test_host_disc.py repeats
that check against the fixture.  The keyword arguments are the mistakes the fixture must be able to see."""
import numpy as np

PERIODS = (2, 3, 5, 7, 11)
S_CONVS = ((1, 7, 1), (4, 20, 4), (4, 20, 16), (4, 20, 64), (4, 20, 256), (1, 2, 1))      # (stride, pad, groups) of DiscriminatorS convs.0 .. 5
P_STRIDES = (3, 3, 3, 3, 1)


def conv1d(x, w, b, stride=1, pad=0, groups=1, group_of=None):
    """x [R, Cin, T], w [Cout, Cin / groups, K] -> [R, Cout, (T + 2 pad - K) // stride + 1]; group_of(g): the input group output
    group g reads (None: g)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    R, Cin, T = x.shape
    Cout, cg, K = w.shape
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad)))
    nout = (T + 2 * pad - K) // stride + 1
    win = np.lib.stride_tricks.sliding_window_view(xp, K, axis=2)[:, :, ::stride][:, :, :nout]      # [R, Cin, nout, K]
    og = Cout // groups
    out = np.empty((R, Cout, nout), np.float64)
    for g in range(groups):
        gi = g if group_of is None else group_of(g)
        a = win[:, gi * cg:(gi + 1) * cg].transpose(0, 2, 1, 3).reshape(R, nout, cg * K)
        out[:, g * og:(g + 1) * og] = (a @ w[g * og:(g + 1) * og].reshape(og, cg * K).T).transpose(0, 2, 1)
    return out + np.asarray(b, np.float64)[None, :, None]


def lrelu(x, slope=0.1):
    return np.where(x >= 0, x, x * slope)


def period_split(x, p, pad_mode="reflect", left=False):
    """x [B, 1, t] -> [B, 1, H, p]: right-pad by p - t % p (reflect) when t % p != 0, then view"""
    x = np.asarray(x)
    B, _, t = x.shape
    if t % p:
        n = p - t % p
        x = np.pad(x, ((0, 0), (0, 0), (n, 0) if left else (0, n)), mode=pad_mode)
    return x.reshape(B, 1, -1, p)


def disc_s(P, x, slope=0.1, stride=4, group_of=None):
    """DiscriminatorS -> (score [B, T'], maps: 7 x [B, C, T])"""
    pre, fmap = "discriminators.0.", []
    x = np.asarray(x, np.float64)
    for i, (s, pad, g) in enumerate(S_CONVS):
        x = lrelu(conv1d(x, P[f"{pre}convs.{i}.weight"], P[f"{pre}convs.{i}.bias"], stride if s == 4 else s, pad, g, group_of if g > 1 else None), slope)
        fmap.append(x)
    x = conv1d(x, P[pre + "conv_post.weight"], P[pre + "conv_post.bias"], 1, 1)
    fmap.append(x)
    return x.reshape(x.shape[0], -1), fmap


def disc_p(P, d, x, slope=0.1, pad_mode="reflect", left=False, flatten_ph=False):
    """DiscriminatorP number d (1 .. 5) -> (score [B, H p], maps: 6 x [B, C, H, p])"""
    p, pre, fmap = PERIODS[d - 1], f"discriminators.{d}.", []
    x4 = period_split(x, p, pad_mode, left).astype(np.float64)
    B, _, H, _ = x4.shape
    rows = x4.transpose(0, 3, 1, 2).reshape(B * p, 1, H)                     # (K, 1) convs: every column w is a row of its own

    def back(r):
        return r.reshape(B, p, r.shape[1], r.shape[2]).transpose(0, 2, 3, 1)

    for i, s in enumerate(P_STRIDES):
        rows = lrelu(conv1d(rows, P[f"{pre}convs.{i}.weight"][..., 0], P[f"{pre}convs.{i}.bias"], s, 2), slope)
        fmap.append(back(rows))
    rows = conv1d(rows, P[pre + "conv_post.weight"][..., 0], P[pre + "conv_post.bias"], 1, 1)
    fmap.append(back(rows))
    last = fmap[-1]
    score = (last.transpose(0, 1, 3, 2) if flatten_ph else last).reshape(B, -1)
    return score, fmap


def mpd(P, y, y_hat, s_kw=None, p_kw=None):
    """MultiPeriodDiscriminator.forward -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs)"""
    s_kw, p_kw = s_kw or {}, p_kw or {}
    out = ([], [], [], [])
    for d in range(6):
        for side, x in ((0, y), (1, y_hat)):
            sc, fm = disc_s(P, x, **s_kw) if d == 0 else disc_p(P, d, x, **p_kw)
            out[side].append(sc)
            out[2 + side].append(fm)
    return out


def map_means(fmap_r, fmap_g, per_row=False):
    """mean |r - g| of every map, in list order (37); per_row: the mean of the rows' means of |r - g| summed over everything but rows
    (a mistake)"""
    out = []
    for dr, dg in zip(fmap_r, fmap_g):
        for r, g in zip(dr, dg):
            a = np.abs(np.asarray(r, np.float64) - np.asarray(g, np.float64))
            out.append(a.reshape(a.shape[0], -1).sum(1).mean() if per_row else a.mean())
    return np.array(out)


def feature_loss(fmap_r, fmap_g, factor=2.0, skip_post=False):
    m = map_means(fmap_r, fmap_g)
    if skip_post:
        keep, k = [], 0
        for dr in fmap_r:
            keep += list(range(k, k + len(dr) - 1))
            k += len(dr)
        m = m[keep]
    return float(m.sum() * factor)


def discriminator_loss(drs, dgs):
    r = [float(np.mean((1 - np.asarray(a, np.float64)) ** 2)) for a in drs]
    g = [float(np.mean(np.asarray(a, np.float64) ** 2)) for a in dgs]
    return sum(a + b for a, b in zip(r, g)), r, g


def generator_loss(dgs):
    l = [float(np.mean((1 - np.asarray(a, np.float64)) ** 2)) for a in dgs]
    return sum(l), l


def spec_to_mel(spec, basis):
    return np.log(np.maximum(np.asarray(basis, np.float64) @ np.asarray(spec, np.float64), 1e-5))
