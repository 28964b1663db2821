"""The exact-fp32 flash attention (csrc/attention.hip: flash_attn_kernel<D, MODE>, vits_rel_key_kernel, vits_rel_value_kernel) in numpy.
Shared by tests/test_gpu_attn_f32.py (through Runtime.op_attention / Runtime.op_attention_rel) and tests/test_host_attn_f32.py:
  * float64 references of every mode, written from the formula in the header comment of attention.hip:
        out[h D + c, t] = sum_{s < len} softmax_s(scale q_t . k_s + extra(h, t, s)) v[c, s]
    extra = tab[h][clamp(s - t, -64, 64) + 64] (bias), -inf at s > t (causal), band[h, t, s - t + W] inside |s - t| <= W (band);
  * rel_reference(): the reference's windowed relative-position attention (vqvae/modules/attentions.py MultiHeadAttention.attention,
    window_size = W) restated from its PYTHON - pad / slice the embeddings, pad / reshape / slice the logits ("skew") - not from the
    kernels' band formulation: that restatement (rel_key -> band -> rel_value) is the thing under test;
  * MUTATIONS: placement errors applied to the float64 reference (the arithmetic is exact fp32, so there is no scheme to emulate), each
    case lists the ones it claims to catch and test_host_attn_f32.py holds every claim at >= 3 x the gate;
  * the case table and its planted data.

The kernel's constants, from which the shapes below are chosen: 128 queries per workgroup (QPB), 32 per wave (QPW), 64-key LDS tiles
(KT), two LDS buffers with a register prefetch for D <= 96 (tile kt in buffer kt & 1: the third tile is the first to reuse buffer 0) and
one buffer for D = 192, the bias offset clipped to +-64 (CLIP), the causal key loop cut at min(len, q0 + 128) (klimit), a 1-D grid
remapped over the 8 XCDs.  So: lengths on and beside 32 / 64 / 128; 129 or more for a second query block, a third tile and a cut key
loop; T between 130 and 400; H x query blocks > 8 workgroups for the remap.

The four production call sites, at the default config (config.py), give the (D, mode) pairs below - PRODUCTION:
    gpt      Model::gpt_forward (model_gpt.hip)          D = 768 / 16 = 48, causal, blocks [Q | K | V], head stride D
    enc_p    Model::enc_p_fwd (model_vocoder.hip)        D = 192 / 4 = 48, band W = 4 + ml_out, blocks, head stride D
    style    Model::mel_style (model_vocoder.hip)        D = 128 / 2 = 64 (ref_enc, vq_ref_enc) and 384 / 2 = 192 (gpt conditioning
                                                         encoder), plain, blocks, head stride D, scale 1 / sqrt(hidden)
    trunk    attention_block (model_diffusion.hip)       D = 768 / 16 = 48, bias table, per head [q | k | v], head stride 3 D, cs = Ta > T
"""
import zlib

import numpy as np

KT, QPW, QPB, CLIP = 64, 32, 128, 64
DIMS = (48, 64, 96, 192)
MODES = ("plain", "bias", "causal", "band")
PRODUCTION = {"gpt": (48, "causal"), "enc_p": (48, "band"), "style64": (64, "plain"), "style192": (192, "plain"), "trunk": (48, "bias")}

# The gates, per data kind, in the metric rel_err: ~20 x the worst figure of profiles/attn_f32_measured_errors.txt (MI355X), and none above
# GATE_CAP = 2e-5, the gate the split-precision kernel meets.  The pointer kinds and std 0.6 take their 20 x.  At score std >= 2 and on
# the ramp the kernel measures 1.6 - 2.0e-6, so 20 x would pass the cap; those gates stay AT the cap, 10 x the measurement.  That level is
# fp32's own, not a defect: a plain fp32 restatement of the formula on the same data - q pre-scaled by scale log2(e), QK^T accumulated in
# fp32 four channels at a time, exp2, P V and the denominator accumulated in fp32 - lands at 0.8 - 1.1e-6 against float64 (scores of
# 8 .. 35 nats: the accumulator's ulp near 2^4 .. 2^5 in the log2 domain is 1 - 2e-6, and it enters every weight relatively); the
# hardware exp2 and the per-tile rescale of O and l make up the rest.
GATE_CAP = 2e-5
KINDS = ("bias_ptr", "band_ptr", "score_ptr", "prec", "ramp")
GATES = {"bias_ptr": 2.5e-6, "band_ptr": 2e-6, "score_ptr": 5.5e-6, "prec_std0.6": 1.2e-5, "prec_std2": 2e-5, "prec_std5": 2e-5, "ramp": 2e-5}
LSE_GATE = 1.4e-5        # ml[0] + log(ml[1]) against the float64 log-sum-exp, same metric (measured 6.9e-7)


def gate_key(c):
    return f"prec_std{c['std']:g}" if c["kind"] == "prec" else c["kind"]


def gate(c):
    return GATES[gate_key(c)]


def rel_err(y, ref):
    """the metric of the gates: max |y - ref| / max(1, max |ref|)"""
    return float(np.max(np.abs(y - ref))) / max(1.0, float(np.max(np.abs(ref)))) if ref.size else 0.0


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


# ---- layouts
def layout_args(layout, H, D):
    """-> (q_off, k_off, v_off, head_stride) of the 3 H D rows"""
    return (0, D, 2 * D, 3 * D) if layout == "head" else (0, H * D, 2 * H * D, D)


def pack_rows(q, k, v, layout, cs, lens):
    """q, k, v [B, H, D, T] -> qkv [B, 3 H D, cs] fp32 in the layout; every column >= len (the tail [T, cs) included) is NaN"""
    B, H, D, T = q.shape
    out = np.full((B, 3 * H * D, cs), np.nan, np.float32)
    view = out.reshape(B, H, 3, D, cs) if layout == "head" else out.reshape(B, 3, H, D, cs).transpose(0, 2, 1, 3, 4)
    for i, a in enumerate((q, k, v)):
        view[:, :, i, :, :T] = a
    for bi, L in enumerate(lens):
        out[bi, :, L:] = np.nan
    return out


# ---- float64 references
def bias_index(L, Lk=None, lo=-CLIP, hi=CLIP, shift=0):
    t, s = np.arange(L), np.arange(L if Lk is None else Lk)
    return np.clip(s[None, :] - t[:, None] + shift, lo, hi) + CLIP           # [t, s]


def band_matrix(band, L, W, Lk=None, shift=0, w_used=None):
    """band [H, L, 2 W + 1] -> additive [H, L, Lk]: band[h, t, s - t + W + shift] where |s - t| <= w_used and the index exists"""
    Lk = L if Lk is None else Lk
    w_used = W if w_used is None else w_used
    t, s = np.arange(L)[:, None], np.arange(Lk)[None, :]
    r = s - t + W + shift
    ok = (np.abs(s - t) <= w_used) & (r >= 0) & (r <= 2 * W)
    return np.where(ok[None], band[:, t, np.clip(r, 0, 2 * W)], 0.0)


MUTATIONS = ("mask_last", "admit_len", "causal_ge", "causal_t1", "bias_off1", "clamp63", "band_off1", "band_w_1", "band_pad_query", "v_swap",
             "head_k", "stale_tile", "skip_rescale", "relv_wrong_l")
# band_pad_query - the band added without the kernel's `t < len` condition - reaches only the score column of a query t >= len: a lane's
# scores, running maximum, denominator and its column of the PV product belong to that one query, and nothing of a query >= len is stored.
# No output at t < len can show it (test_host_attn_f32.py asserts exactly that on every band case), so no case can claim it; what the
# condition buys is that band rows >= len - uninitialised in enc_p - are never READ.
NO_OUTPUT_EFFECT = ("band_pad_query",)


def scores64(c, q, k, L, tab=None, band=None, mut=None):
    """-> (scores [H, Lq, Lk] float64 with -inf at masked keys, key count Lk).  q, k [H, D, >= L] float64 of ONE sample.  Lq = L, except
    under band_pad_query: the queries of the last active wave up to the next multiple of 32 ride along as the kernel runs them - q clamped
    to column len - 1, band rows as the data holds them (NaN) - and the caller drops them again."""
    H = q.shape[0]
    Lq = min(-(-L // QPW) * QPW, c["T"]) if mut == "band_pad_query" else L
    q = q[:, :, np.minimum(np.arange(Lq), L - 1)]
    kk = k[:, :, :L]
    if mut == "head_k":
        kk = np.roll(kk, -1, axis=0)                                           # head h reads head h + 1's K
    if mut == "stale_tile":
        kk = kk.copy()
        kk[:, :, 2 * KT:] = k[:, :, :L][:, :, :max(L - 2 * KT, 0)]             # tile kt >= 2 holds tile kt - 2's K
    Lk = L
    if mut == "admit_len":                                                     # key `len`: the clamped load gives K[len - 1], V = 0
        kk = np.concatenate([kk, kk[:, :, -1:]], axis=2)
        Lk = L + 1
    s = c["scale"] * np.einsum("hct,hcs->hts", q, kk)
    mode, W = c["mode"], c["W"]
    t, sk = np.arange(Lq)[:, None], np.arange(Lk)[None, :]
    if mode == "bias":
        hi = 63 if mut == "clamp63" else CLIP
        s = s + np.asarray(tab, np.float64)[:, bias_index(Lq, Lk, -hi, hi, 1 if mut == "bias_off1" else 0)]
    if mode == "band":
        b = np.asarray(band, np.float64)[:, :Lq]
        s = s + band_matrix(b, Lq, W, Lk, 1 if mut == "band_off1" else 0, W - 1 if mut == "band_w_1" else W)
    if mode == "causal":
        dead = (sk >= t) if mut == "causal_ge" else (sk > t + 1) if mut == "causal_t1" else (sk > t)
        s = np.where(dead[None], -np.inf, s)
    if mut == "mask_last" and L > 1:
        s[:, :, L - 1] = -np.inf
    return s, Lk


def softmax_pv(s, v, mut=None):
    """scores [H, L, Lk], v [H, D, Lk] -> (out [H, D, L], lse [H, L], p [H, L, Lk]); a wholly masked row gives zeros.  skip_rescale: the
    tile-by-tile running form with the rescale of O and l skipped once, after tile 0."""
    H, L, Lk = s.shape
    if mut == "skip_rescale":
        O, l, m = np.zeros((H, L, v.shape[1])), np.zeros((H, L)), np.full((H, L), -np.inf)
        for kt in range(-(-Lk // KT)):
            st = s[:, :, kt * KT: (kt + 1) * KT]
            m_new = np.maximum(m, st.max(-1))
            m_use = np.where(np.isfinite(m_new), m_new, 0.0)
            alpha = np.exp(m - m_use) if kt != 1 else np.ones_like(m)
            e = np.exp(st - m_use[:, :, None])
            l = l * alpha + e.sum(-1)
            O = O * alpha[:, :, None] + np.einsum("hts,hcs->htc", e, v[:, :, kt * KT: (kt + 1) * KT])
            m = m_new
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.where(l[:, :, None] > 0, O / l[:, :, None], 0.0)
            return out.transpose(0, 2, 1), m + np.log(l), None
    m = s.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(l > 0, e / l, 0.0)
        lse = (m + np.log(l))[:, :, 0]
    return np.einsum("hts,hcs->hct", p, v), lse, p


def swap_col(L):
    """v_swap exchanges V columns s, s + 1 (L > 1)"""
    return min(L - 2, (L // 2) // KT * KT + 36) // 2 * 2


def mutate_v(v, L, mut):
    v = v[:, :, :L]
    if mut == "v_swap" and L > 1:
        s = swap_col(L)
        v = v.copy()
        v[:, :, [s, s + 1]] = v[:, :, [s + 1, s]]
    if mut == "admit_len":
        v = np.concatenate([v, np.zeros_like(v[:, :, :1])], axis=2)
    return v


def reference(c, d, bi, mut=None):
    """the flash kernel's formula (and, for a rel case, the kernels' band formulation) for sample bi -> (out [H D, len], lse [H, len]) in
    float64; mut: one of MUTATIONS.  For a rel case with mut = None, test_host_attn_f32.py holds this equal to rel_reference()."""
    assert mut is None or mut in MUTATIONS
    L = d["lens"][bi]
    q, k, v = (np.asarray(d[n][bi], np.float64) for n in ("q", "k", "v"))
    H, D = q.shape[:2]
    if L == 0:
        return np.zeros((H * D, 0)), np.zeros((H, 0))
    band = d.get("band")
    if c["entry"] == "rel":                                                   # relk[h, t, r] = scale q_t . ek[r]
        band = c["scale"] * np.einsum("hct,rc->htr", q[:, :, :L], np.asarray(d["ek"], np.float64))
    elif band is not None:
        band = band[bi]
    if mut == "band_pad_query" and c["entry"] == "rel":                       # rel_key writes t < len only; the entry hands relk over as NaN
        band = np.concatenate([band, np.full((H, c["T"] - L, band.shape[2]), np.nan)], axis=1)
    s, Lk = scores64(c, q, k, L, d.get("tab"), band, mut)
    with np.errstate(invalid="ignore"):
        out, lse, p = softmax_pv(s, mutate_v(v, L, mut), mut)
    out, lse = out[:, :, :L], lse[:, :L]
    if c["entry"] == "rel":                                                   # out[h, c, t] += sum_r p(t, t + r - W) ev[r][c], from (m, l)
        W = c["W"]
        strue, _ = scores64(c, q, k, L, None, band, None)
        m = strue.max(-1)
        l = np.exp(strue - m[:, :, None]).sum(-1)
        if mut == "relv_wrong_l":
            l = np.roll(l, -1, axis=1)                                          # query t normalised by l of query t + 1
        t = np.arange(L)
        ev = np.asarray(d["ev"], np.float64)
        for r in range(2 * W + 1):
            sk = t + r - W
            ok = (sk >= 0) & (sk < L)
            pr = np.where(ok[None], np.exp(strue[:, t, np.clip(sk, 0, L - 1)] - m) / l, 0.0)      # [H, L]
            out = out + pr[:, None, :] * ev[r][None, :, None]
    return out.reshape(H * D, L), lse


# ---- the reference's relative-position attention, from its Python (vqvae/modules/attentions.py:208-303)
def _get_relative_embeddings(emb, length, W):
    """emb [1, 2 W + 1, D] -> [1, 2 length - 1, D]: pad first, then slice"""
    pad_length = max(length - (W + 1), 0)
    start = max((W + 1) - length, 0)
    end = start + 2 * length - 1
    if pad_length > 0:
        emb = np.pad(emb, [[0, 0], [pad_length, pad_length], [0, 0]])
    return emb[:, start:end]


def _relative_position_to_absolute_position(x):
    """[h, l, 2 l - 1] -> [h, l, l]"""
    h, length, _ = x.shape
    x = np.pad(x, [[0, 0], [0, 0], [0, 1]])
    x_flat = np.pad(x.reshape(h, length * 2 * length), [[0, 0], [0, length - 1]])
    return x_flat.reshape(h, length + 1, 2 * length - 1)[:, :length, length - 1:]


def _absolute_position_to_relative_position(x):
    """[h, l, l] -> [h, l, 2 l - 1]"""
    h, length, _ = x.shape
    x = np.pad(x, [[0, 0], [0, 0], [0, length - 1]])
    x_flat = np.pad(x.reshape(h, length ** 2 + length * (length - 1)), [[0, 0], [length, 0]])
    return x_flat.reshape(h, length, 2 * length)[:, :, 1:]


def rel_reference(c, d, bi):
    """MultiHeadAttention.attention on sample bi cut to its length (the reference masks keys >= len with -1e4, whose softmax weight is 0
    to every digit, and a masked query is no output) -> out [H D, len] float64.  heads_share: one embedding for all heads."""
    L, W = d["lens"][bi], c["W"]
    q, k, v = (np.asarray(d[n][bi], np.float64)[:, :, :L].transpose(0, 2, 1) for n in ("q", "k", "v"))      # [h, t, d_k]
    H, _, D = q.shape
    if L == 0:
        return np.zeros((H * D, 0))
    emb_k, emb_v = np.asarray(d["ek"], np.float64)[None], np.asarray(d["ev"], np.float64)[None]
    query = q * c["scale"]                                                    # query / sqrt(k_channels)
    scores = query @ k.transpose(0, 2, 1)
    rel_logits = query @ _get_relative_embeddings(emb_k, L, W).transpose(0, 2, 1)                             # [h, l, 2 l - 1]
    scores = scores + _relative_position_to_absolute_position(rel_logits)
    scores = scores - scores.max(-1, keepdims=True)
    p = np.exp(scores)
    p /= p.sum(-1, keepdims=True)
    out = p @ v
    out = out + _absolute_position_to_relative_position(p) @ _get_relative_embeddings(emb_v, L, W)
    return out.transpose(0, 2, 1).reshape(H * D, L)


def brute_force(c, d, bi):
    """one query at a time, straight from the formula; for the tiny agreement test"""
    L = d["lens"][bi]
    q, k, v = (np.asarray(d[n][bi], np.float64) for n in ("q", "k", "v"))
    H, D = q.shape[:2]
    out, lse = np.zeros((H, D, L)), np.zeros((H, L))
    for h in range(H):
        for t in range(L):
            sc = []
            for s in range(L):
                x = c["scale"] * float(q[h, :, t] @ k[h, :, s])
                if c["mode"] == "bias":
                    x += float(d["tab"][h, min(max(s - t, -CLIP), CLIP) + CLIP])
                if c["mode"] == "band" and abs(s - t) <= c["W"]:
                    x += c["scale"] * float(q[h, :, t] @ d["ek"][s - t + c["W"]]) if c["entry"] == "rel" else float(d["band"][bi, h, t, s - t + c["W"]])
                if c["mode"] == "causal" and s > t:
                    x = -np.inf
                sc.append(x)
            sc = np.array(sc)
            p = np.exp(sc - sc.max())
            lse[h, t] = sc.max() + np.log(p.sum())
            p /= p.sum()
            out[h, :, t] = v[h, :, :L] @ p
            if c["entry"] == "rel":
                for s in range(max(0, t - c["W"]), min(L, t + c["W"] + 1)):
                    out[h, :, t] += p[s] * np.asarray(d["ev"], np.float64)[s - t + c["W"]]
    return out.reshape(H * D, L), lse


def score_margin(c, d, bi):
    """nats between the best and the second-best admitted key of every query that has two (pointer cases assert >= 10)"""
    L = d["lens"][bi]
    if L < 2:
        return np.inf
    q, k = np.asarray(d["q"][bi], np.float64), np.asarray(d["k"][bi], np.float64)
    band = c["scale"] * np.einsum("hct,rc->htr", q[:, :, :L], np.asarray(d["ek"], np.float64)) if c["entry"] == "rel" else \
        (d["band"][bi] if d.get("band") is not None else None)
    s = np.sort(scores64(c, q, k, L, d.get("tab"), band)[0], axis=-1)
    two = np.isfinite(s[..., -2])
    return float((s[..., -1] - s[..., -2])[two].min()) if two.any() else np.inf


def pointed_key(c, d, bi):
    """the arg-max key of every query [H, len]"""
    L = d["lens"][bi]
    q, k = np.asarray(d["q"][bi], np.float64), np.asarray(d["k"][bi], np.float64)
    band = c["scale"] * np.einsum("hct,rc->htr", q[:, :, :L], np.asarray(d["ek"], np.float64)) if c["entry"] == "rel" else \
        (d["band"][bi] if d.get("band") is not None else None)
    return scores64(c, q, k, L, d.get("tab"), band)[0].argmax(-1)


# ---- cases
BIAS_OFFSETS = (-64, -63, -1, 0, 1, 63, 64)
COMMON = ("mask_last", "v_swap", "head_k", "skip_rescale")


def case(name, entry, D, mode, H, T, lens, layout, kind, *, claims, cs=None, std=0.0, W=0, scale=None, prod=None, offsets=None):
    assert D in DIMS and mode in MODES and layout in ("head", "block") and kind in KINDS and entry in ("attn", "rel")
    return dict(name=name, entry=entry, D=D, mode=mode, H=H, T=T, cs=cs or T, lens=list(lens), layout=layout, kind=kind, claims=tuple(claims),
                std=std, W=W, scale=float(np.float32(scale if scale is not None else 1.0 / np.sqrt(D))), prod=prod, offsets=offsets)


CASES = [
    # ---- the production (D, mode) pairs, with their layouts
    # GPT prefill / teacher-forced passes: 16 heads x 2 query blocks x 4 samples > 8 workgroups of distinct heads (the XCD remap);
    # len 200: block 1's key loop is cut at klimit = 200 < 256 and tiles 2, 3 reuse both buffers; 129: one active wave beside three idle
    case("gpt_causal_d48_h16", "attn", 48, "causal", 16, 200, [200, 129, 64, 0], "block", "prec", std=2.0, prod="gpt",
         claims=COMMON + ("causal_ge", "causal_t1", "stale_tile")),
    case("gpt_causal_d48_ptr", "attn", 48, "causal", 2, 300, [300, 128, 65, 1], "block", "score_ptr", prod="gpt",
         claims=("mask_last", "v_swap", "causal_ge", "stale_tile", "skip_rescale")),
    case("gpt_causal_d48_ramp", "attn", 48, "causal", 2, 300, [300, 33], "block", "ramp", std=1.0, prod="gpt",
         claims=COMMON + ("causal_ge", "causal_t1", "stale_tile")),
    # the trunk under conv_x3 = 0: per-head rows, row stride Ta > T
    case("trunk_bias_d48_h16", "attn", 48, "bias", 16, 130, [130, 63, 31], "head", "prec", std=0.6, cs=192, prod="trunk",
         claims=COMMON + ("admit_len", "bias_off1", "clamp63", "stale_tile")),
    case("trunk_bias_d48_ptr", "attn", 48, "bias", 8, 333, [333, 193, 128, 63], "head", "bias_ptr", cs=384, prod="trunk",
         offsets=BIAS_OFFSETS + (-32,), claims=("mask_last", "admit_len", "v_swap", "bias_off1", "clamp63", "skip_rescale")),
    case("trunk_bias_d48_std5", "attn", 48, "bias", 4, 200, [200, 193, 128, 33], "head", "prec", std=5.0, cs=200, prod="trunk",
         claims=COMMON + ("admit_len", "bias_off1", "clamp63", "stale_tile")),
    # enc_p: the composed entry (rel_key -> band + ml -> rel_value), W = 4, 4 heads
    case("encp_rel_d48", "rel", 48, "band", 4, 150, [150, 129, 33, 0], "block", "prec", std=2.0, W=4, prod="enc_p",
         claims=COMMON + ("admit_len", "band_off1", "band_w_1", "relv_wrong_l", "stale_tile")),
    case("encp_rel_d48_ptr", "rel", 48, "band", 4, 140, [140, 65, 31], "block", "band_ptr", W=4, prod="enc_p",
         claims=("mask_last", "admit_len", "v_swap", "band_off1", "band_w_1", "skip_rescale", "relv_wrong_l")),
    case("encp_rel_d48_std0.6", "rel", 48, "band", 4, 257, [257, 64, 1], "block", "prec", std=0.6, W=4, prod="enc_p",
         claims=COMMON + ("admit_len", "band_off1", "band_w_1", "relv_wrong_l", "stale_tile")),
    # the band mode alone through op_attention (band as data, cs > T), one pointer per head at each of the 2 W + 1 offsets
    case("band_d48_ptr", "attn", 48, "band", 9, 131, [131, 64, 5], "block", "band_ptr", W=4, cs=136, prod="enc_p",
         claims=("mask_last", "admit_len", "v_swap", "band_off1", "band_w_1", "skip_rescale")),
    # the MelStyleEncoders: plain, padded keys masked, scale 1 / sqrt(hidden)
    case("style_plain_d64", "attn", 64, "plain", 2, 257, [257, 192, 127, 31], "block", "prec", std=0.6, scale=1.0 / np.sqrt(128.0), prod="style64",
         claims=COMMON + ("admit_len", "stale_tile")),
    case("style_plain_d64_ptr", "attn", 64, "plain", 2, 384, [384, 191, 65, 1], "block", "score_ptr", scale=1.0 / np.sqrt(128.0), prod="style64",
         claims=("mask_last", "admit_len", "v_swap", "stale_tile", "skip_rescale")),
    case("style_plain_d64_ramp", "attn", 64, "plain", 2, 400, [400, 90], "block", "ramp", std=1.0, scale=1.0 / np.sqrt(128.0), prod="style64",
         claims=COMMON + ("admit_len", "stale_tile")),
    # D = 192: one LDS buffer, staged directly
    case("style_plain_d192", "attn", 192, "plain", 2, 200, [200, 129, 64, 1], "block", "prec", std=2.0, scale=1.0 / np.sqrt(384.0), prod="style192",
         claims=COMMON + ("admit_len",)),
    case("style_plain_d192_ramp", "attn", 192, "plain", 2, 160, [160, 65], "block", "ramp", std=1.0, scale=1.0 / np.sqrt(384.0), prod="style192",
         claims=COMMON + ("admit_len",)),
]


def _rest():
    """one small case for every instantiation production does not use, layouts and row strides alternating"""
    out, i = [], 0
    used = set(PRODUCTION.values())
    for D in DIMS:
        for mode in MODES:
            if (D, mode) in used:
                continue
            layout, cs = ("head", "block")[i % 2], (130, 160)[(i // 2) % 2]
            claims = COMMON + {"plain": ("admit_len",), "bias": ("admit_len", "bias_off1", "clamp63"), "causal": ("causal_ge", "causal_t1"),
                               "band": ("admit_len", "band_off1", "band_w_1")}[mode] + (("stale_tile",) if D <= 96 else ())
            out.append(case(f"rest_{mode}_d{D}", "attn", D, mode, 2, 130, [130, 65, 0] if i % 2 else [130, 33, 1], layout, "prec", std=2.0,
                            W=3 if mode == "band" else 0, cs=cs, claims=claims))
            i += 1
    return out


CASES += _rest()
BY_NAME = {c["name"]: c for c in CASES}


def pointer_targets(L, causal):
    """pi(t) for the score-pointer cases: key 0, key len - 1, both sides of every 64-key seam around the query, and for causal the
    diagonal itself, cycled over the queries (causal: clipped to s <= t); the last query and the two columns v_swap exchanges point at
    themselves, so that mask_last and v_swap show on pointer data too"""
    t = np.arange(L)
    cand = [np.zeros(L, int), np.full(L, L - 1), t // KT * KT - 1, t // KT * KT, t // KT * KT + KT - 1, t // KT * KT + KT, t]
    cand += [np.full(L, e) for kt in range(1, -(-L // KT)) for e in (KT * kt - 1, KT * kt)]
    pi = np.clip(np.stack(cand)[(t + t // KT) % len(cand), t], 0, L - 1)
    own = [L - 1] + ([swap_col(L), swap_col(L) + 1] if L > 1 else [])
    pi[own] = own
    return np.minimum(pi, t) if causal else pi


def make_data(c):
    """-> dict(q, k, v [B, H, D, T] fp32 (finite everywhere; pack_rows puts NaN beyond each length), lens, and per mode tab [H, 129],
    band [B, H, T, 2 W + 1] (NaN at t >= len), ek / ev [2 W + 1, D]); seeded per case"""
    rs = np.random.RandomState(seed_of(c["name"]))
    H, D, T, lens, W = c["H"], c["D"], c["T"], c["lens"], c["W"]
    B, R = len(lens), 2 * c["W"] + 1
    q, k = np.zeros((B, H, D, T), np.float32), np.zeros((B, H, D, T), np.float32)
    v = rs.randn(B, H, D, T).astype(np.float32)
    d = dict(lens=list(lens))
    kind = c["kind"]
    if kind in ("prec", "ramp"):
        g = np.sqrt(c["std"] / (c["scale"] * np.sqrt(D)))                      # scale q . k has the std asked for
        q[:], k[:] = rs.randn(B, H, D, T) * g, rs.randn(B, H, D, T) * g
        if kind == "ramp":      # test_attention_block_with_growing_scores_rescales_mid_sequence: later frames ~9 x larger
            ramp = (0.3 + 2.7 * np.arange(T) / T).astype(np.float32)
            q *= ramp
            k *= ramp
    elif kind == "score_ptr":
        # k_s = the key's own +-1 code, q_t = gain x the code of its target pi(t); the gain comes from the data so that the runner-up is
        # >= 10.5 nats below (score_margin re-checks it in the host test)
        worst = 0.0
        for bi, L in enumerate(lens):
            code = np.where(rs.rand(D, T) < 0.5, -1.0, 1.0).astype(np.float32)
            k[bi, :] = code
            q[bi, :, :, :L] = code[:, pointer_targets(L, c["mode"] == "causal")]
            if L > 1:
                worst = max(worst, float(np.max(code[:, :L].T @ code[:, :L] - 2 * D * np.eye(L))))
        gain = np.float32(10.5 / (c["scale"] * (D - worst)))
        q *= gain
    if c["mode"] == "bias":
        if kind == "bias_ptr":                                                 # scores 0, head h's table = small noise + 20 at offset o_h
            tab = rs.randn(H, 2 * CLIP + 1) * 0.05
            for h in range(H):
                tab[h, c["offsets"][h % len(c["offsets"])] + CLIP] = 20.0
        else:
            tab = rs.randn(H, 2 * CLIP + 1)
        d["tab"] = np.ascontiguousarray(tab, np.float32)
    if c["mode"] == "band":
        if c["entry"] == "rel":
            ek = rs.randn(R, D) / np.sqrt(D)
            if kind == "band_ptr":
                # scores 0 (k = 0); (sample b, head h) owns channel b H + h: q = 4 there, ek[r*] = 20 / (4 scale) there, r* = (b H + h) % R
                ek = rs.randn(R, D) * 0.002
                for bi in range(B):
                    for h in range(H):
                        ch = bi * H + h
                        q[bi, h, ch, :] = 4.0
                        ek[:, ch] = rs.randn(R) * 0.01
                        ek[ch % R, ch] = 20.0 / (4.0 * c["scale"])
            d["ek"], d["ev"] = np.ascontiguousarray(ek, np.float32), np.ascontiguousarray(rs.randn(R, D) / np.sqrt(D), np.float32)
        else:
            band = rs.randn(B, H, T, R)
            if kind == "band_ptr":
                band *= 0.05
                for bi in range(B):
                    for h in range(H):
                        band[bi, h, :, (bi * H + h) % R] = 20.0
            for bi, L in enumerate(lens):
                band[bi, :, L:] = np.nan                                        # rel_key writes t < len only: the kernel must not read beyond
            d["band"] = np.ascontiguousarray(band, np.float32)
    d.update(q=q, k=k, v=v)
    return d


# ---- what the entries refuse; kwargs on top of a plain D = 48, H = 2, T = cs = 100, lens [100, 50], per-head layout call
REJECTS = [          # (name, kwargs, what the refusal says)
    ("dim32", dict(dim=32), "head dim"),
    ("dim128", dict(dim=128), "head dim"),
    ("k_off_beyond_rows", dict(k_off=200), "leave the tensor"),
    ("v_off_negative", dict(v_off=-1), "leave the tensor"),
    ("head_stride_beyond_rows", dict(head_stride=241), "leave the tensor"),
    ("len_beyond_T", dict(lens=[100, 101]), "lengths"),
    ("len_negative", dict(lens=[-1, 50]), "lengths"),
    ("T_beyond_cs", dict(T=101), "row stride"),
    ("bias_shape", dict(bias_shape=(2, 128)), "bias_tab must be"),
    ("bias_heads", dict(bias_shape=(3, 129)), "bias_tab must be"),
    ("band_shape", dict(band_shape=(2, 2, 100, 8), band_w=4), "band must be"),
    ("band_window", dict(band_shape=(2, 2, 100, 17), band_w=8), "band window"),
    ("bias_and_causal", dict(bias_shape=(2, 129), causal=True), "at most one"),
    ("bias_and_band", dict(bias_shape=(2, 129), band_shape=(2, 2, 100, 9), band_w=4), "at most one"),
    ("causal_and_band", dict(causal=True, band_shape=(2, 2, 100, 9), band_w=4), "at most one"),
    ("heads_0", dict(heads=0), "empty attention"),
]
REL_REJECTS = [      # on top of D = 48, H = 2, T = 100, W = 4, lens [100, 50]
    ("ek_shape", dict(ek_shape=(8, 48)), "ek and ev must be"),
    ("window_8", dict(window=8), "window"),
    ("dim32", dict(dim=32), "head dim"),
    ("len_beyond_T", dict(lens=[100, 101]), "lengths"),
    ("rows", dict(rows=200), "qkv must be"),
]
