"""The launch-per-GEMV decode chain of the GPT (csrc/gpt_kernels.hip: gemv_block_kernel with its four prologues,
decode_attention_qkv_kernel<48, PROJ>, gpt_final_ln_kernel, ln_fold_vectors_kernel, kv_to_cache_kernel) in numpy.  Shared by
tests/test_gpu_gpt_decode.py (one launch at a time through Runtime.op_gemv_block / op_decode_attention / op_gpt_final_ln /
op_ln_fold_vectors / op_kv_to_cache) and tests/test_host_gpt_decode.py.  It holds
  * the case table and its planted data;
  * float64 references written from the DEFINITION of each operation - LayerNorm, softmax, gelu_new, a matrix product - on the data the
    operation is defined on (the row x that is normalised, the weight behind it), not on the kernel's inputs: where the kernel is fed
    something derived (split-K partials of (gamma . x)^T W, per-slice (sum, sum of squares) of x, the fold vectors c = W^T gamma and
    d = W^T beta + b) the data builder derives it in float64 and rounds it to fp32 once;
  * kernel models: the kernel's own algebra - r (a - mu c) + d, records (m, l, o) per key range, the exp(m_j - m) merge - in float64 on the
    kernel's inputs, which test_host_gpt_decode.py holds equal to the definition, and which takes the MUTATIONS;
  * the mutation table: wrong kernels, each claimed by the cases that catch it at >= 3 x their gate;
  * the gates, and the fp32 evaluation of the definition they are held above.

Metric, as everywhere in this suite: rel_err = max |y - ref| / max(1, max |ref|).

The launcher's rules, re-derived here (gemv_rule) and compared with what the entry reports: 64 VEC columns x 8 RPW input rows per
workgroup; wide (VEC 4, RPW 16) when ceil(CoutP / 256) (K / 128) >= 192, else narrow (VEC 1) with 64 input rows (RPW 8) when
ceil(CoutP / 64) (K / 128) < 128, else 128 (RPW 16); NB = 8 for B <= 8, else 16; one partial slice per RB = 8 RPW input rows.
sum_parts has unrolled bodies for 1, 6, 12, 16 and 24 slices and a rolled one (4 at a time + a tail) for every other count.  The
attention gives key range ks of KS the cached keys [ks per, min(nc, (ks + 1) per)), per = ceil(nc / KS), nc = lp + step - 1, and the
last range the new key as well; its score loop strides by 256 threads, its PV loop gives key s to slot s % 21, 8 keys per round while
slot + 147 < ncl, then a tail of up to 7."""
import functools
import math
import zlib

import numpy as np

LN_EPS = 1e-5
HEAD_DIM = 48
ATT_REC = 64
PV_SLOTS = 21
UNROLLED = (1, 6, 12, 16, 24)

# ---- gates.  Every operation here is a sum of K <= 3072 fp32 products behind an O(1) prologue.  A sum of K terms of size t rounded
# to nearest carries an error of about sqrt(K) eps t (eps = 2^-24 = 6e-8: a random walk of K roundings), i.e. 1 - 3e-6 of the result's
# scale at K = 768 .. 3072, and the LayerNorm algebra adds the same again (a and mu c are each about the size of their difference: the
# planted rows have mean = standard deviation, so nothing is amplified beyond a factor ~ 2).  f32_figure() measures exactly that on the
# CPU: the definition evaluated in fp32 in numpy's order against float64.  The kernel sums the same terms in ANOTHER order (RB-row
# slices, 8 waves, 4 interleaved accumulators), which is a second, independent draw of the same random walk, and its maximum is taken
# over up to 127 000 outputs; hardware tanh / exp add an ulp or two per element.  MARGIN = 4 between the fp32 figure and the gate
# covers two draws of one distribution (a factor ~ 2 between maxima) and those ulps (another ~ 2); test_host_gpt_decode.py holds every
# gate >= MARGIN x the family's worst fp32 figure and <= 1/3 of the smallest mutation a case claims.  The gates are per family:
MARGIN = 4.0
GATES = {
    "plain": 4e-6,          # sqrt(768) eps = 1.7e-6 of |x| |W| sqrt(K) ~ the result's scale
    "ressum": 4e-6,
    "lnparts": 1e-5,        # + the LayerNorm algebra and gelu_new in front of a K <= 768 sum
    "attn_merge": 4e-6,
    "attn_split": 1e-5,     # LayerNorm algebra over C, 48-term scores, exp, up to 600 keys
    "attn_fused": 1e-5,
    "final_ln": 1e-5,       # two LayerNorms back to back
    "ln_fold": 4e-6,
    "layer": 2e-5,          # five kernels in a row at K = 768 / 3072
}


def rel_err(y, ref):
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    if not np.isfinite(y).all():
        return float("inf")
    return float(np.max(np.abs(y - ref))) / max(1.0, float(np.max(np.abs(ref))))


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


def cdiv(a, b):
    return -(-a // b)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


# ---- the launcher's rules
def gemv_rule(K, CoutP, B):
    """-> dict(vec, rpw, nb, rb, slices, shape): what launch_gemv_block picks for (K, CoutP, B)"""
    wide = cdiv(CoutP, 256) * (K // 128) >= 192
    rows = 64 if (cdiv(CoutP, 64) * (K // 128) < 128 and K % 64 == 0) else 128
    vec, rpw = (4, 16) if wide else (1, 8 if rows == 64 else 16)
    nb = 8 if B <= 8 else 16
    return dict(vec=vec, rpw=rpw, nb=nb, rb=8 * rpw, slices=K // (8 * rpw), shape="wide" if wide else ("n64" if rpw == 8 else "n128"),
                tail_cols=CoutP % (64 * vec))


def sum_body(n):
    """the body of sum_parts a slice count takes"""
    if n == 0:
        return "none"
    if n in UNROLLED:
        return f"unrolled{n}"
    return "rolled" + ("_loop" if n >= 4 else "") + ("_tail" if n % 4 else "")


def key_ranges(nc, KS):
    """-> [(s_lo, s_hi)] cached keys of every split; an empty range has s_hi <= s_lo"""
    per = cdiv(nc, KS)
    return [(ks * per, min(nc, ks * per + per)) for ks in range(KS)]


def attention_paths(nc, KS):
    """loop edges the (row, split) workgroups of a launch run into"""
    out = set()
    for ks, (lo, hi) in enumerate(key_ranges(nc, KS)):
        ncl = max(hi - lo, 0)
        last = ks == KS - 1
        nk = ncl + (1 if last else 0)
        if ncl == 0:
            out.add("new_key_only" if last else "empty_split")
        if lo + cdiv(nc, KS) > nc and ncl > 0:
            out.add("range_overshoots_nc")
        for e in (256, 257, 258):                          # 256 threads: one key each at 256, thread 0 takes a second at 257
            if nk == e:
                out.add(f"score_loop_nk{e}")
        for e in (147, 148, 168, 169):
            if ncl == e:
                out.add(f"pv_ncl{e}")
        if ncl > 8 * PV_SLOTS + 147:
            out.add("pv_two_rounds")
        if 0 < ncl <= 147:
            out.add("pv_tail_only")
        for e in (20, 21, 22):
            if ncl == e:
                out.add(f"pv_slots{e}")
    return out


# ---- the definitions, in the dtype of their arguments
def layer_norm(x, g, b, eps=LN_EPS):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + x.dtype.type(eps)) * g + b


def gelu_new(x):
    t = x.dtype.type
    return t(0.5) * x * (t(1.0) + np.tanh(t(math.sqrt(2.0 / math.pi)) * (x + t(0.044715) * x * x * x)))


def gelu_erf(x):
    return 0.5 * x * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))


def softmax(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


ROW_SCALE = (1.0, 0.02, 0.3)      # rows b % 3; 0.02: variance 4e-4, where the LayerNorm's eps = 1e-5 is 1.2 % of the rstd


def ln_rows(rs, B, K):
    """rows to be normalised: mean = standard deviation (= the row's scale), so that a lost or misplaced mean term is as large as the row"""
    sc = np.array([ROW_SCALE[b % 3] for b in range(B)])[:, None]
    return f32(sc * (1.0 + rs.randn(B, K)))


def nan_pad(a, shape):
    """a in the leading corner of a NaN-filled fp32 array of `shape`"""
    out = np.full(shape, np.nan, np.float32)
    out[tuple(slice(0, n) for n in a.shape)] = a
    return out


def split_slices(rs, total, n, extra=1):
    """total [B, N] float64 -> fp32 [n + extra, B, N]: n slices of DISTINCT magnitudes (slice i: weight (i + 1) and noise of scale
    0.5 + i / n times the total's) that sum to `total` in float64 before the one rounding to fp32; `extra` more slices of NaN"""
    B, N = total.shape
    w = np.arange(1, n + 1, dtype=np.float64)
    w /= w.sum()
    scale = np.abs(total).mean() + 1e-30
    noise = rs.randn(n, B, N) * (scale * (0.5 + np.arange(n) / n) / math.sqrt(n))[:, None, None]
    noise -= w[:, None, None] * noise.sum(0)
    return nan_pad(f32(w[:, None, None] * total + noise), (n + extra, B, N))


def slice_stats(x, n, extra=1):
    """x [B, K] float64 -> fp32 [n + extra, B, 2]: (sum, sum of squares) over n contiguous column ranges; NaN slices behind"""
    B, K = x.shape
    edges = [K * i // n for i in range(n + 1)]
    st = np.stack([np.stack([x[:, a:b].sum(-1), (x[:, a:b] ** 2).sum(-1)], -1) for a, b in zip(edges[:-1], edges[1:])])
    return nan_pad(f32(st), (n + extra, B, 2))


def stats_of(stats, n, K, mut=None):
    """the kernel's ln_row_stats in float64 -> (mean [B, 1], rstd [B, 1])"""
    use = n - 1 if mut == "stats_short" else n
    S, Q = stats[:use, :, 0].astype(np.float64).sum(0), stats[:use, :, 1].astype(np.float64).sum(0)
    mean = S / K
    var = np.maximum(Q / K - mean * mean, 0.0)
    return mean[:, None], 1.0 / np.sqrt(var + (0.0 if mut == "eps_missing" else LN_EPS))[:, None]


def sum_slices(parts, n, mut=None):
    """sum of the first n slices in float64; slice_dropped / slice_twice hit slice n // 2"""
    p = parts[:n].astype(np.float64)
    s = p.sum(0)
    if mut == "slice_dropped" and n:
        s = s - p[n // 2]
    if mut == "slice_twice" and n:
        s = s + p[n // 2]
    return s


@functools.lru_cache(maxsize=None)
def weight(K, N, tag="w", gain=1.0):
    """fp32 [K, N] ~ N(0, gain^2 / K), one per (shape, tag): shared by the cases of a shape"""
    rs = np.random.RandomState(seed_of(f"{tag}_{K}_{N}"))
    return f32(rs.standard_normal((K, N)) * (gain / math.sqrt(K)))


@functools.lru_cache(maxsize=None)
def weight64(K, N, tag="w", gain=1.0):
    return weight(K, N, tag, gain).astype(np.float64)


MUTATIONS = ("slice_dropped", "slice_twice", "bias_twice", "gamma_in_y", "stats_short", "mu_c_dropped", "fold_swapped", "eps_missing",
             "erf_gelu", "scale_missing", "new_key_out", "split_shift", "merge_no_rescale", "v_row_prev", "k_append_next", "clamp_leak")

# ================================================================================================================= GEMV cases
SHAPES = {"n64": (128, 68), "n128": (256, 4096), "wide": (768, 7940)}


def gemv_case(pro, shape, B, in_slices=0, stats_slices=0, K_ln=0, KS=0, act=4, claims=()):
    K, N = SHAPES[shape]
    name = f"{pro}_{shape}_B{B}" + (f"_s{in_slices}" if pro in ("ressum", "lnparts") else "") + (f"_st{stats_slices}" if pro == "lnparts" else "") + \
        (f"_ks{KS}" if pro == "attn" else "") + ("_noact" if pro == "lnparts" and act == 0 else "")
    rule = gemv_rule(K, N, B)
    assert rule["shape"] == shape, (name, rule)
    hd = 0 if pro != "attn" else (48 if K % 48 == 0 else 32)
    return dict(name=name, family={"attn": "attn_merge"}.get(pro, pro), pro=pro, shape=shape, K=K, CoutP=N, B=B, in_slices=KS if pro == "attn" else in_slices,
                stats_slices=stats_slices, K_ln=K_ln, act=act, head_dim=hd, rule=rule, claims=tuple(claims))


_RES = ("slice_dropped", "slice_twice", "bias_twice", "gamma_in_y")
_LNP = ("slice_dropped", "slice_twice", "stats_short", "mu_c_dropped", "fold_swapped", "erf_gelu")
GEMV_CASES = [
    gemv_case("plain", "n64", 1),
    gemv_case("plain", "n64", 9, claims=("clamp_leak",)),
    gemv_case("plain", "n128", 3, claims=("clamp_leak",)),
    gemv_case("plain", "n128", 16, claims=("clamp_leak",)),
    gemv_case("plain", "wide", 8, claims=("clamp_leak",)),
    gemv_case("plain", "wide", 16, claims=("clamp_leak",)),
    gemv_case("ressum", "n64", 3, 5, claims=_RES + ("clamp_leak",)),
    gemv_case("ressum", "n64", 8, 0, claims=("bias_twice", "gamma_in_y", "clamp_leak")),
    gemv_case("ressum", "n64", 9, 12, claims=_RES),
    gemv_case("ressum", "n128", 1, 1, claims=_RES),
    gemv_case("ressum", "n128", 3, 6, claims=_RES),
    gemv_case("ressum", "n128", 16, 7, claims=_RES + ("clamp_leak",)),
    gemv_case("ressum", "wide", 8, 16, claims=_RES),
    gemv_case("ressum", "wide", 9, 24, claims=_RES + ("clamp_leak",)),
    gemv_case("lnparts", "n64", 8, 6, 1, 96, claims=_LNP + ("eps_missing", "clamp_leak")),
    gemv_case("lnparts", "n64", 16, 7, 6, 192, claims=_LNP + ("eps_missing",)),
    gemv_case("lnparts", "n128", 1, 12, 1, 96, claims=_LNP),
    gemv_case("lnparts", "n128", 9, 5, 6, 192, claims=_LNP + ("eps_missing", "clamp_leak")),
    gemv_case("lnparts", "n128", 3, 16, 6, 96, act=0, claims=("slice_dropped", "slice_twice", "stats_short", "mu_c_dropped", "fold_swapped", "eps_missing")),
    gemv_case("lnparts", "wide", 3, 24, 6, 192, claims=_LNP + ("eps_missing", "clamp_leak")),
    gemv_case("lnparts", "wide", 16, 1, 6, 96, claims=("stats_short", "mu_c_dropped", "fold_swapped", "erf_gelu", "eps_missing")),
    gemv_case("attn", "n64", 3, KS=1, claims=("clamp_leak",)),
    gemv_case("attn", "n64", 9, KS=8, claims=("merge_no_rescale", "clamp_leak")),
    gemv_case("attn", "n128", 1, KS=8, claims=("merge_no_rescale",)),
    gemv_case("attn", "n128", 16, KS=2, claims=("merge_no_rescale", "clamp_leak")),
    gemv_case("attn", "wide", 8, KS=4, claims=("merge_no_rescale", "clamp_leak")),
    gemv_case("attn", "wide", 9, KS=2, claims=("merge_no_rescale",)),
]
GEMV_BY_NAME = {c["name"]: c for c in GEMV_CASES}
assert len(GEMV_BY_NAME) == len(GEMV_CASES)


@functools.lru_cache(maxsize=None)
def gemv_data(name):
    """the kernel's inputs (fp32, NaN wherever the kernel may not read: columns >= K of x and parts, rows >= B of x, slices >=
    in_slices / stats_slices) and what they were derived from.  Never modified."""
    c = GEMV_BY_NAME[name]
    rs = np.random.RandomState(seed_of(name))
    K, N, B, pro, n = c["K"], c["CoutP"], c["B"], c["pro"], c["in_slices"]
    d = dict(W=weight(K, N))
    if pro == "plain":
        d["x"] = nan_pad(ln_rows(rs, B, K), (B + 2, K + 8))
    elif pro == "ressum":
        d["x"] = nan_pad(f32(0.6 + 0.6 * rs.randn(B, K)), (B + 2, K + 8))
        d["in_bias"] = f32(0.3 * rs.randn(K))
        d["gamma"] = f32(1.0 + 0.3 * rs.randn(K))
        if n:
            d["parts"] = nan_pad(split_slices(rs, 0.5 + 0.7 * rs.randn(B, K), n), (n + 1, B, K + 4))
    elif pro == "lnparts":
        Kl = c["K_ln"]
        d["y"], d["g"], d["b"] = ln_rows(rs, B, Kl), f32(1.0 + 0.3 * rs.randn(Kl)), f32(0.2 * rs.randn(Kl))
        d["Wfc"], d["bfc"] = weight(Kl, K, "fc"), f32(0.2 * rs.randn(K))
        y, g, bta, Wfc = (d[k].astype(np.float64) for k in ("y", "g", "b", "Wfc"))
        d["parts"] = nan_pad(split_slices(rs, (g * y) @ Wfc, n), (n + 1, B, K + 4))
        d["stats_in"] = slice_stats(y, c["stats_slices"])
        d["fold_c"], d["fold_d"] = f32(g @ Wfc), f32(bta @ Wfc + d["bfc"].astype(np.float64))
    else:
        hd, H, KS = c["head_dim"], K // c["head_dim"], n
        rec = np.full((B, H, KS, ATT_REC), np.nan, np.float32)
        live = rs.rand(B, H, KS) < 0.7 if KS > 2 else np.ones((B, H, KS), bool)
        live[:, :, -1] = True                                  # the last split owns the new key: never empty
        m = 3.0 * rs.randn(B, H, KS)
        l = 0.5 + 20.0 * rs.rand(B, H, KS)
        o = l[..., None] * (0.3 + rs.randn(B, H, KS, hd))
        rec[..., 0] = np.where(live, m, -np.inf)
        rec[..., 1] = np.where(live, l, 0.0)
        rec[..., 2:2 + hd] = np.where(live[..., None], o, 0.0)
        d["parts"] = rec
    return d


def gemv_input(c, d, mut=None, dt=np.float64):
    """v [B, K]: the GEMV's input rows by the DEFINITION of the prologue (plain, ressum, attn), or by the kernel's algebra on its inputs
    (lnparts: the definition is gemv_reference's direct LayerNorm) -> (v, y_out or None)"""
    K, B, pro, n = c["K"], c["B"], c["pro"], c["in_slices"]
    y_out = None
    if pro == "plain":
        v = d["x"][:B, :K].astype(dt)
    elif pro == "ressum":
        bias = d["in_bias"].astype(dt)
        v = d["x"][:B, :K].astype(dt) + bias * (2 if mut == "bias_twice" else 1)
        if n:
            v = v + (sum_slices(d["parts"][:, :, :K], n, mut) if dt == np.float64 else d["parts"][:n, :, :K].sum(0, dtype=dt))
        y_out = v * d["gamma"].astype(dt) if mut == "gamma_in_y" else v
        v = v * d["gamma"].astype(dt)
    elif pro == "lnparts":
        mean, rstd = stats_of(d["stats_in"], c["stats_slices"], c["K_ln"], mut)
        a = sum_slices(d["parts"][:, :, :K], n, mut)
        fc, fd = d["fold_c"].astype(np.float64), d["fold_d"].astype(np.float64)
        if mut == "fold_swapped":
            fc, fd = fd, fc
        t = rstd * (a - (0.0 if mut == "mu_c_dropped" else mean) * fc) + fd
        v = t if c["act"] == 0 else (gelu_erf(t) if mut == "erf_gelu" else gelu_new(t))
    else:
        hd, KS = c["head_dim"], n
        rec = d["parts"].astype(dt)
        m, l, o = rec[..., 0], rec[..., 1], rec[..., 2:2 + hd]
        w = np.ones_like(m) if mut == "merge_no_rescale" else np.exp(m - m.max(-1, keepdims=True))
        v = ((w[..., None] * o).sum(2) / (w * l).sum(2)[..., None]).reshape(B, K)
    if mut == "clamp_leak" and B >= 2:
        v = v.copy()
        v[B - 2] = v[B - 1]
    return v, y_out


def gemv_reference(c, d, mut=None, dt=np.float64):
    """-> dict(part [slices, B, CoutP], and for ressum y_out [B, K], stats_out [slices, B, 2]).  mut None: the definition."""
    K, B, rb, S = c["K"], c["B"], c["rule"]["rb"], c["rule"]["slices"]
    if c["pro"] == "lnparts" and mut is None:
        y, g, bta, Wfc, bfc = (d[k].astype(dt) for k in ("y", "g", "b", "Wfc", "bfc"))
        t = layer_norm(y, g, bta) @ Wfc + bfc
        v, y_out = (t if c["act"] == 0 else gelu_new(t)), None
    else:
        v, y_out = gemv_input(c, d, mut, dt)
    W = weight64(K, c["CoutP"]) if dt == np.float64 else d["W"]
    out = dict(part=np.stack([v[:, i * rb:(i + 1) * rb] @ W[i * rb:(i + 1) * rb] for i in range(S)]))
    if c["pro"] == "ressum":
        out["y_out"] = y_out
        out["stats_out"] = np.stack([np.stack([y_out[:, i * rb:(i + 1) * rb].sum(-1), (y_out[:, i * rb:(i + 1) * rb] ** 2).sum(-1)], -1) for i in range(S)])
    return out


def dict_err(got, ref):
    """the case's metric: the worst rel_err over its outputs"""
    return max(rel_err(got[k], ref[k]) for k in ref)


# ================================================================================================================= attention cases
NC_ALL = (1, 7, 20, 21, 22, 147, 148, 168, 169, 255, 256, 257, 600)


def attn_case(name, form, H, ncs, steps, KS=0, slices=6, stats_slices=6, claims=()):
    assert len(ncs) == len(steps)
    return dict(name=name, family="attn_" + form, form=form, H=H, C=H * HEAD_DIM, B=len(ncs), ncs=tuple(ncs), steps=tuple(steps), KS=KS,
                slices=slices, stats_slices=stats_slices, cap=max(ncs) + 4, CoutP=3 * H * HEAD_DIM + 4, claims=tuple(claims))


_ATT = ("stats_short", "mu_c_dropped", "fold_swapped", "eps_missing", "scale_missing", "new_key_out", "v_row_prev", "k_append_next")
_STEPS13 = (0, 3, 5, 0, 2, 40, 0, 7, 1, 0, 100, 9, 33)
ATTN_CASES = [
    attn_case("split_ks1", "split", 2, NC_ALL, _STEPS13, KS=1, slices=6, claims=_ATT + ("slice_dropped", "slice_twice")),
    attn_case("split_ks2", "split", 2, NC_ALL, _STEPS13, KS=2, slices=7, stats_slices=1, claims=_ATT + ("split_shift", "slice_dropped", "slice_twice")),
    attn_case("split_ks3", "split", 2, NC_ALL, _STEPS13, KS=3, slices=1, claims=_ATT + ("split_shift",)),
    attn_case("split_ks8", "split", 2, NC_ALL, _STEPS13, KS=8, slices=5, claims=_ATT + ("split_shift", "slice_dropped", "slice_twice")),
    attn_case("fused_small", "fused", 16, (1, 7, 20, 21, 22), (0, 3, 0, 2, 5), claims=_ATT + ("slice_dropped", "slice_twice")),
    attn_case("fused_pv_edge", "fused", 16, (147, 148, 168, 169), (0, 40, 7, 0), claims=_ATT),
    attn_case("fused_score_edge", "fused", 16, (255, 256, 257, 600), (100, 0, 9, 0), slices=12, stats_slices=1, claims=_ATT),
]
ATTN_BY_NAME = {c["name"]: c for c in ATTN_CASES}


@functools.lru_cache(maxsize=None)
def attn_data(name):
    c = ATTN_BY_NAME[name]
    return make_attn_data(c, np.random.RandomState(seed_of(name)))


def make_attn_data(c, rs, x=None):
    """the layer's input rows x [B, C] (what LayerNorm is defined on), c_attn and the planted cache -> the kernel's inputs: split-K partials
    of (gamma . x)^T W, per-slice statistics of x, the fold vectors, cache [B, 2 C cap] with NaN at every column >= nc = n - 1, (lp, step)
    with lp + step = nc + 1; in the fused form also the projection weight [C, 768]"""
    B, C, cap, N, H = c["B"], c["C"], c["cap"], c["CoutP"], c["H"]
    d = dict(x=ln_rows(rs, B, C) if x is None else x, g=f32(1.0 + 0.3 * rs.randn(C)), b=f32(0.2 * rs.randn(C)),
             W=weight(C, 3 * C, "attn", 1.5), bias=f32(0.2 * rs.randn(3 * C)))
    x64, g, bta, W = (d[k].astype(np.float64) for k in ("x", "g", "b", "W"))
    d["part"] = nan_pad(split_slices(rs, (g * x64) @ W, c["slices"]), (c["slices"] + 1, B, N))
    d["stats"] = slice_stats(x64, c["stats_slices"])
    d["fold_c"], d["fold_d"] = nan_pad(f32(g @ W), (N,)), nan_pad(f32(bta @ W + d["bias"].astype(np.float64)), (N,))
    cache = np.full((B, 2 * C * cap), np.nan, np.float32)
    for b, nc in enumerate(c["ncs"]):
        cache[b, :C * cap].reshape(C, cap)[:, :nc] = rs.randn(C, nc)
        cache[b, C * cap:].reshape(cap, C)[:nc] = rs.randn(nc, C)
    d["cache"] = cache
    d["step"] = np.array(c["steps"], np.int32)
    d["lp"] = np.array(c["ncs"], np.int32) + 1 - d["step"]
    if c["form"] == "fused":
        d["wproj"] = weight(C, 768, "proj")
    return d


def attn_qkv(c, d, mut=None, dt=np.float64):
    """q, k, v [B, 3 C]: by the definition LayerNorm(x)^T W + b (mut None), or by the kernel's algebra on its inputs (any mut, or
    mut = "algebra")"""
    C = c["C"]
    if mut is None:
        return layer_norm(d["x"].astype(dt), d["g"].astype(dt), d["b"].astype(dt)) @ d["W"].astype(dt) + d["bias"].astype(dt)
    mean, rstd = stats_of(d["stats"], c["stats_slices"], C, mut)
    a = sum_slices(d["part"][:, :, :3 * C], c["slices"], mut)
    fc, fd = d["fold_c"][:3 * C].astype(np.float64), d["fold_d"][:3 * C].astype(np.float64)
    if mut == "fold_swapped":
        fc, fd = fd, fc
    return rstd * (a - (0.0 if mut == "mu_c_dropped" else mean) * fc) + fd


def attn_reference(c, d, mut=None, dt=np.float64, rows=None):
    """-> dict(out [B, C] softmax(q k / sqrt(48)) v over the nc cached keys and the new one, cache [B, 2 C cap] after the call (fp32
    image: the planted cache with k / v at column pos = nc), and by form: records rec_m / rec_l [B, H, KS], rec_o [B, H, KS, 48] of
    the key ranges (an empty range: -inf, 0, 0) or partial [H, B, 768] = out_h^T wproj_h"""
    B, C, H, cap, D = c["B"], c["C"], c["H"], c["cap"], HEAD_DIM
    qkv = attn_qkv(c, d, mut, dt)
    scale = dt(1.0) if mut == "scale_missing" else dt(1.0 / math.sqrt(D))
    KS = max(c["KS"], 1)
    out = np.zeros((B, C), dt)
    rec_m, rec_l, rec_o = np.full((B, H, KS), -np.inf), np.zeros((B, H, KS)), np.zeros((B, H, KS, D))
    cache = d["cache"].copy()
    for b in (range(B) if rows is None else rows):
        nc = c["ncs"][b]
        Kc, Vc = d["cache"][b, :C * cap].reshape(C, cap)[:, :nc].astype(dt), d["cache"][b, C * cap:].reshape(cap, C)[:nc].astype(dt)
        # the append: k to column pos = nc of K [C, cap], v to row pos of V [cap, C] (k_append_next / v_row_prev: one off; cap > nc + 1)
        cache[b, :C * cap].reshape(C, cap)[:, nc + 1 if mut == "k_append_next" else nc] = qkv[b, C:2 * C]
        cache[b, C * cap:].reshape(cap, C)[nc - 1 if mut == "v_row_prev" else nc] = qkv[b, 2 * C:]
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            q, k, v = qkv[b, sl], qkv[b, C + h * D: C + (h + 1) * D], qkv[b, 2 * C + h * D: 2 * C + (h + 1) * D]
            keys = np.concatenate([Kc[sl].T, k[None]]) if mut != "new_key_out" else Kc[sl].T
            vals = np.concatenate([Vc[:, sl], v[None]]) if mut != "new_key_out" else Vc[:, sl]
            s = (keys @ q) * scale
            if len(s):
                out[b, sl] = softmax(s) @ vals
            if c["form"] == "split" and dt == np.float64:
                for ks, (lo, hi) in enumerate(key_ranges(nc, KS)):
                    if mut == "split_shift" and ks > 0:
                        lo = lo - 1                               # the boundary key is taken by both ranges
                    idx = list(range(lo, hi)) if hi > lo else []
                    if ks == KS - 1 and mut != "new_key_out":
                        idx.append(nc)
                    if idx:
                        ss = s[idx]
                        e = np.exp(ss - ss.max())
                        rec_m[b, h, ks], rec_l[b, h, ks], rec_o[b, h, ks] = ss.max(), e.sum(), e @ vals[idx]
    res = dict(out=out, cache=cache)
    if c["form"] == "split":
        res.update(rec_m=rec_m, rec_l=rec_l, rec_o=rec_o)
    else:
        wp = d["wproj"].astype(dt)
        res["partial"] = np.stack([out[:, h * D:(h + 1) * D] @ wp[h * D:(h + 1) * D] for h in range(H)])
    return res


def merge_records(m, l, o):
    """float64 merge of key-range records -> normalised out [..., 48]"""
    w = np.exp(m - m.max(-1, keepdims=True))
    return (w[..., None] * o).sum(-2) / (w * l).sum(-1)[..., None]


def cache_placement(got, ref):
    """exact part of the cache check: the same cells written, every other cell bit-identical to the planted image -> number of cells
    whose NaN-ness differs"""
    return int((np.isnan(got) != np.isnan(ref)).sum())


def attn_err(c, got, ref):
    """the case's metric.  got / ref: dicts as attn_reference returns them (got's records taken from the kernel's [B, H, KS, 64]).  A cache
    written in other cells than the reference's is an infinite error."""
    if cache_placement(got["cache"], ref["cache"]):
        return float("inf")
    fin = ~np.isnan(ref["cache"])
    errs = [rel_err(got["cache"][fin], ref["cache"][fin])]
    if c["form"] == "fused":
        errs.append(rel_err(got["partial"], ref["partial"]))
    else:
        live = np.isfinite(ref["rec_m"])
        if not np.array_equal(live, np.isfinite(got["rec_m"])) or (got["rec_l"][~live] != 0).any() or (got["rec_o"][~live] != 0).any():
            return float("inf")
        errs += [rel_err(got["rec_m"][live], ref["rec_m"][live]), rel_err(got["rec_l"][live], ref["rec_l"][live]), rel_err(got["rec_o"][live], ref["rec_o"][live]),
                 rel_err(merge_records(got["rec_m"], got["rec_l"], got["rec_o"]).reshape(ref["out"].shape), ref["out"])]
    return max(errs)


# ================================================================================================================= the small kernels
FINAL_LN_CASES = [dict(name="final_ln_C768_s24", family="final_ln", C=768, B=3, in_slices=24, bias=True, steps=(0, 2, 4), max_steps=4, lat_cs=5,
                       claims=("slice_dropped", "slice_twice", "bias_twice", "eps_missing")),
                  dict(name="final_ln_C1000_s5", family="final_ln", C=1000, B=4, in_slices=5, bias=True, steps=(1, 0, 3, 2), max_steps=8, lat_cs=4,
                       claims=("slice_dropped", "slice_twice", "bias_twice", "eps_missing")),
                  dict(name="final_ln_C1024_s0", family="final_ln", C=1024, B=2, in_slices=0, bias=False, steps=(0, 0), max_steps=1, lat_cs=0,
                       claims=("eps_missing",))]
FINAL_BY_NAME = {c["name"]: c for c in FINAL_LN_CASES}


@functools.lru_cache(maxsize=None)
def final_ln_data(name):
    c = FINAL_BY_NAME[name]
    rs = np.random.RandomState(seed_of(name))
    C, B, n = c["C"], c["B"], c["in_slices"]
    sc = np.array([ROW_SCALE[(b + 1) % 3] for b in range(B)])[:, None]
    d = dict(res=f32(sc * (1.0 + rs.randn(B, C))), g1=f32(1.0 + 0.3 * rs.randn(C)), b1=f32(0.2 * rs.randn(C)), g2=f32(1.0 + 0.3 * rs.randn(C)),
             b2=f32(0.2 * rs.randn(C)))
    if c["bias"]:
        d["bias"] = f32(0.004 * (1.0 + rs.randn(C)))
    if n:
        d["parts"] = nan_pad(split_slices(rs, sc * (0.5 + 0.7 * rs.randn(B, C)), n), (n + 1, B, C + 4))
    return d


def final_ln_reference(c, d, mut=None, dt=np.float64):
    C, n = c["C"], c["in_slices"]
    v = d["res"].astype(dt)
    if "bias" in d:
        v = v + d["bias"].astype(dt) * (2 if mut == "bias_twice" else 1)
    if n:
        v = v + (sum_slices(d["parts"][:, :, :C], n, mut) if dt == np.float64 else d["parts"][:n, :, :C].sum(0, dtype=dt))
    eps = 0.0 if mut == "eps_missing" else LN_EPS
    return dict(y=layer_norm(layer_norm(v, d["g1"].astype(dt), d["b1"].astype(dt), eps), d["g2"].astype(dt), d["b2"].astype(dt), eps))


FOLD_CASES = [dict(name="ln_fold_256x300", family="ln_fold", K=256, N=300, bias=True, claims=("fold_swapped",)),
              dict(name="ln_fold_96x256", family="ln_fold", K=96, N=256, bias=False, claims=("fold_swapped",))]
FOLD_BY_NAME = {c["name"]: c for c in FOLD_CASES}


@functools.lru_cache(maxsize=None)
def fold_data(name):
    c = FOLD_BY_NAME[name]
    rs = np.random.RandomState(seed_of(name))
    d = dict(W=weight(c["K"], c["N"], "fold", math.sqrt(c["K"])), gamma=f32(1.0 + 0.3 * rs.randn(c["K"])), beta=f32(0.3 + 0.2 * rs.randn(c["K"])))
    if c["bias"]:
        d["bias"] = f32(rs.randn(c["N"]))
    return d


def fold_reference(c, d, mut=None, dt=np.float64):
    W = d["W"].astype(dt)
    cc, dd = d["gamma"].astype(dt) @ W, d["beta"].astype(dt) @ W + (d["bias"].astype(dt) if "bias" in d else 0)
    return dict(c=dd, d=cc) if mut == "fold_swapped" else dict(c=cc, d=dd)


KV_CASE = dict(name="kv_to_cache_ragged", C=52, L=137, cap=141, lens=(137, 5, 0, 129, 64))       # 137 columns: two 128-thread blocks, neither full


@functools.lru_cache(maxsize=None)
def kv_data():
    c = KV_CASE
    rs = np.random.RandomState(seed_of(c["name"]))
    qkv = f32(rs.randn(len(c["lens"]), 3 * c["C"], c["L"]))
    for b, n in enumerate(c["lens"]):
        qkv[b, :, n:] = np.nan
    return qkv


def kv_reference(c, qkv):
    """-> cache [B, 2 C cap] fp32, NaN where nothing is written: K [C, cap] (row c = qkv row C + c), V [cap, C] (V row t = qkv rows 2 C .., column t)"""
    C, cap = c["C"], c["cap"]
    out = np.full((len(c["lens"]), 2 * C * cap), np.nan, np.float32)
    for b, n in enumerate(c["lens"]):
        out[b, :C * cap].reshape(C, cap)[:, :n] = qkv[b, C:2 * C, :n]
        out[b, C * cap:].reshape(cap, C)[:n] = qkv[b, 2 * C:, :n].T
    return out


# ================================================================================================================= one whole layer
LAYER = dict(name="layer_300keys", family="layer", C=768, H=16, F=3072, B=3, ncs=(300, 212, 7), steps=(40, 0, 3), cap=304,
             claims=("mu_c_dropped", "scale_missing", "new_key_out", "erf_gelu", "bias_twice", "merge_no_rescale"))


@functools.lru_cache(maxsize=None)
def layer_data():
    """a GPT-2 block on the reference shape: x [B, C] (the residual stream in front of it), ln_1, c_attn, the attention's c_proj, ln_2,
    c_fc, the mlp's c_proj, and a planted KV cache"""
    c = LAYER
    rs = np.random.RandomState(seed_of(c["name"]))
    C, F, B = c["C"], c["F"], c["B"]
    ac = attn_case("layer_attn", "fused", c["H"], c["ncs"], c["steps"])
    ac["cap"] = c["cap"]
    d = make_attn_data(ac, rs)
    d.update(attn_case=ac, g2=f32(1.0 + 0.3 * rs.randn(C)), b2=f32(0.2 * rs.randn(C)), bproj=f32(0.2 * rs.randn(768)), Wfc=weight(C, F, "lfc"),
             bfc=f32(0.2 * rs.randn(F)), Wfc2=weight(F, C, "lfc2"), bfc2=f32(0.2 * rs.randn(C)))
    return d


def layer_reference(d, dt=np.float64):
    """HF GPT2Block in one piece: h = x + c_proj(attn(ln_1(x))); out = h + c_proj(gelu_new(c_fc(ln_2(h)))) -> dict(h, out)"""
    c, ac = LAYER, d["attn_case"]
    C, H, D, cap = c["C"], c["H"], HEAD_DIM, c["cap"]
    x = d["x"].astype(dt)
    qkv = layer_norm(x, d["g"].astype(dt), d["b"].astype(dt)) @ d["W"].astype(dt) + d["bias"].astype(dt)
    a = np.zeros_like(x)
    for b, nc in enumerate(c["ncs"]):
        Kc = np.concatenate([d["cache"][b, :C * cap].reshape(C, cap)[:, :nc].astype(dt), qkv[b, C:2 * C, None]], 1)      # [C, n]
        Vc = np.concatenate([d["cache"][b, C * cap:].reshape(cap, C)[:nc].astype(dt), qkv[b, None, 2 * C:]], 0)          # [n, C]
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            a[b, sl] = softmax((qkv[b, sl] @ Kc[sl]) / dt(math.sqrt(D))) @ Vc[:, sl]
    h1 = x + a @ d["wproj"].astype(dt) + d["bproj"].astype(dt)
    m = gelu_new(layer_norm(h1, d["g2"].astype(dt), d["b2"].astype(dt)) @ d["Wfc"].astype(dt) + d["bfc"].astype(dt))
    return dict(h=h1, out=h1 + m @ d["Wfc2"].astype(dt) + d["bfc2"].astype(dt))


def layer_from_kernel_references(d, mut=None, split=False):
    """the same block as the chain computes it, kernel reference by kernel reference in float64 (K1 ressum -> K2 attention (+ K3 merge
    GEMV) -> K4 ressum -> K5 lnparts -> the next K1's residual sum), each reference fed what the one before it gives -> dict(h, out).
    mut: a mutation applied in the kernel it belongs to."""
    c, ac = LAYER, dict(d["attn_case"])
    C, F, H, D, B = c["C"], c["F"], c["H"], HEAD_DIM, c["B"]
    x = d["x"].astype(np.float64)
    g1, W = d["g"].astype(np.float64), d["W"].astype(np.float64)
    # K1: X = x (first layer: no partials), part = (gamma1 . X)^T W_attn, statistics of X
    part = ((g1 * x) @ W)[None]
    stats = np.stack([x.sum(-1), (x ** 2).sum(-1)], -1)[None]
    ac.update(slices=1, stats_slices=1, form="split" if split else "fused", KS=2 if split else 0, CoutP=3 * C)
    ad = dict(d, part=part, stats=stats, fold_c=g1 @ W, fold_d=d["b"].astype(np.float64) @ W + d["bias"].astype(np.float64))
    r = attn_reference(ac, ad, mut if mut in ("mu_c_dropped", "scale_missing", "new_key_out") else "algebra")
    wp = d["wproj"].astype(np.float64)
    if split:                                             # K3: the GP_ATTN GEMV merges the records and projects
        w = np.ones_like(r["rec_m"]) if mut == "merge_no_rescale" else np.exp(r["rec_m"] - r["rec_m"].max(-1, keepdims=True))
        a = ((w[..., None] * r["rec_o"]).sum(2) / (w * r["rec_l"]).sum(2)[..., None]).reshape(B, C)
        proj = a @ wp
    else:
        proj = r["partial"].sum(0)
    # K4: Y = X + b_proj + proj, part = (gamma2 . Y)^T W_fc, statistics of Y
    h1 = x + d["bproj"].astype(np.float64) * (2 if mut == "bias_twice" else 1) + proj
    g2, Wfc = d["g2"].astype(np.float64), d["Wfc"].astype(np.float64)
    mean = h1.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(np.maximum((h1 ** 2).mean(-1, keepdims=True) - mean ** 2, 0.0) + LN_EPS)
    # K5: gelu_new(r (a - mu c) + d)^T W_fc2
    t = rstd * ((g2 * h1) @ Wfc - mean * (g2 @ Wfc)) + (d["b2"].astype(np.float64) @ Wfc + d["bfc"].astype(np.float64))
    m = (gelu_erf(t) if mut == "erf_gelu" else gelu_new(t)) @ d["Wfc2"].astype(np.float64)
    return dict(h=h1, out=h1 + d["bfc2"].astype(np.float64) + m)


# ================================================================================================================= tables
ALL_CASES = GEMV_CASES + ATTN_CASES + FINAL_LN_CASES + FOLD_CASES


def reference_of(c, mut=None, dt=np.float64):
    """(reference outputs) of any case of ALL_CASES"""
    if c in GEMV_CASES:
        return gemv_reference(c, gemv_data(c["name"]), mut, dt)
    if c in ATTN_CASES:
        return attn_reference(c, attn_data(c["name"]), mut, dt)
    if c in FINAL_LN_CASES:
        return final_ln_reference(c, final_ln_data(c["name"]), mut, dt)
    return fold_reference(c, fold_data(c["name"]), mut, dt)


def case_err(c, got, ref):
    return attn_err(c, got, ref) if c in ATTN_CASES else dict_err(got, ref)


def f32_figure(c):
    """the definition evaluated in plain fp32 (numpy's order) against float64, in the case's metric"""
    ref = reference_of(c)
    got = reference_of(c, dt=np.float32)
    if c in ATTN_CASES:                                   # the fp32 pass carries no records: compare what both hold
        keys = ("partial",) if c["form"] == "fused" else ("out",)
        return max([rel_err(got[k], ref[k]) for k in keys] + [rel_err(np.nan_to_num(got["cache"]), np.nan_to_num(ref["cache"]))])
    return dict_err(got, ref)


def gate(c):
    return GATES[c["family"]]


def reached_paths():
    """every path the issue names -> the cases that reach it"""
    reach = {}

    def add(path, name):
        reach.setdefault(path, []).append(name)
    for c in GEMV_CASES:
        r = c["rule"]
        add(f"gemv_{c['shape']}_nb{r['nb']}_{c['pro']}", c["name"])
        add(f"gemv_B{c['B']}", c["name"])
        if r["tail_cols"]:
            add(f"gemv_{c['shape']}_column_tail", c["name"])
        if c["B"] < r["nb"]:
            add(f"gemv_row_clamp_nb{r['nb']}", c["name"])
        if c["pro"] in ("ressum", "lnparts"):
            add(f"in_slices_{c['in_slices']}", c["name"])
            add("sum_" + sum_body(c["in_slices"]), c["name"])
        if c["pro"] == "ressum":
            add(f"lead_writes_{c['shape']}", c["name"])
        if c["pro"] == "lnparts":
            add(f"stats_slices_{c['stats_slices']}", c["name"])
            add("K_ln_differs" if c["K_ln"] != c["K"] else "K_ln_equal", c["name"])
        if c["pro"] == "attn":
            add(f"merge_ks{c['in_slices']}", c["name"])
            if np.isneginf(gemv_data(c["name"])["parts"][..., 0]).any():
                add("merge_empty_split", c["name"])
    for c in ATTN_CASES:
        add(f"attn_{c['form']}" + (f"_ks{c['KS']}" if c["form"] == "split" else ""), c["name"])
        add("sum_" + sum_body(c["slices"]), c["name"])
        if len(set(np.array(c["ncs"]) + 1 - np.array(c["steps"]))) > 1:
            add(f"attn_{c['form']}_ragged_lp", c["name"])
        for nc, st in zip(c["ncs"], c["steps"]):
            add(f"attn_{c['form']}_nc{nc}", c["name"])
            add(f"attn_{c['form']}_step{'0' if st == 0 else 'pos'}", c["name"])
            for p in attention_paths(nc, max(c["KS"], 1)):
                add(f"attn_{c['form']}_{p}", c["name"])
    for c in FINAL_LN_CASES:
        add(f"final_ln_C{c['C']}", c["name"])
        add("final_ln_" + ("parts" if c["in_slices"] else "no_parts"), c["name"])
        add("final_ln_" + ("latents" if c["lat_cs"] else "no_latents"), c["name"])
        add("sum_" + sum_body(c["in_slices"]), c["name"])
    return reach


REQUIRED_PATHS = (
    [f"gemv_{s}_nb{nb}_{p}" for s in SHAPES for nb in (8, 16) for p in ("plain", "ressum", "lnparts", "attn")] +
    [f"gemv_B{b}" for b in (1, 3, 8, 9, 16)] + [f"gemv_{s}_column_tail" for s in ("n64", "wide")] + ["gemv_row_clamp_nb8", "gemv_row_clamp_nb16"] +
    [f"in_slices_{n}" for n in (0, 1, 5, 6, 7, 12, 16, 24)] + [f"sum_unrolled{n}" for n in UNROLLED] + ["sum_rolled_loop_tail", "sum_none"] +
    [f"lead_writes_{s}" for s in SHAPES] + ["stats_slices_1", "stats_slices_6", "K_ln_differs"] + [f"merge_ks{k}" for k in (1, 2, 4, 8)] +
    ["merge_empty_split"] + [f"attn_split_ks{k}" for k in (1, 2, 3, 8)] + ["attn_fused", "attn_split_ragged_lp", "attn_fused_ragged_lp"] +
    [f"attn_{f}_nc{n}" for f in ("split", "fused") for n in NC_ALL] + ["attn_split_empty_split", "attn_split_range_overshoots_nc", "attn_split_new_key_only"] +
    [f"attn_{f}_{p}" for f in ("split", "fused") for p in ("score_loop_nk256", "score_loop_nk257", "score_loop_nk258", "pv_ncl147", "pv_ncl148", "pv_ncl168",
                                                          "pv_ncl169", "pv_two_rounds", "pv_tail_only", "pv_slots20", "pv_slots21", "pv_slots22")] +
    ["attn_fused_step0", "attn_fused_steppos", "attn_split_step0", "attn_split_steppos"] + [f"final_ln_C{n}" for n in (768, 1000, 1024)] +
    ["final_ln_parts", "final_ln_no_parts", "final_ln_latents", "final_ln_no_latents"])

# ---- refusals: (name, entry, changed arguments, a piece of the message)
REJECTS = [
    ("K_not_128", "gemv", dict(K=192), "multiple of 128"),
    ("B_17", "gemv", dict(B=17), "1 .. 16 batch rows"),
    ("CoutP_not_4", "gemv", dict(CoutP=66), "multiple of 4"),
    ("D_32", "attn", dict(dim=32), "head dim 48"),
    ("cap_beyond_lds", "attn", dict(cap=16384), "LDS score buffer"),
    ("wproj_512", "attn", dict(wproj_cols=512), "768 columns"),
]
