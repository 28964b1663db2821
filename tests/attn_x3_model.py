"""The trunk's split-precision attention path in numpy: qkv conv with the operand-image epilogue (csrc/conv_x3.hip, EPI 2) ->
flash_attn_x3b_kernel (csrc/attention_x3b.hip) -> output planes.  Shared by tests/test_gpu_attn_x3.py (through Runtime.op_attention_x3)
and tests/test_host_attn_x3.py:
  * the AttnPlanes image and the output planes, encoded / decoded from the layout COMMENTS of csrc/attention.h and csrc/conv_x3.h;
  * the float64 reference out[h, :, t] = sum_s softmax_s(q_t . k_s / sqrt(48) + tab[h][clamp(s - t, -64, 64) + 64]) v_s, s < len;
  * plan(): a Python restatement of the kernel's per-wave loop partition (jA, jB, jM, e1, e2).  It is a RESTATEMENT: it can drift from the
    kernel; its job is to choose and label the GPU cases (which loops run for which waves), and test_host_attn_x3.py checks its
    properties exhaustively;
  * emulate(): the arithmetic scheme with a switch per single mutation (MUTATIONS);
  * the case table with planted data (bias pointers, score pointers) and precision data (score std 0.6 / 2 / 5, growing scores).

What emulate() models: the conv's two-plane operands and three products (conv_x3_model), its fp32 result, Q / K / V rounded to two fp16
planes with the kernels' scales (Q: log2(e) / sqrt(48) * 16, K and V: 16), the cross products kept, the fp32 exponent argument s / 256 +
bias * log2(e), the lazy running maximum with its 2^3 slack per 32-key block, P = exp2(e - m + 10) split in two planes, the denominator
from the same planes (the "ones" fragment: 16 (P0 + P1)), and the output split.  What it leaves out: fp32 accumulation (order and
rounding: products are summed in float64), the hardware exp2 (float64 exp2 rounded to fp32), the FAR loop's fused form of the exponent
(fma(s, 1 / 256, bias - m) instead of (s / 256 + bias) - m), and the key split's merge (S > 1 changes only which maximum each range's
P were taken against)."""
import zlib

import numpy as np

import conv_x3_model as CM

D, KT, QPW, CLIP = 48, 64, 32, 64
GATE = CM.GATE                      # 2e-5: stands because the scheme is <= GATE / 10 and every claimed mutation >= 3 GATE (test_host_attn_x3.py)
# The one-product mode rounds x, w (in the conv), then Q, K, V and P to ONE fp16 plane each: 2^-11 = 4.9e-4 relative per rounding.  V's
# and P's enter the output directly, Q's and K's through the exponent (x the score's magnitude, O(1) on the p1 cases: score std 0.6 and
# one-key pointers), the conv's through all three: a handful of independent 4.9e-4 roundings of O(1) values, ~ 1e-3 in all.  The gate is
# 5 x that; test_host_attn_x3.py holds the emulated one-product scheme under P1_GATE / 10 (it gives 3 - 5e-4) and above GATE.
P1_GATE = 5e-3
LOG2E = float(np.float32(1.4426950408889634))
QSCALE = float(np.float32(np.float32(1.0 / np.sqrt(np.float32(48.0))) * np.float32(1.4426950408889634)))      # qkv_qscale of the launch
TILE_BYTES = 2 * (6 * 64 + 8 * 48) * 16


def tq(T):
    return -(-T // KT) * KT


def nt64(T):
    return -(-T // KT)


def head_bytes(T):
    return 2 * 6 * tq(T) * 16 + nt64(T) * TILE_BYTES


def image_bytes(B, H, T):
    return B * H * head_bytes(T)


def x3_tp(T):
    return -(-T // 192) * 192 + 2


# V chunk (u, j, hh, channel) holds keys 32 u + 16 j + 4 hh + {0..3, 8..11} of that channel (attention.h)
V_KEYS = np.array([[[[32 * u + 16 * j + 4 * hh + o for o in (0, 1, 2, 3, 8, 9, 10, 11)] for hh in range(2)] for j in range(2)] for u in range(2)])


# ---- layouts
def decode_image(raw, B, H, T):
    """raw bytes of AttnPlanes::bytes(B, H, T) -> (q [B, H, 2, 48, Tq], k [B, H, 2, 48, 64 nt], v [same]) as uint16 bit patterns of fp16.
    Per (sample, head): Q [plane 2][c8 6][Tq] chunks of 8 channels; then per 64-key tile K [plane 2][c8 6][key 64] chunks of 8 channels
    and V [plane 2][u 2][j 2][hh 2][channel 48] chunks of 8 KEYS (V_KEYS)."""
    a = np.frombuffer(raw, np.uint16).reshape(B, H, head_bytes(T) // 2)
    Tq, nt = tq(T), nt64(T)
    nq = 2 * 6 * Tq * 8
    q = a[:, :, :nq].reshape(B, H, 2, 6, Tq, 8).transpose(0, 1, 2, 3, 5, 4).reshape(B, H, 2, 48, Tq)
    tiles = a[:, :, nq:].reshape(B, H, nt, TILE_BYTES // 2)
    nk = 2 * 6 * 64 * 8
    k = tiles[..., :nk].reshape(B, H, nt, 2, 6, 64, 8).transpose(0, 1, 3, 4, 6, 2, 5).reshape(B, H, 2, 48, nt * 64)
    vc = tiles[..., nk:].reshape(B, H, nt, 2, 2, 2, 2, 48, 8)                 # tile, plane, u, j, hh, channel, slot
    v = np.zeros((B, H, 2, 48, nt, 64), np.uint16)
    for u in range(2):
        for j in range(2):
            for hh in range(2):
                v[:, :, :, :, :, V_KEYS[u, j, hh]] = vc[:, :, :, :, u, j, hh].transpose(0, 1, 3, 4, 2, 5)
    return np.ascontiguousarray(q), np.ascontiguousarray(k), v.reshape(B, H, 2, 48, nt * 64)


def encode_image(q, k, v, T):
    """inverse of decode_image (uint16 arrays) -> bytes; the host test round-trips the two"""
    B, H = q.shape[:2]
    Tq, nt = tq(T), nt64(T)
    qa = q.reshape(B, H, 2, 6, 8, Tq).transpose(0, 1, 2, 3, 5, 4).reshape(B, H, -1)
    ka = k.reshape(B, H, 2, 6, 8, nt, 64).transpose(0, 1, 5, 2, 3, 6, 4).reshape(B, H, nt, -1)
    v6 = v.reshape(B, H, 2, 48, nt, 64)
    vc = np.zeros((B, H, nt, 2, 2, 2, 2, 48, 8), np.uint16)
    for u in range(2):
        for j in range(2):
            for hh in range(2):
                vc[:, :, :, :, u, j, hh] = v6[:, :, :, :, :, V_KEYS[u, j, hh]].transpose(0, 1, 4, 2, 3, 5)
    tiles = np.concatenate([ka, vc.reshape(B, H, nt, -1)], axis=-1).reshape(B, H, -1)
    return np.ascontiguousarray(np.concatenate([qa, tiles], axis=-1)).tobytes()


def f16(bits):
    return np.ascontiguousarray(bits).view(np.float16).astype(np.float64)


def decode_out_planes(raw, B, H, T):
    """raw bytes of the planes [B][6 H][2][x3_tp(T)][8 fp16] (conv_x3.h; value x 16 = plane 0 + plane 1, column t + 1)
    -> (y [B, 48 H, T] float64, the raw uint16 array [B, 6 H, 2, Tp, 8])"""
    Tp = x3_tp(T)
    a = np.frombuffer(raw, np.uint16).reshape(B, 6 * H, 2, Tp, 8)
    val = (f16(a[:, :, 0]) + f16(a[:, :, 1])) / CM.SCALE_X                 # [B, 6 H, Tp, 8]
    y = val[:, :, 1: T + 1].transpose(0, 1, 3, 2).reshape(B, 48 * H, T)
    return y, a


# ---- float64 reference
def qkv64(w, b, x):
    """rows 144 h + [q 48 | k 48 | v 48] (QKVAttentionLegacy) of the 1 x 1 conv -> q, k, v [H, 48, L] float64"""
    y = np.asarray(w, np.float64) @ np.asarray(x, np.float64) + np.asarray(b, np.float64)[:, None]
    y = y.reshape(-1, 3, D, x.shape[1])
    return y[:, 0], y[:, 1], y[:, 2]


def bias_index(L, lo=-CLIP, hi=CLIP, shift=0):
    t = np.arange(L)
    return np.clip(t[None, :] - t[:, None] + shift, lo, hi) + CLIP           # [t, s]


def attention64(q, k, v, tab):
    L = q.shape[2]
    s = np.einsum("hct,hcs->hts", q, k) / np.sqrt(48.0) + np.asarray(tab, np.float64)[:, bias_index(L)]
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return np.einsum("hts,hcs->hct", p, v)


def reference(d, bi):
    """-> out [48 H, len] float64 of sample bi"""
    L = d["lens"][bi]
    q, k, v = qkv64(d["w"], d["b"], d["x"][bi, :, :L])
    return attention64(q, k, v, d["tab"]).reshape(-1, L)


def score_margin(d, bi):
    """nats between the best and the second-best key of every query (score-pointer cases assert >= 10)"""
    L = d["lens"][bi]
    q, k, _ = qkv64(d["w"], d["b"], d["x"][bi, :, :L])
    s = np.sort(np.einsum("hct,hcs->hts", q, k) / np.sqrt(48.0) + np.asarray(d["tab"], np.float64)[:, bias_index(L)], axis=-1)
    return float((s[..., -1] - s[..., -2]).min()) if L > 1 else np.inf


# ---- the kernel's per-wave plan, restated
FAR, GEN = "far", "general"


def plan(tq0, length, ntiles, boff):
    """Wave with queries tq0 .. tq0 + 31 of a sample of `length` keys, on the key range of `ntiles` 64-key tiles whose first 32-key block
    has absolute index boff.  Block 0 and block 2 ntiles - 1 run in the general prologue / epilogue steps; iteration j = 1 .. ntiles - 1
    runs blocks 2 j - 1 and 2 j, in four loops [1, e1) FAR (below), [e1, e2) general (the band), [e2, jM) FAR (above), [jM, ntiles)
    general (masked tail)."""
    rel = lambda v: max(v - boff, 0)
    b_lo_end = rel((tq0 - CLIP - 31) // 32 + 1 if tq0 - CLIP - 31 >= 0 else 0)
    b_hi_beg = rel((tq0 + QPW - 1 + CLIP + 31) // 32)
    bmask = rel(length // 32)
    clampj = lambda v: min(max(v, 1), ntiles)
    jA, jB, jM = clampj((b_lo_end + 1) // 2), clampj((b_hi_beg + 2) // 2), clampj((bmask + 1) // 2)
    e1 = min(jA, jM)
    e2 = min(max(jB, e1), jM)
    return dict(jA=jA, jB=jB, jM=jM, e1=e1, e2=e2, loops=((1, e1, FAR), (e1, e2, GEN), (e2, jM, FAR), (jM, ntiles, GEN)))


def split_ranges(length, S):
    """(first tile, tiles) of each of the S key ranges"""
    n = nt64(length)
    return [(z * n // S, (z + 1) * n // S - z * n // S) for z in range(S)]


def block_side(tq0, ablk):
    """absolute 32-key block against the wave's queries: -1 wholly beyond -64, +1 wholly beyond +64, 0 near"""
    s0 = 32 * ablk
    if s0 - (tq0 + QPW - 1) >= CLIP:
        return 1
    if s0 + 31 - tq0 <= -CLIP:
        return -1
    return 0


def labels(c, S=1):
    """what the case exercises, over its samples, waves and key ranges: a set of strings (see test_host_attn_x3.py coverage)"""
    out = set()
    for L in c["lens"]:
        nwav = -(-c["T"] // 128) * 4
        act = [32 * w for w in range(nwav) if 32 * w < L]
        if any(32 * w >= L and (32 * w) // 128 * 128 < L for w in range(nwav)):
            out.add("idle_wave_beside_active")
        if nt64(L) == 1:
            out.add("single_tile")
        if nt64(L) < S:
            out.add("ntiles_lt_S")
        for jt0, n in split_ranges(L, S):
            if n == 0:
                out.add("empty_range")
                continue
            for tq0 in act:
                p = plan(tq0, L, n, 2 * jt0)
                for i, (a, b, _) in enumerate(p["loops"]):
                    out.add(f"loop{i}_{'run' if b > a else 'empty'}")
                if n > 1:
                    for nm, eq in (("jA=jM", p["jA"] == p["jM"]), ("jB=jM", p["jB"] == p["jM"]), ("e1=e2", p["e1"] == p["e2"])):
                        if eq:
                            out.add(nm)
    return out


# ---- cases
MUTATIONS = ("qk_k1q0", "qk_k0q1", "pv_v1p0", "pv_v0p1", "p_low", "q_low_tile", "k_low_tile", "v_low_tile", "skip_rescale", "bias_off1",
             "clamp63", "bias_swap", "mask_last", "admit_invalid", "v_swap")
PLACEMENT = ("bias_off1", "mask_last", "admit_invalid", "v_swap")
LOW = ("qk_k1q0", "qk_k0q1", "pv_v1p0", "pv_v0p1", "p_low")


def case(name, kind, H, cin, T, lens, *, claims, std=0.0, offsets=None, ksplit=(1,), p1=False, fp32_form=False):
    return dict(name=name, kind=kind, H=H, cin=cin, T=T, lens=list(lens), claims=tuple(claims), std=std, offsets=offsets, ksplit=tuple(ksplit),
                p1=p1, fp32_form=fp32_form)


CASES = [
    # (b) bias pointers: all scores 0, head h's table = small noise + 20 at offset o*_h
    case("bias_ptr_h8", "bias_ptr", 8, 64, 333, [333, 193, 128, 63], offsets=[-64, -63, -33, -32, -1, 0, 1, 31],
         claims=PLACEMENT + ("clamp63", "bias_swap", "skip_rescale")),
    case("bias_ptr_h3_b1", "bias_ptr", 3, 32, 200, [200], offsets=[32, 63, 64], claims=PLACEMENT + ("clamp63", "bias_swap", "skip_rescale"), fp32_form=True,
         ksplit=(1, 2)),
    # (b) score pointers: q of query t matches the code of key pi(t) with >= 10 nats over the runner-up; flat table
    case("score_ptr_T384", "score_ptr", 2, 96, 384, [384, 191, 65, 1], claims=("mask_last", "v_swap"), p1=True),
    case("score_ptr_split_T700", "score_ptr", 2, 96, 700, [700, 100], claims=("mask_last", "v_swap"), ksplit=(1, 2, 3, 4)),
    # (c) precision: random data, score std (nats) 0.6 = the synthetic weights' regime, 2, 5; random O(1) table
    # (at std 0.6 a dropped low plane of P - alone or with the V0 P1 product - stays at 5.0e-5, under 3 GATE: claimed from std 2 on)
    case("prec_std0.6", "prec", 4, 64, 257, [257, 192, 127, 31], std=0.6,
         claims=("qk_k1q0", "qk_k0q1", "pv_v1p0", "q_low_tile", "k_low_tile", "v_low_tile", "bias_swap") + PLACEMENT, p1=True, fp32_form=True),
    case("prec_std2", "prec", 4, 64, 320, [320, 129, 64, 32], std=2.0,
         claims=LOW + ("q_low_tile", "k_low_tile", "v_low_tile", "bias_swap", "clamp63") + PLACEMENT),
    case("prec_std5_table", "prec_table", 4, 48, 200, [200, 193, 128, 33], std=5.0, claims=LOW + ("q_low_tile", "k_low_tile", "v_low_tile")),
    case("prec_ramp_split_T700", "ramp", 4, 64, 700, [700, 90], std=1.0, claims=LOW + ("skip_rescale",), ksplit=(1, 2, 3, 4)),
    # the production head count: 18 M tiles of the qkv conv (the EPI 2 tile-order remap), 16 heads over the XCDs
    case("prec_h16_cin768", "prec", 16, 768, 130, [130, 64], std=0.6, claims=("p_low", "pv_v0p1")),
]


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


def pointer_targets(L, T):
    """pi(t) for the score-pointer cases: key 0, len - 1, both sides of every 32 / 64 seam near the query, distance 63 / 64 / 65 on both
    sides, and the first and last key of every key-split range (S = 2 .. 4), cycled over the queries"""
    t = np.arange(L)
    edges = sorted({64 * jt0 for S in (2, 3, 4) for jt0, n in split_ranges(L, S) if n} | {64 * (jt0 + n) - 1 for S in (2, 3, 4) for jt0, n in split_ranges(L, S) if n})
    cand = [np.zeros(L, int), np.full(L, L - 1), t // 32 * 32 - 1, t // 32 * 32, t // 32 * 32 + 31, t // 32 * 32 + 32, t // 64 * 64 - 1, t // 64 * 64 + 64,
            t - 63, t - 64, t - 65, t + 63, t + 64, t + 65] + [np.full(L, e) for e in edges]
    pi = np.stack(cand)[(t * 7 + t // 32) % len(cand), t]
    return np.clip(pi, 0, L - 1)


def make_data(c):
    """-> dict(x [B, cin, T] (random beyond each length), w [144 H, cin], b [144 H], tab [H, 129], lens); fp32, seeded per case"""
    rs = np.random.RandomState(seed_of(c["name"]))
    H, cin, T, lens = c["H"], c["cin"], c["T"], c["lens"]
    B = len(lens)
    x = rs.randn(B, cin, T).astype(np.float32)
    w = np.zeros((H, 3, D, cin), np.float32)
    b = np.zeros((H, 3, D), np.float32)
    w[:, 2] = rs.randn(H, D, cin) / np.sqrt(cin)
    b[:, 2] = rs.randn(H, D)
    tab = np.zeros((H, 2 * CLIP + 1), np.float32)
    if c["kind"] == "bias_ptr":
        tab[:] = rs.randn(H, 2 * CLIP + 1) * 0.05
        for h, o in enumerate(c["offsets"]):
            tab[h, o + CLIP] = 20.0
    elif c["kind"] == "score_ptr":
        # channels 0..47: the key's own +-1 code; 48..95: the code of the query's target pi(t).  q reads the second group, k the first,
        # with a gain chosen from the data so that the runner-up is >= 10.5 nats below (score_margin re-checks it in the host test)
        assert cin == 2 * D
        for bi, L in enumerate(lens):
            code = np.where(rs.rand(D, T) < 0.5, -1.0, 1.0).astype(np.float32)
            x[bi, :D] = code
            x[bi, D:, :L] = code[:, pointer_targets(L, T)]
        worst = max(float(np.max(x[bi, :D, :L].T @ x[bi, :D, :L] - 2 * D * np.eye(L))) for bi, L in enumerate(lens))
        gain = np.float32(np.sqrt(10.5 * np.sqrt(D) / (D - worst)))
        for h in range(H):
            sign = np.where(rs.rand(D) < 0.5, -1.0, 1.0)
            w[h, 0, np.arange(D), D + np.arange(D)] = gain * sign
            w[h, 1, np.arange(D), np.arange(D)] = gain * sign
        w[:, 2] = rs.randn(H, D, cin) / np.sqrt(cin)
    else:
        g = np.sqrt(c["std"])
        w[:, 0] = rs.randn(H, D, cin) * g / np.sqrt(cin)
        w[:, 1] = rs.randn(H, D, cin) * g / np.sqrt(cin)
        b[:, 0] = rs.randn(H, D) * 0.1
        b[:, 1] = rs.randn(H, D) * 0.1
        if c["kind"] == "prec_table":
            from detail_tts_amd.packing import bias_table            # the production table builder in the loop
            tab = bias_table((rs.randn(32, H) / np.sqrt(D)).astype(np.float32), D)
        else:
            tab[:] = rs.randn(H, 2 * CLIP + 1)
        if c["kind"] == "ramp":          # test_attention_block_with_growing_scores_rescales_mid_sequence: later frames ~9 x larger
            x *= (0.3 + 2.7 * np.arange(T) / T).astype(np.float32)[None, None, :]
    return dict(x=x, w=np.ascontiguousarray(w.reshape(3 * D * H, cin)), b=np.ascontiguousarray(b.reshape(-1)), tab=np.ascontiguousarray(tab, np.float32),
                lens=list(lens))


# ---- the arithmetic scheme
def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def conv_scheme(d, bi, p1=False):
    """the qkv conv as the kernel computes it (two planes, three products - p1: one -, float64 sums), its fp32 result -> [144 H, L]"""
    L = d["lens"][bi]
    xs, ws = CM.split(d["x"][bi, :, :L], CM.SCALE_X), CM.split(d["w"], CM.SCALE_W)
    terms = ((0, 0),) if p1 else CM.ALL_TERMS
    acc = sum(ws[pw] @ xs[px] for pw, px in terms) / (CM.SCALE_X * CM.SCALE_W)
    return f32(acc + d["b"].astype(np.float64)[:, None])


def operand_planes(d, bi, p1=False):
    """-> (Q, K, V): each a pair of [H, 48, L] float64 arrays holding the fp16 plane values the image must carry for keys / queries < len"""
    y = conv_scheme(d, bi, p1).reshape(-1, 3, D, d["lens"][bi])
    return (CM.split(np.float32(y[:, 0]) * np.float32(QSCALE * 16.0), 1.0), CM.split(y[:, 1], 16.0), CM.split(y[:, 2], 16.0))


def emulate(d, bi, mut=None, p1=False, fp32_form=False):
    """the scheme for sample bi -> out [48 H, len] float64; mut: one of MUTATIONS"""
    assert mut is None or mut in MUTATIONS
    L = d["lens"][bi]
    H = d["tab"].shape[0]
    (q0, q1), (k0, k1), (v0, v1) = operand_planes(d, bi, p1)
    Lp = tq(L) + KT                                                            # keys >= len hold zeros (one spare tile: admit_invalid at len % 64 == 0)
    pad = lambda a: np.concatenate([a, np.zeros((H, D, Lp - L))], axis=2)
    k0, k1, v0, v1 = pad(k0), pad(k1), pad(v0), pad(v1)
    mid = (L // 2) // KT * KT
    if mut == "q_low_tile":
        q1 = q1.copy(); q1[:, :, mid: mid + KT] = 0.0
    if mut == "k_low_tile":
        k1[:, :, mid: mid + KT] = 0.0
    if mut == "v_low_tile":
        v1[:, :, mid: mid + KT] = 0.0
    if mut == "v_swap" and L > 1:
        s = min(L - 2, mid + 36) // 2 * 2                                       # s, s + 1: one 32-key block
        for a in (v0, v1):
            a[:, :, [s, s + 1]] = a[:, :, [s + 1, s]]
    qk_terms = [(1, 0), (0, 1), (0, 0)]                                          # (K plane, Q plane), smallest first
    pv_terms = [(1, 0), (0, 1), (0, 0)]                                          # (V plane, P plane)
    if p1:
        qk_terms = pv_terms = [(0, 0)]
    if mut == "qk_k1q0": qk_terms.remove((1, 0))
    if mut == "qk_k0q1": qk_terms.remove((0, 1))
    if mut == "pv_v1p0": pv_terms.remove((1, 0))
    if mut == "pv_v0p1": pv_terms.remove((0, 1))
    K, Q, V = (k0, k1), (q0, q1), (v0, v1)
    tabl = f32(np.float32(d["tab"]) * np.float32(LOG2E))                        # [H, 129], log2 domain, fp32
    t = np.arange(L)
    tq0 = t // QPW * QPW
    valid = L + 1 if mut == "admit_invalid" else L
    O, l, m = np.zeros((H, D, L)), np.zeros((H, L)), np.full((H, L), -np.inf)
    skipped = False
    for blk in range(2 * nt64(L)):
        s = np.arange(32 * blk, 32 * blk + 32)
        acc = sum(np.matmul(Q[b].transpose(0, 2, 1), K[a][:, :, s]) for a, b in qk_terms)          # [H, t, s]
        dlt = s[None, :] - t[:, None]
        idx = np.clip(dlt + (1 if mut == "bias_off1" else 0), -(63 if mut == "clamp63" else CLIP), 63 if mut == "clamp63" else CLIP) + CLIP
        if mut == "bias_swap":
            idx = np.where((s[0] - (tq0 + QPW - 1) >= CLIP)[:, None], 0, np.where((s[0] + 31 - tq0 <= -CLIP)[:, None], 2 * CLIP, idx))
        e = f32(f32(acc / 256.0) + tabl[:, idx])
        dead = s >= valid
        if mut == "mask_last" and L > 1:
            dead = dead | (s == L - 1)
        e[:, :, dead] = -np.inf
        mx = e.max(-1)
        upd = mx > m + 3.0
        alpha = np.where(upd, f32(np.exp2(m - np.where(upd, mx, 0.0))), 1.0)      # exp2(m_run - m_new); 0 while m_run = -inf
        if mut == "skip_rescale" and not skipped and blk >= 1 and np.any(upd & np.isfinite(m)):
            skipped = True
        else:
            O *= alpha[:, None, :]
            l *= alpha
        m = np.where(upd, mx, m)
        msub = np.where(np.isfinite(m), m, 0.0) - 10.0
        p = f32(np.exp2(f32(e - msub[:, :, None])))
        pp0 = np.float16(p).astype(np.float64)
        pp1 = np.float16(np.float32(p - pp0)).astype(np.float64)
        if mut == "p_low":
            pp1 = np.zeros_like(pp1)
        P = (pp0, pp1)
        for a, b in pv_terms:
            O += np.matmul(V[a][:, :, s], P[b].transpose(0, 2, 1))
            if a == 0:
                l += 16.0 * P[b].sum(-1)                                            # the ones fragment: plane 0 = 16, plane 1 = 0
    out = f32(O * f32(1.0 / l)[:, None, :])                                          # 16384 O / (16 * 1024 l)
    if not fp32_form:
        h0, h1 = CM.split(out, CM.SCALE_X)
        out = (h0 + h1) / CM.SCALE_X
    return out.reshape(-1, L)


def rel_err(y, ref):
    """the metric of the precision gate: max |y - ref| / max(1, max |ref|)"""
    return float(np.max(np.abs(y - ref))) / max(1.0, float(np.max(np.abs(ref))))


# ---- what op_attention_x3 accepts; REJECTS: kwargs on top of a plain H = 2, Cin = 32, T = 100, lens [100, 50] call
REJECTS = [          # (name, kwargs, what the refusal says)
    ("cin24", dict(cin=24), "op_attention_x3"),
    ("p1_cin48", dict(cin=48, p1=1), "op_attention_x3"),
    ("len_beyond_T", dict(lens=[100, 101]), "op_attention_x3"),
    ("len_negative", dict(lens=[-1, 50]), "op_attention_x3"),
    ("heads_0", dict(H=0), "op_attention_x3"),
    ("heads_mismatch", dict(H_arg=3), "weight 't.wp': expected"),          # the packed weight holds 144 * 2 rows
    ("p1_2", dict(p1=2), "op_attention_x3"),
]


def eligible(cin, H, T, lens, p1=0, H_arg=None):
    ok = cin > 0 and cin % 16 == 0 and 1 <= H <= 64 and (H_arg is None or H_arg == H) and 0 < T <= (1 << 16) and p1 in (0, 1)
    ok = ok and all(0 <= n <= T for n in lens) and (not p1 or cin % 32 == 0)
    return bool(ok)
