"""The split-precision conv (csrc/conv_x3.hip) in numpy: the case table of tests/test_gpu_conv_x3.py, its data, its float64 references,
and an emulation of the two-plane split with the three (or, p1, one) products - shared by the GPU test and by tests/test_host_conv_x3.py,
which shows on the CPU that the 2e-5 gate separates the scheme from each seeded fault.

Arithmetic emulated (csrc/split3.h, csrc/conv_x3.h): v = clamp(fp32(a) * s, +-65504); h0 = fp16(v) (nearest-even); h1 = fp16(v - fp32(h0))
(the difference is exact in fp32); s = 16 for activations, 64 for weights.  The kernel accumulates h0 h0' + h0 h1' + h1 h0' (p1: h0 h0' alone)
in fp32 and multiplies by 1 / 1024; the emulation accumulates the same products in float64, so what it measures is the scheme's own error
(the dropped h1 h1' term and the 22-bit operands), not a summation order."""
import zlib

import numpy as np

GATE = 2e-5
SLOPE = float(np.float32(0.1))          # op_conv1d_x3's leaky-relu slope (0.1f)
ACT_SILU, ACT_LRELU, ACT_TANH = 1, 2, 5
BM, BN = 128, 192                       # the kernel's tile: output rows x columns
SCALE_X, SCALE_W = 16.0, 64.0


# ---- cases.  Every case states the variant it was written for: epi (0 bias (+ res), 1 activation / scale, 4 gated), kw3, ksplit,
# epi_vec (1: LDS-staged 16-byte stores), cols (1: live-column table attached).  tests/test_host_conv_x3.py checks these against the
# launcher's rule written out in Python; tests/test_gpu_conv_x3.py against what the launcher reports.
def case(name, cin, cout, k, T, *, epi, ksplit, epi_vec, cols=1, act=0, scale=1.0, res=False, gate=0, badd=False, p1=0, cap=0, lens=None):
    return dict(name=name, cin=cin, cout=cout, k=k, T=T, epi=epi, kw3=int(k == 3), ksplit=ksplit, epi_vec=epi_vec, cols=cols, act=act, scale=scale,
                res=res, gate=gate, badd=badd, p1=p1, cap=cap, lens=lens)


CASES = []
# K-loop length against the prefetch distance D = stages - 1 = 1 .. 3: 1 .. 4 channel blocks (k = 1: 1 .. 4 steps, k = 3: 3 .. 12); the
# second N tile holds ONE column
for _k in (1, 3):
    for _cin in (16, 32, 48, 64):
        CASES.append(case(f"kloop_k{_k}_cin{_cin}", _cin, 128, _k, 193, epi=0, ksplit=1, epi_vec=0))
# padded rows (CoutP = 256: rows 200 .. 255 write nothing); T = 385: scalar epilogue, T = 388: LDS-staged 16-byte stores
for _k, _s in ((1, 2), (3, 4)):
    CASES.append(case(f"rows200_k{_k}_T385", 768, 200, _k, 385, epi=0, ksplit=_s, epi_vec=0))
    CASES.append(case(f"rows200_k{_k}_T388", 768, 200, _k, 388, epi=0, ksplit=_s, epi_vec=1))
# split-K: 48 channel blocks over 4, 25 over 3 (8 / 8 / 9), 17 over 2 (8 / 9), k = 1: at most 2; each again with the cap at 1
for _nm, _cin, _k, _s in (("cin768_k3", 768, 3, 4), ("cin400_k3", 400, 3, 3), ("cin272_k3", 272, 3, 2), ("cin768_k1", 768, 1, 2)):
    CASES.append(case(f"splitk_{_nm}", _cin, 128, _k, 385, epi=0, ksplit=_s, epi_vec=0))
    CASES.append(case(f"splitk_{_nm}_cap1", _cin, 128, _k, 385, epi=0, ksplit=1, epi_vec=0, cap=1))
# epilogues.  EPI 0 with a residual, both store forms (without: every case above)
CASES += [
    case("epi0_res_k3_T385", 128, 200, 3, 385, epi=0, ksplit=1, epi_vec=0, res=True),
    case("epi0_res_k3_T388", 128, 200, 3, 388, epi=0, ksplit=1, epi_vec=1, res=True),
    case("epi0_res_k1_T388_splitk", 256, 200, 1, 388, epi=0, ksplit=2, epi_vec=1, res=True),
    # EPI 1: activation, then out_scale = 0.5, then the residual
    case("epi1_lrelu_k1_T385", 128, 200, 1, 385, epi=1, ksplit=1, epi_vec=0, act=ACT_LRELU, scale=0.5, res=True),
    case("epi1_lrelu_k3_T388", 128, 200, 3, 388, epi=1, ksplit=1, epi_vec=1, act=ACT_LRELU, scale=0.5, res=True),
    case("epi1_silu_k3_T385", 256, 128, 3, 385, epi=1, ksplit=2, epi_vec=0, act=ACT_SILU, scale=0.5, res=True),
    case("epi1_silu_k1_T388", 128, 200, 1, 388, epi=1, ksplit=1, epi_vec=1, act=ACT_SILU, scale=0.5, res=True),
    case("epi1_tanh_k1_T385", 128, 128, 1, 385, epi=1, ksplit=1, epi_vec=0, act=ACT_TANH, scale=0.5, res=True),
    case("epi1_tanh_k3_T388", 128, 200, 3, 388, epi=1, ksplit=1, epi_vec=1, act=ACT_TANH, scale=0.5, res=True),
    case("epi1_scale_only_k3_T388", 128, 128, 3, 388, epi=1, ksplit=1, epi_vec=1, scale=0.5),
    # EPI 4: tanh * sigmoid over gate_perm-packed row pairs, 1 x 1 conv, Cout = 256 -> 128 output rows (needs 16-byte aligned rows)
    case("epi4_gate_T388", 192, 256, 1, 388, epi=4, ksplit=1, epi_vec=1, gate=1),
    case("epi4_gate_badd_T388", 192, 256, 1, 388, epi=4, ksplit=1, epi_vec=1, gate=1, badd=True),
    case("epi4_gate_badd_rows300_T388", 256, 300, 1, 388, epi=4, ksplit=2, epi_vec=1, gate=1, badd=True),
    # live-column table: lengths [385, 192, 193, 1] leave 7 of 12 (sample, N tile) columns
    case("cols_k3_cin768", 768, 128, 3, 385, epi=0, ksplit=4, epi_vec=0, cols=1, lens=[385, 192, 193, 1]),
    # no table: every sample reaches the third tile
    case("nocols_k3_cin768", 768, 128, 3, 385, epi=0, ksplit=4, epi_vec=0, cols=0, lens=[385, 385, 385, 385]),
]
# one-product mode: 32 channels per K-step (Cin = 32: a single step for k = 1)
for _k in (1, 3):
    for _cin in (32, 64, 96, 768):
        _s = 1 if _cin < 768 else (2 if _k == 1 else 4)
        CASES.append(case(f"p1_k{_k}_cin{_cin}", _cin, 128, _k, 193 if _cin < 768 else 385, epi=0, ksplit=_s, epi_vec=0, p1=1))
CASES += [
    case("p1_epi1_lrelu_k1_T388", 64, 128, 1, 388, epi=1, ksplit=1, epi_vec=1, act=ACT_LRELU, scale=0.5, res=True, p1=1),
    case("p1_epi1_tanh_k3_T385", 96, 200, 3, 385, epi=1, ksplit=1, epi_vec=0, act=ACT_TANH, scale=0.5, res=True, p1=1),
]

# what op_conv1d_x3 must refuse on the host (kwargs of Runtime.op_conv1d_x3 on top of a plain k = 1, Cin = 64, Cout = 128, T = 196 conv)
REJECTS = [
    ("cout50", dict(cout=50)),
    ("cin24", dict(cin=24)),
    ("k5", dict(k=5)),
    ("gate_k3", dict(cout=256, k=3, gate=1)),
    ("gate_res", dict(cout=256, gate=1, res=True)),
    ("gate_T_not_multiple_of_4", dict(cout=256, gate=1, T=385)),
    ("p1_cin48", dict(cin=48, p1=1)),
]


def lens_of(c):
    """T, the largest multiple m of the N tile with m + 1 < T, m + 1, and 1 (one tile: T, T - 1, 2, 1)"""
    if c["lens"]:
        return list(c["lens"])
    T = c["T"]
    m = (T - 2) // BN * BN
    return [T, m, m + 1, 1] if m > 0 else [T, T - 1, 2, 1]


def gate_perm(rows):
    half = rows // 2
    return np.stack([np.arange(half), np.arange(half) + half], 1).reshape(-1)


def make_data(c):
    """w ~ N(0, 1 / (cin k)), x ~ N(0, 1) (random beyond each length too), b ~ N(0, 1); res / badd ~ N(0, 1).  Seeded per case."""
    rs = np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7fffffff)
    cin, cout, k, T = c["cin"], c["cout"], c["k"], c["T"]
    rows = cout // 2 if c["gate"] else cout
    d = dict(w=(rs.randn(cout, cin, k) / np.sqrt(cin * k)).astype(np.float32), b=rs.randn(cout).astype(np.float32),
             x=rs.randn(4, cin, T).astype(np.float32), lens=lens_of(c))
    d["res"] = rs.randn(4, rows, T).astype(np.float32) if c["res"] else None
    d["badd"] = rs.randn(4, cout).astype(np.float32) if c["badd"] else None      # in the conv's own row order (a | b halves)
    return d


# ---- float64 arithmetic
def act64(v, act):
    if act == ACT_LRELU:
        return np.where(v >= 0, v, v * SLOPE)
    if act == ACT_SILU:
        return v / (1.0 + np.exp(-v))
    if act == ACT_TANH:
        return np.tanh(v)
    assert act == 0
    return v


def conv64(x, w, skip=None):
    """x [cin, L], w [cout, cin, k] float64, "same" padding, no bias -> [cout, L].  skip = (tap, column): that tap's term is left out of
    that output column."""
    k = w.shape[2]
    pad = (k - 1) // 2
    L = x.shape[1]
    xp = np.pad(x, ((0, 0), (pad, pad)))
    out = np.zeros((w.shape[0], L))
    for tap in range(k):
        term = w[:, :, tap] @ xp[:, tap: tap + L]
        if skip is not None and skip[0] == tap:
            term[:, skip[1]] = 0.0
        out += term
    return out


def epilogue64(c, d, bi, acc, skip_bias_row=None):
    """bias (+ badd), gate or activation, out_scale, residual - on acc [cout, L] of sample bi"""
    L = acc.shape[1]
    b = d["b"].astype(np.float64).copy()
    if skip_bias_row is not None:
        b[skip_bias_row] = 0.0
    h = acc + b[:, None]
    if d["badd"] is not None:
        h = h + d["badd"][bi].astype(np.float64)[:, None]
    if c["gate"]:
        half = c["cout"] // 2
        return np.tanh(h[:half]) / (1.0 + np.exp(-h[half:]))
    y = act64(h, c["act"]) * c["scale"]
    if d["res"] is not None:
        y = y + d["res"][bi, :, :L].astype(np.float64)
    return y


def fp16_rounded(a, scale):
    """the one-product mode's operand: fp16(fp32(scale a)) / scale, nearest-even as split_pair rounds"""
    return np.float16(np.float32(scale) * np.asarray(a, np.float32)).astype(np.float64) / scale


def reference(c, d, bi, rounded=False):
    """float64 conv of sample bi on x[:, :len] (rounded: of the fp16-rounded operands, the exact value of the one-product mode)"""
    L = d["lens"][bi]
    x, w = d["x"][bi, :, :L], d["w"]
    if rounded:
        x, w = fp16_rounded(x, SCALE_X), fp16_rounded(w, SCALE_W)
    return epilogue64(c, d, bi, conv64(np.asarray(x, np.float64), np.asarray(w, np.float64)))


# ---- the scheme
def split(a, scale):
    """fp32 a -> (h0, h1) as float64 arrays holding fp16 values of a * scale"""
    v = np.clip(np.asarray(a, np.float32) * np.float32(scale), -65504.0, 65504.0).astype(np.float32)
    h0 = v.astype(np.float16)
    r = (v - h0.astype(np.float32)).astype(np.float32)
    h1 = r.astype(np.float16)
    return h0.astype(np.float64), h1.astype(np.float64)


ALL_TERMS = ((0, 0), (0, 1), (1, 0))     # (weight plane, input plane) of the three products


class Scheme:
    """The kernel's arithmetic for sample bi with the products accumulated in float64: every (weight plane, input plane, tap) term is
    computed once, a result is a sum of terms - so the seeded faults cost a column update each, not a conv."""

    def __init__(self, c, d, bi):
        self.c, self.d, self.bi = c, d, bi
        L = d["lens"][bi]
        k = c["k"]
        self.pad = (k - 1) // 2
        self.xs = [np.pad(h, ((0, 0), (self.pad, self.pad))) for h in split(d["x"][bi, :, :L], SCALE_X)]       # zero planes outside [0, len)
        self.ws = split(d["w"], SCALE_W)
        self.L = L
        self.term = {}

    def _term(self, pw, px, tap):
        key = (pw, px, tap)
        if key not in self.term:
            self.term[key] = self.ws[pw][:, :, tap] @ self.xs[px][:, tap: tap + self.L]
        return self.term[key]

    def result(self, terms=None, zero_low_col=None, skip=None, skip_bias_row=None):
        """terms: the (weight plane, input plane) products kept (default: the three of the scheme; p1: (0, 0) alone).  Seeded faults:
        zero_low_col = the input's low plane is zero in that column; skip = (tap, column): that tap's products are left out of that
        output column; skip_bias_row."""
        c = self.c
        if terms is None:
            terms = ((0, 0),) if c["p1"] else ALL_TERMS
        acc = np.zeros((c["cout"], self.L))
        for pw, px in terms:
            for tap in range(c["k"]):
                t = self._term(pw, px, tap)
                if skip is not None and skip[0] == tap:
                    t = t.copy()
                    t[:, skip[1]] = 0.0
                acc += t
                if zero_low_col is not None and px == 1:
                    n = zero_low_col - tap + self.pad              # the output column that reads input column zero_low_col at this tap
                    if 0 <= n < self.L and not (skip is not None and skip == (tap, n)):
                        acc[:, n] -= self.ws[pw][:, :, tap] @ self.xs[1][:, zero_low_col + self.pad]
        return epilogue64(c, self.d, self.bi, acc / (SCALE_X * SCALE_W), skip_bias_row=skip_bias_row)


def emulate(c, d, bi, **faults):
    return Scheme(c, d, bi).result(**faults)


# ---- the launcher's rule (launch_conv_x3), written out
def packed_rows(cout):
    return -(-cout // 128) * 128 if cout > 64 else (64 if cout > 32 else 32)


def eligible(c):
    """what op_conv1d_x3 accepts"""
    ok = c["k"] in (1, 3) and c["cin"] % 16 == 0 and packed_rows(c["cout"]) % BM == 0
    if c["p1"]:
        ok = ok and c["cin"] % 32 == 0 and not c["gate"]
    if c["gate"]:
        ok = ok and c["k"] == 1 and not c["res"] and c["act"] == 0 and c["scale"] == 1.0 and c["cout"] % 2 == 0 and c["T"] % 4 == 0
    else:
        ok = ok and not c["badd"]
    return ok


def expected_variant(c):
    nt = -(-c["T"] // BN)
    tiles_pad = packed_rows(c["cout"]) // BM * nt * 4
    s = 1
    if tiles_pad <= 128:
        s = min(4 if c["k"] == 3 else 2, 256 // tiles_pad, (c["cin"] // 16) // 8)
    if c["cap"] > 0:
        s = min(s, c["cap"])
    s = max(s, 1)
    live = sum(min(nt, -(-n // BN)) for n in lens_of(c))
    epi = 4 if c["gate"] else (1 if (c["act"] != 0 or c["scale"] != 1.0) else 0)
    return dict(epi=epi, kw3=int(c["k"] == 3), ksplit=s, epi_vec=int(c["T"] % 4 == 0), cols=int(0 < live < 4 * nt), p1=c["p1"])
