"""GPU parity of every tile shape of the exact-fp32 MFMA conv (csrc/conv_gemm_kernel.h) the launcher can pick, one conv at a time.

By default a launch of at most 384 128 x 128 tiles takes the 64 x 64 tile, so at unit-test sizes the 128-row tiles and the 64 x 128
tile never run.  Option "conv_small_tiles" = 0 switches that rule off: the launcher then picks by shape alone (csrc/conv_gemm.hip),

    CoutP % 128 == 0, wide   -> 128,128,k16        CoutP == 64, Nout > 64  -> 64,128,k16
    CoutP % 128 == 0, narrow -> 128,64,k16         CoutP == 64, Nout <= 64 -> 64,64,k16          CoutP == 32 -> 32,128,k16

(wide: the 128-column input tile fits and (round_up(Nout, 128) - round_up(Nout, 64)) * 10 <= Nout).  Every case names the tile it was
written for and asserts, through the launch profiler, that exactly that kernel ran once.

Every case is a batch of four samples whose output lengths are Nout, a multiple of the tile's BN, that multiple + 1, and 1: an error
at a tile edge, in the halo, or in a row guard shows on different samples.  Per case:
  (a) per sample max |y - ref| < 2e-5 over the live columns, ref in float64 (the gate of test_conv1d_kernel on the same data:
      w ~ N(0, 1 / (cin k)), x ~ N(0, 1), b ~ N(0, 1); cin k <= 2304.  A dropped tap or halo column costs ~ 1 / sqrt(cin k) >= 0.02);
  (b) the columns at and beyond a sample's length are exactly 0: op_conv1d hands the kernel a zeroed buffer and the bias is non-zero;
  (c) where the small-launch tile of the same problem is 64,64,k16 (CinP % 32 != 0 or k dil > 3) the output equals the default's bit
      for bit: all k16 tiles run the same K loop, "same k order per output: identical sums" (csrc/conv_gemm.hip).
The measured figures are in profiles/conv_tiles_measured_errors.txt (DTTS_TEST_LOG=<file> appends them run by run)."""
import os
import zlib

import numpy as np
import pytest

from conv_tile_probe import launches_of

torch = pytest.importorskip("torch")

GATE = 2e-5
SLOPE = float(np.float32(0.1))          # op_conv1d's leaky-relu slope (0.1f)
ACT_SILU, ACT_LRELU, ACT_TANH = 1, 2, 5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def record(name, value, limit):
    print(f"{name}\t{value:.3e}\t{limit:.1e}")
    log = os.environ.get("DTTS_TEST_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{name}\t{value:.3e}\t{limit:.1e}\n")


def tag(tile):
    return f"conv_gemm_kernel<{tile}>"


# ---- float64 references
def act64(v, act):
    if act == ACT_LRELU:
        return np.where(v >= 0, v, v * SLOPE)
    if act == ACT_SILU:
        return v / (1.0 + np.exp(-v))
    if act == ACT_TANH:
        return np.tanh(v)
    assert act == 0
    return v


def conv64(x, w, b, stride, pad, dil):
    """x [cin, L], w [cout, cin, k], all float64 -> [cout, n] (torch conv1d semantics)"""
    k = w.shape[2]
    xp = np.pad(x, ((0, 0), (pad, pad)))
    n = (x.shape[1] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    out = np.repeat(b[:, None], n, axis=1)
    for tap in range(k):
        out += w[:, :, tap] @ xp[:, tap * dil: tap * dil + (n - 1) * stride + 1: stride]
    return out


def conv_transpose64(x, w, b, s, p):
    """x [cin, L], w [cin, cout, k] (k - s == 2p), float64 -> [cout, L s] (torch ConvTranspose1d)"""
    L, k = x.shape[1], w.shape[2]
    full = np.zeros((w.shape[1], (L - 1) * s + k))
    for j in range(k):
        full[:, j: j + (L - 1) * s + 1: s] += w[:, :, j].T @ x
    return full[:, p: p + L * s] + b[:, None]


# ---- cases.  tile: what conv_small_tiles = 0 must launch; small: what the default rule launches for the same problem
def case(tile, name, cin, cout, k, nout, pad=0, dil=1, stride=1, small=None, **opts):
    return pytest.param(dict(tile=tile, name=name, cin=cin, cout=cout, k=k, nout=nout, pad=pad, dil=dil, stride=stride, small=small, **opts),
                        id=f"{tile}-{name}")


K3 = dict(cin=128, cout=768, k=3, pad=1)                       # compile-time taps (KWT = 3) on the 128-row tiles; the small tile is k32
K1 = dict(cin=768, cout=200, k=1)                              # KWT = 1; CoutP = 256: rows 200 .. 255 are padding
K7 = dict(cin=100, cout=100, k=7, dil=3, pad=9, small="64,64,k16")        # CinP = 112: channels 100 .. 111 of the last K block are zero fill
K11 = dict(cin=200, cout=200, k=11, dil=5, pad=25, small="64,64,k16")     # halo 50: XW = 178 at BN = 128, beyond two 64-lane columns
S2 = dict(cin=128, cout=768, k=3, pad=1, stride=2)             # XW = 129 at BN = 64; never "wide"
GATED = dict(cin=192, cout=384, k=5, pad=2, small="64,64,k16")
UP4 = dict(cin=200, cout=100, k=8, up=(4, 2), small="64,64,k16")          # ConvTranspose1d(200, 100, 8, 4, 2) as 4 phases: rows 400, CoutP 512
N50_K3 = dict(cin=50, cout=50, k=3, pad=1)                     # CoutP = 64; the small tile is k32
N50_K7 = dict(cin=50, cout=50, k=7, dil=3, pad=9, small="64,64,k16")
N50_K11 = dict(cin=50, cout=50, k=11, dil=5, pad=25, small="64,64,k16")
N25 = dict(cin=25, cout=25, k=11, pad=5)                       # CoutP = 32: the small-launch rule never applies
N12 = dict(cin=12, cout=1, k=7, pad=3)

CASES = [
    # 128,128,k16: wide Nout
    case("128,128,k16", "k3", nout=250, **K3),
    case("128,128,k16", "k1_cout200", nout=333, **K1),
    case("128,128,k16", "k7_dil3_cin100", nout=380, **K7),
    case("128,128,k16", "k11_dil5", nout=250, **K11),
    case("128,128,k16", "epi_lrelu", nout=250, epi_act=ACT_LRELU, **K7),
    case("128,128,k16", "epi_tanh", nout=333, epi_act=ACT_TANH, **K3),
    case("128,128,k16", "gate1", nout=250, gate=1, **GATED),
    case("128,128,k16", "gate2", nout=380, gate=2, **GATED),
    case("128,128,k16", "res_k3", nout=380, res=True, **K3),
    case("128,128,k16", "res_k11_dil5", nout=333, res=True, **K11),
    case("128,128,k16", "pro_lrelu", nout=333, pro_act=ACT_LRELU, **K7),
    case("128,128,k16", "pro_silu", nout=250, pro_act=ACT_SILU, **K3),
    case("128,128,k16", "phases4_ragged", nout=250, **UP4),
    # 128,64,k16: narrow Nout, or stride 2
    case("128,64,k16", "k3", nout=257, **K3),
    case("128,64,k16", "k1_cout200", nout=300, **K1),
    case("128,64,k16", "k7_dil3_cin100", nout=129, **K7),
    case("128,64,k16", "k11_dil5", nout=257, **K11),
    case("128,64,k16", "stride2", nout=150, **S2),
    case("128,64,k16", "epi_lrelu", nout=300, epi_act=ACT_LRELU, **K7),
    case("128,64,k16", "epi_tanh", nout=129, epi_act=ACT_TANH, **S2),
    case("128,64,k16", "gate1", nout=129, gate=1, **GATED),
    case("128,64,k16", "gate2", nout=257, gate=2, **GATED),
    case("128,64,k16", "res_k3", nout=129, res=True, **K3),
    case("128,64,k16", "res_k7_dil3", nout=257, res=True, **K7),
    case("128,64,k16", "pro_lrelu", nout=257, pro_act=ACT_LRELU, **K11),
    case("128,64,k16", "pro_silu", nout=300, pro_act=ACT_SILU, **K1),
    case("128,64,k16", "phases4_ragged", nout=130, **UP4),
    # 64,128,k16: CoutP = 64, Nout > 64
    case("64,128,k16", "k3", nout=200, **N50_K3),
    case("64,128,k16", "k11_dil5", nout=300, **N50_K11),
    case("64,128,k16", "epi_lrelu", nout=130, epi_act=ACT_LRELU, **N50_K7),
    case("64,128,k16", "epi_tanh", nout=257, epi_act=ACT_TANH, **N50_K11),
    case("64,128,k16", "res", nout=257, res=True, **N50_K7),
    case("64,128,k16", "pro_lrelu", nout=130, pro_act=ACT_LRELU, **N50_K11),
    case("64,128,k16", "pro_silu", nout=300, pro_act=ACT_SILU, **N50_K7),
    case("64,128,k16", "phases2_ragged", nout=130, cin=40, cout=25, k=4, up=(2, 1), small="64,64,k16"),
    # 32,128,k16: CoutP = 32
    case("32,128,k16", "k11", nout=130, **N25),
    case("32,128,k16", "cout1_k7", nout=300, **N12),
    case("32,128,k16", "epi_lrelu", nout=257, epi_act=ACT_LRELU, **N25),
    case("32,128,k16", "epi_tanh", nout=130, epi_act=ACT_TANH, **N12),
    case("32,128,k16", "res", nout=300, res=True, **N25),
    case("32,128,k16", "pro_lrelu", nout=257, pro_act=ACT_LRELU, **N12),
    case("32,128,k16", "pro_silu", nout=130, pro_act=ACT_SILU, **N25),
    case("32,128,k16", "phases2_ragged", nout=257, cin=25, cout=12, k=2, up=(2, 0)),
    # the launcher's last product tile with the rule off: CoutP = 64, Nout <= 64
    case("64,64,k16", "k11_dil5_nout64", nout=64, **N50_K11),
]


RESTORE = {"conv_small_tiles": -1, "conv_x3": 1}


@pytest.fixture
def option():
    """option(rt, key, value) sets "conv_small_tiles" (process-wide) or "conv_x3" and always puts the default back: a leaked
    conv_small_tiles would silently change which tile every later test exercises."""
    touched = []

    def set_(rt, key, value):
        touched.append((rt, key))
        rt.set_option(key, value)
    try:
        yield set_
    finally:
        for rt, key in touched:
            rt.set_option(key, RESTORE[key])


def out_lens(c):
    bn = int(c["tile"].split(",")[1])
    m = (c["nout"] - 2) // bn * bn          # the largest multiple of BN with m + 1 < Nout: four different lengths
    return [c["nout"], m, m + 1, 1] if m > 0 else [c["nout"], c["nout"] - 1, 2, 1]      # (one N tile: Nout itself is the multiple)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES)
def test_conv_tile(c, option):
    from detail_tts_amd.packing import convtranspose_as_phases, gate_perm, pack_conv
    from detail_tts_amd.runtime import Runtime
    rs = np.random.RandomState(zlib.crc32(f"{c['tile']}-{c['name']}".encode()) & 0x7fffffff)
    cin, cout, k, stride, dil, pad = c["cin"], c["cout"], c["k"], c["stride"], c["dil"], c["pad"]
    gate, up = c.get("gate", 0), c.get("up")
    assert cin * k <= 2304
    b = rs.randn(cout).astype(np.float32)
    if up:                                              # ConvTranspose1d(cin, cout, k, s, p) as s phases of an equivalent correlation
        s, p = up
        w = (rs.randn(cin, cout, k) / np.sqrt(cin * k / s)).astype(np.float32)      # k / s taps meet in an output
        weq, pad = convtranspose_as_phases(w, s, p)
        wp, bp = pack_conv(weq, np.tile(b, s))
        kw, phases = weq.shape[2], s
    else:
        w = (rs.randn(cout, cin, k) / np.sqrt(cin * k)).astype(np.float32)
        wp, bp = pack_conv(w, b, row_perm=gate_perm(cout) if gate else None)
        kw, phases = k, 1
    lo = out_lens(c)
    li = [(n - 1) * stride + dil * (kw - 1) + 1 - 2 * pad for n in lo]
    assert min(li) >= 1 and li[0] == max(li)
    x = rs.randn(4, cin, li[0]).astype(np.float32)      # columns at and beyond a sample's length hold data the kernel must not read as input
    rows_out = cout // 2 if gate else cout
    res = rs.randn(4, rows_out, lo[0] * phases).astype(np.float32) if c.get("res") else None
    r = Runtime({}, parts=(), extra={"t.wp": wp, "t.bp": bp})

    def run():
        return host(r.op_conv1d("t", dev(x), cout, kw, stride=stride, dil=dil, pad=pad, pro_act=c.get("pro_act", 0), epi_act=c.get("epi_act", 0),
                                gate=gate, phases=phases, res=None if res is None else dev(res), lens_in=li))

    option(r, "conv_small_tiles", 0)
    y, ran = launches_of(r, run)
    assert ran == {tag(c["tile"]): 1}, ran
    assert y.shape == (4, rows_out, lo[0] * phases)
    worst = 0.0
    for bi in range(4):
        L = lo[bi] * phases
        xin = act64(x[bi, :, :li[bi]].astype(np.float64), c.get("pro_act", 0))
        if up:
            ref = conv_transpose64(xin, w.astype(np.float64), b.astype(np.float64), *up)
        else:
            ref = conv64(xin, w.astype(np.float64), b.astype(np.float64), stride, pad, dil)
        if gate:
            h = cout // 2
            ref = (np.tanh(ref[:h]) if gate == 1 else ref[:h]) / (1.0 + np.exp(-ref[h:]))
        ref = act64(ref, c.get("epi_act", 0))
        if res is not None:
            ref = ref + res[bi, :, :L].astype(np.float64)
        assert ref.shape == (rows_out, L)
        err = float(np.max(np.abs(y[bi, :, :L].astype(np.float64) - ref)))
        worst = max(worst, err)
        record(f"conv_tile<{c['tile']}>_{c['name']}_len{lo[bi]}", err, GATE)
        assert err < GATE, (c["name"], bi, lo[bi], err)                                            # (a)
        assert not y[bi, :, L:].any(), (c["name"], bi, lo[bi], np.argwhere(y[bi, :, L:])[:4])      # (b)
    record(f"conv_tile<{c['tile']}>_{c['name']}", worst, GATE)
    if c["small"]:                                                                                 # (c)
        option(r, "conv_small_tiles", -1)
        y0, ran0 = launches_of(r, run)
        assert ran0 == {tag(c["small"]): 1}, ran0
        if c["small"] != c["tile"]:
            assert np.array_equal(y, y0), (c["name"], float(np.abs(y - y0).max()), np.argwhere(y != y0)[:4])


def test_case_table_reaches_every_product_tile_and_every_k16_small_tile_claim():
    """The table above, checked against the launcher's rule written out here: a case whose geometry no longer lands on the tile it
    names is a mistake in the table (the kernel-side assertion in test_conv_tile is the launch profiler's)."""
    from detail_tts_amd.packing import ceil_to, packed_cout
    tiles = set()
    for prm in CASES:
        c = prm.values[0]
        kw = c["k"]
        if c.get("up"):                                 # taps of the equivalent correlation (packing.convtranspose_as_phases)
            s, p = c["up"]
            kw = (s - 1 + p) // s + (c["k"] - 1 - p) // s + 1
        coutp = packed_cout(c["cout"] * (c["up"][0] if c.get("up") else 1))
        halo, nout = (kw - 1) * c["dil"], c["nout"]
        fits = lambda bn: (bn - 1) * c["stride"] + halo + 1 <= 192
        if coutp % 128 == 0:
            wide = fits(128) and (ceil_to(nout, 128) - ceil_to(nout, 64)) * 10 <= nout
            tile = "128,128,k16" if wide else "128,64,k16"
        elif coutp == 64:
            tile = "64,128,k16" if fits(128) and nout > 64 else "64,64,k16"
        else:
            tile = "32,128,k16"
        assert tile == c["tile"], c
        small_k16 = coutp % 64 == 0 and (ceil_to(c["cin"], 16) % 32 != 0 or kw * c["dil"] > 3)
        assert (c["small"] == "64,64,k16") == small_k16, c
        tiles.add(tile)
        tiles.add(c["small"])
    assert tiles >= {"128,128,k16", "128,64,k16", "64,128,k16", "64,64,k16", "32,128,k16"}


# ---- the diffusion trunk's ResBlock on the 128-row tiles: GroupNorm affine + SiLU prologue (PRO 1) on the compile-time-tap paths
# (KWT = 1 for in_layers.2, KWT = 3 + the residual epilogue for out_layers.3), reachable from no single-conv entry
@pytest.fixture(scope="module")
def rt(weights):
    from detail_tts_amd.runtime import Runtime
    return Runtime(weights, folded=True, parts=("diffusion",))


@pytest.mark.gpu
@pytest.mark.parametrize("T,lens,tile", [(129, [129, 1], "128,64,k16"), (257, [256, 130], "128,64,k16"), (250, [250, 128], "128,128,k16")])
def test_exact_fp32_resblock_on_the_128_row_tiles(rt, weights, option, T, lens, tile):
    from oracle import diffusion as D
    rs = np.random.RandomState(1000 + T)
    sched = D.make_schedule()
    x = rs.randn(len(lens), 768, T).astype(np.float32)
    step = int(rs.randint(0, 50))
    prefix = "diffusion.layers.5.resblk"
    option(rt, "conv_x3", 0)
    option(rt, "conv_small_tiles", 0)
    y, ran = launches_of(rt, lambda: host(rt.op_resblock(prefix, dev(x), step, lens)))
    assert {n: v for n, v in ran.items() if n.startswith("conv_")} == {tag(tile): 2}, ran       # in_layers.2 and out_layers.3
    temb = D.time_embed(weights, [sched["timestep_map"][step]], 768)
    for b, L in enumerate(lens):
        ref = D.res_block(weights, prefix, x[b:b + 1, :, :L], temb)[0]
        err = float(np.max(np.abs(y[b, :, :L].astype(np.float64) - ref.astype(np.float64))))
        record(f"resblock_fp32<{tile}>_T{T}_len{L}", err, 1e-4)
        assert err < 1e-4, (T, b, err)
        assert not y[b, :, L:].any(), (T, b)
