"""GPU parity of the diffusion trunk's split-precision attention path, one piece at a time through Runtime.op_attention_x3: the qkv conv's
operand-image epilogue (csrc/conv_x3.hip, EPI 2), flash_attn_x3b_kernel (csrc/attention_x3b.hip) with its FAR / NEAR / masked loops,
bias table, key split and one-product mode, and its plane-writing epilogue.  The block tests (test_gpu_diffusion.py, test_gpu_fp16.py)
reach these only under the synthetic weights (score std ~0.3: near-uniform softmax) and behind proj_out, at 1e-4 absolute - under which
a build that never multiplies P's low plane in the PV product, and one that drops K1 Q0 from QK^T, pass all of them while failing five
cases here (mutated builds, run once by hand: profiles/attn_x3_measured_errors.txt).

The table, its planted data, the float64 reference, the layout decoders and the emulated scheme are in tests/attn_x3_model.py;
tests/test_host_attn_x3.py shows on the CPU that the gate used here (2e-5, max |y - ref| / max(1, max |ref|)) sits a factor 10 above
the scheme and a factor 3 below every mutation a case claims, and that the table covers every loop combination of the kernel's plan.
Every case is a ragged batch (random x beyond each length) with lengths on and beside the 32 / 64 / 128 / 192 seams.

(a) test_operand_image: the decoded Q (scale folded in), K and V of the image match the float64 conv at the conv suite's gate; keys in
    [len, next multiple of 64) are exactly zero; whole tiles beyond the length and Q columns >= len still hold the 0xFF fill the entry
    wrote before the conv (the contract between writer and reader); bit-identical under 2 / 3 / 4 conv stages; the conv reports epi 2
    and one conv launch + one attention launch ran; p1: the image matches the conv of the fp16-rounded operands.
(b), (c) test_attention: bias pointers (scores 0, one table entry of 20 nats per head: query t returns v[t + o], at o = +-64 the mean
    of all far keys), score pointers (>= 10 nats margin to a chosen key: key 0, len - 1, seam neighbours, distance 63 / 64 / 65, the ends
    of every key range), random data at score std 0.6 / 2 / 5 (one with packing.bias_table's table) and the growing-scores ramp; every
    sample under the gate, output columns >= len exactly zero, guard slab untouched.
(d) key split S = 1 .. 4 forced through options "attn_ksplit" / "attn_ksplit_cus" (restored in finally; the info struct confirms S;
    three repeated calls bit-identical; vs unsplit within 2e-5), the one-product mode (differs, larger error, under P1_GATE), and the
    fp32 output form against the planes form to the split's 22 bits.
The measured figures are in profiles/attn_x3_measured_errors.txt (DTTS_TEST_LOG=<file> appends them run by run)."""
import functools
import os

import numpy as np
import pytest

import attn_x3_model as M
import conv_x3_model as CM
from conv_tile_probe import launches_of

torch = pytest.importorskip("torch")

GATE = M.GATE
IDS = [c["name"] for c in M.CASES]
BY_NAME = {c["name"]: c for c in M.CASES}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def record(name, value, limit):
    print(f"{name}\t{value:.3e}\t{limit:.1e}")
    log = os.environ.get("DTTS_TEST_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{name}\t{value:.3e}\t{limit:.1e}\n")


@functools.lru_cache(maxsize=None)
def data_of(name):
    """(data, float64 references per sample): computed once, shared by the tests, never modified"""
    d = M.make_data(BY_NAME[name])
    return d, [M.reference(d, bi) for bi in range(len(d["lens"]))]


RESTORE = {"conv_stages": -1, "attn_ksplit": 4, "attn_ksplit_cus": 256}


@pytest.fixture
def option():
    """option(rt, key, value) sets a process-wide launcher option and always puts the default back"""
    touched = []

    def set_(rt, key, value):
        touched.append((rt, key))
        rt.set_option(key, value)
    try:
        yield set_
    finally:
        for rt, key in touched:
            rt.set_option(key, RESTORE[key])


class Attn:
    """one case on the device: the packed qkv weights bound to a Runtime of its own, inputs uploaded once"""

    def __init__(self, c, d):
        from detail_tts_amd.packing import pack_conv
        from detail_tts_amd.runtime import Runtime
        self.c, self.lens = c, d["lens"]
        wp, bp = pack_conv(d["w"][:, :, None], d["b"])
        self.rt = Runtime({}, parts=(), extra={"t.wp": wp, "t.bp": bp})
        self.x, self.tab = dev(d["x"]), dev(d["tab"])

    def run(self, p1=0, out_f32=False):
        """-> (y numpy: raw plane bytes [B, n] or fp32 [B, 48 H, T], image bytes, info, guard numpy, launches)"""
        call = lambda: self.rt.op_attention_x3("t", self.x, self.c["H"], self.tab, lens=self.lens, p1=p1, out_f32=out_f32)
        (y, image, info, guard), ran = launches_of(self.rt, call)
        return y.cpu().numpy(), image.cpu().numpy().tobytes(), info, guard.cpu().numpy(), ran


def tags(p1):
    return {"conv_x3_kernel<128,192,fp16>" if p1 else "conv_x3_kernel<128,192>": 1, "flash_attn_x3b_kernel<fp16>" if p1 else "flash_attn_x3b_kernel": 1}


def check_image(c, d, raw, p1):
    """(a) on one image; returns the worst decoded error"""
    H, T, lens = c["H"], c["T"], d["lens"]
    B = len(lens)
    qb, kb, vb = M.decode_image(raw, B, H, T)
    worst = 0.0
    for bi, L in enumerate(lens):
        x, w = d["x"][bi, :, :L], d["w"]
        if p1:
            x, w = CM.fp16_rounded(x, CM.SCALE_X), CM.fp16_rounded(w, CM.SCALE_W)
        q, k, v = M.qkv64(w, d["b"], x)
        for nm, bits, ref, scale in (("q", qb, q * M.QSCALE, 16.0), ("k", kb, k, 16.0), ("v", vb, v, 16.0)):
            got = (M.f16(bits[bi, :, 0, :, :L]) + M.f16(bits[bi, :, 1, :, :L])) / scale
            e = float(np.max(np.abs(got - ref)))
            worst = max(worst, e)
            assert e < CM.GATE, (c["name"], nm, bi, L, e)
            if p1:
                # plane 0 - all the one-product attention reads - is the fp16 rounding of that value: half an fp16 ulp (2^-11 relative,
                # 2^-25 absolute below the normal range) on top of the gate
                e0 = np.abs(M.f16(bits[bi, :, 0, :, :L]) / scale - ref)
                assert np.all(e0 <= CM.GATE + np.abs(ref) * 2.0 ** -11 + 2.0 ** -25 / scale), (c["name"], nm, bi, float(e0.max()))
        Lt = M.tq(L)
        for nm, bits in (("k", kb), ("v", vb)):
            assert not M.f16(bits[bi, :, :, :, L:Lt]).any(), (c["name"], nm, bi, L, "keys in [len, tile end) must be zero")
            assert np.all(bits[bi, :, :, :, Lt:] == 0xFFFF), (c["name"], nm, bi, L, "tiles beyond the length must keep the fill")
        assert np.all(qb[bi, :, :, :, L:] == 0xFFFF), (c["name"], bi, L, "Q columns >= len must keep the fill")
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("c", M.CASES, ids=IDS)
def test_operand_image(c, option):
    d, _ = data_of(c["name"])
    at = Attn(c, d)
    option(at.rt, "attn_ksplit", 1)
    images = {}
    for stg in (2, 3, 4):
        option(at.rt, "conv_stages", stg)
        _, raw, info, _, ran = at.run()
        assert ran == tags(0), ran
        assert info["epi"] == 2 and info["stages"] == stg and info["p1"] == 0 and info["kw3"] == 0, info
        assert len(raw) == M.image_bytes(len(d["lens"]), c["H"], c["T"])
        images[stg] = raw
    assert images[2] == images[3] == images[4], c["name"]
    record(f"attn_x3_image_{c['name']}", check_image(c, d, images[4], 0), CM.GATE)
    if c["p1"]:
        option(at.rt, "conv_stages", -1)
        _, raw, info, _, ran = at.run(p1=1)
        assert ran == tags(1) and info["epi"] == 2 and info["p1"] == 1 and info["attn_p1"] == 1, (ran, info)
        assert raw != images[4]
        record(f"attn_x3_image_{c['name']}_p1_vs_rounded_operands", check_image(c, d, raw, 1), CM.GATE)


def decode(c, d, y, out_f32):
    """-> [B, 48 H, T] float64 after asserting what must not have been written"""
    H, T, lens = c["H"], c["T"], d["lens"]
    B = len(lens)
    if out_f32:
        for bi, L in enumerate(lens):
            assert np.isnan(y[bi, :, L:]).all() and np.isfinite(y[bi, :, :L]).all(), (c["name"], bi, L)
        return y.astype(np.float64)
    val, bits = M.decode_out_planes(y.tobytes(), B, H, T)
    for bi, L in enumerate(lens):
        assert not bits[bi, :, :, 0].any() and not bits[bi, :, :, L + 1:].any(), (c["name"], bi, L, "columns outside [0, len) must stay zero")
    return val


def worst(c, d, val, refs, tag, limit):
    """the metric per sample, recorded; returns the worst"""
    out = 0.0
    for bi, L in enumerate(d["lens"]):
        e = M.rel_err(val[bi, :, :L], refs[bi])
        record(f"attn_x3_{c['name']}_{tag}_len{L}", e, limit)
        out = max(out, e)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c", M.CASES, ids=IDS)
def test_attention(c, option):
    d, refs = data_of(c["name"])
    lens = d["lens"]
    B = len(lens)
    at = Attn(c, d)
    option(at.rt, "attn_ksplit_cus", 1 << 20)            # (by default a launch is split only while its workgroups x S find a CU each)
    base = -(-c["T"] // 128) * c["H"] * B
    outs = {}
    for S in c["ksplit"]:
        option(at.rt, "attn_ksplit", S)
        y, _, info, guard, ran = at.run()
        assert ran == tags(0), ran
        assert info["epi"] == 2 and info["attn_ksplit"] == S and info["attn_p1"] == 0 and info["attn_workgroups"] == base * S, info
        assert np.all(guard == 0xFF), (c["name"], S, "guard slab written")
        val = decode(c, d, y, False)
        e = worst(c, d, val, refs, f"S{S}", GATE)
        assert e < GATE, (c["name"], S, e)                                                      # (b), (c)
        outs[S] = val
        if S > 1:
            for rep in range(3):                          # counters back at zero, merge in split order
                y2, _, info2, guard2, _ = at.run()
                assert info2["attn_ksplit"] == S and np.array_equal(y2, y) and np.all(guard2 == 0xFF), (c["name"], S, rep)
            ev = max(M.rel_err(val[bi, :, :L], outs[1][bi, :, :L]) for bi, L in enumerate(lens))
            record(f"attn_x3_{c['name']}_S{S}_vs_unsplit", ev, 2e-5)
            assert ev < 2e-5, (c["name"], S, ev)
    option(at.rt, "attn_ksplit", 1)
    if c["fp32_form"]:
        y, _, info, guard, ran = at.run(out_f32=True)
        assert ran == tags(0) and np.isnan(guard).all(), ran
        v32 = decode(c, d, y, True)
        e = worst(c, d, v32, refs, "fp32_form", GATE)
        assert e < GATE, (c["name"], e)
        # the planes are the two-plane split of 16 x the same fp32 value (split3.h: 22 significant bits, an absolute 2^-25 / scale where
        # the low plane is subnormal)
        for bi, L in enumerate(lens):
            a, b = outs[1][bi, :, :L], v32[bi, :, :L]
            assert np.all(np.abs(a - b) <= np.abs(b) * 2.0 ** -22 + 2.0 ** -25 / CM.SCALE_X), (c["name"], bi, float(np.abs(a - b).max()))
    if c["p1"]:
        y, _, info, guard, ran = at.run(p1=1)
        assert ran == tags(1) and info["p1"] == 1 and info["attn_p1"] == 1 and info["attn_ksplit"] == 1, (ran, info)
        assert np.all(guard == 0xFF)
        v1 = decode(c, d, y, False)
        e1, e3 = worst(c, d, v1, refs, "p1", M.P1_GATE), max(M.rel_err(outs[1][bi, :, :L], refs[bi]) for bi, L in enumerate(lens))
        assert not np.array_equal(v1, outs[1]) and e3 < e1 < M.P1_GATE, (c["name"], e1, e3)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,says", M.REJECTS, ids=[r[0] for r in M.REJECTS])
def test_bad_calls_are_refused_on_the_host_before_any_launch(name, kw, says):
    from detail_tts_amd.packing import pack_conv
    from detail_tts_amd.runtime import DttsError, Runtime
    a = dict(cin=32, H=2, T=100, lens=[100, 50], p1=0, H_arg=None)
    a.update(kw)
    rs = np.random.RandomState(0)
    rows = 144 * max(a["H"], 1)                          # (weights packed for the call's own shape: the refusal is the entry's, not a missing tensor's)
    wp, bp = pack_conv(rs.randn(rows, a["cin"], 1).astype(np.float32), rs.randn(rows).astype(np.float32))
    rt = Runtime({}, parts=(), extra={"t.wp": wp, "t.bp": bp})
    heads = a["H"] if a["H_arg"] is None else a["H_arg"]
    x, tab = dev(rs.randn(2, a["cin"], a["T"])), dev(np.zeros((max(heads, 1), 129)))
    if heads < 1:
        tab = tab[:0]

    def attempt():
        with pytest.raises(DttsError) as e:
            rt.op_attention_x3("t", x, heads, tab, lens=a["lens"], p1=a["p1"])
        return str(e.value)
    msg, ran = launches_of(rt, attempt, level=2)          # (level 2: the split passes would show too)
    assert says in msg and ("invalid argument" in msg or says != "op_attention_x3"), msg
    assert ran == {}, ran
