"""GPU parity of every instantiation of the split-precision conv (csrc/conv_x3.hip) the launcher can pick outside EPI 2, one conv at a
time through Runtime.op_conv1d_x3: EPI 0 (bias, + residual), 1 (activation, out_scale, residual) and 4 (gated), k = 1 and k = 3, the
one-product mode p1, split-K 1 .. 4 (uneven splits included), the live-column table of ragged batches and both epilogue forms (LDS-staged
16-byte stores / scalar stores).  The launcher picks the LDS stage count by launch size, so unit-test shapes would only ever see four
stages: option "conv_stages" forces 2, 3 and 4 on every case.  EPI 2 (the qkv conv's operand images) has its own unit tests, with the
attention that reads them, in tests/test_gpu_attn_x3.py (Runtime.op_attention_x3).

The table, its data and the float64 references are in tests/conv_x3_model.py; tests/test_host_conv_x3.py shows on the CPU that the gate
used here separates the scheme (3 - 6e-7) from a dropped cross product, a zeroed low plane of one seam column, a dropped tap and an
omitted bias, and that every case lands on the variant it names under the launcher's rule.  Here every case asserts that the launcher
REPORTS that variant (dtts_conv_x3_info) and that exactly one conv_x3 launch ran.

Every case is a batch of four samples of lengths T, the largest multiple m of the 192-column tile with m + 1 < T, m + 1, and 1 (T, T - 1,
2, 1 where m = 0); x holds random data beyond each length.  Per sample, under each stage count:
  (a) max |y - ref| < 2e-5 over the live columns, ref the float64 conv of x[:, :len] (w ~ N(0, 1 / (cin k)), x, b ~ N(0, 1));
  (b) the columns at and beyond the length are exactly 0 (the buffer is handed over zeroed, the bias is not zero);
  (c) the NaN guard slab behind the batch is untouched;
  (d) p1: ref is the float64 conv of the fp16-rounded operands (fp16 x fp16 products are exact in fp32: same gate); the output differs
      from the three-product output of the same case and its error against the unrounded reference is the larger one.
The outputs under 2, 3 and 4 stages are bit-identical (the K order - channel block, tap - does not depend on the prefetch distance), so
are three repeated calls of a split-K launch (counters back at zero, merge in split order) and a ragged batch with and without its
column table (the split is decided on the padded tile count).
The measured figures are in profiles/conv_x3_measured_errors.txt (DTTS_TEST_LOG=<file> appends them run by run)."""
import os

import numpy as np
import pytest

import conv_x3_model as M
from conv_tile_probe import launches_of

torch = pytest.importorskip("torch")

GATE = M.GATE
STAGES = (2, 3, 4)


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


RESTORE = {"conv_stages": -1, "conv_cols": 1}


@pytest.fixture
def option():
    """option(rt, key, value) sets "conv_stages" (process-wide) or "conv_cols" and always puts the default back: a leaked conv_stages
    would silently change which instantiation every later test exercises."""
    touched = []

    def set_(rt, key, value):
        touched.append((rt, key))
        rt.set_option(key, value)
    try:
        yield set_
    finally:
        for rt, key in touched:
            rt.set_option(key, RESTORE[key])


class Conv:
    """one case on the device: packed weights bound to a Runtime of its own, inputs uploaded once"""

    def __init__(self, c, d):
        from detail_tts_amd.packing import gate_perm, pack_conv
        from detail_tts_amd.runtime import Runtime
        self.c = c
        perm = gate_perm(c["cout"]) if c["gate"] else None
        wp, bp = pack_conv(d["w"], d["b"], row_perm=perm)
        self.rt = Runtime({}, parts=(), extra={"t.wp": wp, "t.bp": bp})
        self.x = dev(d["x"])
        self.res = None if d["res"] is None else dev(d["res"])
        self.badd = None if d["badd"] is None else dev(d["badd"][:, perm])      # packed row order
        self.lens = d["lens"]

    def run(self, p1=None, cap=None):
        """-> (y [4, rows, T] numpy, info, guard slab numpy, launches)"""
        c = self.c
        call = lambda: self.rt.op_conv1d_x3("t", self.x, c["cout"], c["k"], epi_act=c["act"], out_scale=c["scale"], gate=c["gate"], badd=self.badd,
                                            res=self.res, lens=self.lens, p1=c["p1"] if p1 is None else p1, ksplit_max=c["cap"] if cap is None else cap)
        (y, info, guard), ran = launches_of(self.rt, call)
        return host(y), info, host(guard), ran


def tag(p1):
    return "conv_x3_kernel<128,192,fp16>" if p1 else "conv_x3_kernel<128,192>"


def workgroups(c, lens, cols):
    nt = -(-c["T"] // M.BN)
    columns = sum(min(nt, -(-n // M.BN)) for n in lens) if cols else 4 * nt
    return M.packed_rows(c["cout"]) // M.BM * columns * c["ksplit"]


def rule_stages(wgs):
    """the launcher's rule (option "conv_stages" = 0): four LDS stages up to 128 workgroups, three up to 600, two beyond"""
    return 4 if wgs <= 128 else (3 if wgs <= 600 else 2)


def worst_err(y, refs, lens):
    return max(float(np.max(np.abs(y[bi, :, :L].astype(np.float64) - refs[bi]))) for bi, L in enumerate(lens))


@pytest.mark.gpu
@pytest.mark.parametrize("c", M.CASES, ids=[c["name"] for c in M.CASES])
def test_conv_x3(c, option):
    d = M.make_data(c)
    lens = d["lens"]
    refs = [M.reference(c, d, bi, rounded=bool(c["p1"])) for bi in range(4)]      # computed once, shared by the stage counts
    rows = c["cout"] // 2 if c["gate"] else c["cout"]
    cv = Conv(c, d)
    want = {k: c[k] for k in ("epi", "kw3", "ksplit", "p1", "epi_vec", "cols")}
    outs = {}
    for stg in STAGES:
        option(cv.rt, "conv_stages", stg)
        y, info, guard, ran = cv.run()
        assert ran == {tag(c["p1"]): 1}, ran
        assert info == dict(want, stages=stg, workgroups=workgroups(c, lens, c["cols"])), (info, want)
        assert y.shape == (4, rows, c["T"]) and guard.shape == (rows, c["T"])
        worst = 0.0
        for bi, L in enumerate(lens):
            e = float(np.max(np.abs(y[bi, :, :L].astype(np.float64) - refs[bi])))
            worst = max(worst, e)
            record(f"conv_x3_{c['name']}_stages{stg}_len{L}", e, GATE)
            assert e < GATE, (c["name"], stg, bi, L, e)                                                         # (a), (d)
            assert not y[bi, :, L:].any(), (c["name"], stg, bi, L, np.argwhere(y[bi, :, L:])[:4])               # (b)
        assert np.isnan(guard).all(), (c["name"], stg, np.argwhere(~np.isnan(guard))[:4])                        # (c)
        record(f"conv_x3_{c['name']}_stages{stg}", worst, GATE)
        outs[stg] = y
    for stg in STAGES[1:]:
        assert np.array_equal(outs[STAGES[0]], outs[stg]), (c["name"], stg, float(np.abs(outs[STAGES[0]] - outs[stg]).max()),
                                                            np.argwhere(outs[STAGES[0]] != outs[stg])[:4])
    # the launcher's own stage rule, and repeated calls: the split-K counters are back at
    # zero and the slabs are merged in split order
    option(cv.rt, "conv_stages", 0)
    for rep in range(3 if c["ksplit"] > 1 else 1):
        y, info, guard, ran = cv.run()
        assert info["stages"] == rule_stages(info["workgroups"]) and info["ksplit"] == c["ksplit"], info
        assert np.array_equal(y, outs[4]), (c["name"], rep, np.argwhere(y != outs[4])[:4])
        assert np.isnan(guard).all()
    if c["cols"]:
        # without the column table: the padded grid, the same split, the same sums
        option(cv.rt, "conv_cols", 0)
        y, info, guard, ran = cv.run()
        assert info == dict(want, cols=0, stages=rule_stages(workgroups(c, lens, 0)), workgroups=workgroups(c, lens, 0)), info
        assert np.array_equal(y, outs[4]), (c["name"], np.argwhere(y != outs[4])[:4])
        option(cv.rt, "conv_cols", 1)
    if c["p1"]:
        y3, info, guard, ran = cv.run(p1=0)                                                                       # (d): the floor
        assert ran == {tag(0): 1} and info["p1"] == 0, (ran, info)
        assert not np.array_equal(y3, outs[4])
        exact = [M.reference(c, d, bi) for bi in range(4)]
        e1, e3 = worst_err(outs[4], exact, lens), worst_err(y3, exact, lens)
        record(f"conv_x3_{c['name']}_vs_unrounded", e1, float("inf"))
        record(f"conv_x3_{c['name']}_three_products_vs_unrounded", e3, GATE)
        assert e3 < GATE and e1 > e3, (c["name"], e1, e3)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", M.REJECTS, ids=[n for n, _ in M.REJECTS])
def test_bad_shapes_are_refused_on_the_host_before_any_launch(name, kw):
    from detail_tts_amd.runtime import DttsError
    c = M.case(name, 64, 128, 1, 196, epi=0, ksplit=1, epi_vec=1)
    c.update(kw)
    d = M.make_data(c)
    cv = Conv(c, d)                                     # (weights packed for the bad shape itself: the refusal is the entry's, not a missing tensor's)

    def attempt():
        with pytest.raises(DttsError) as e:
            cv.rt.op_conv1d_x3("t", cv.x, c["cout"], c["k"], gate=c["gate"], res=cv.res, lens=cv.lens, p1=c["p1"])
        return str(e.value)
    msg, ran = launches_of(cv.rt, attempt, level=2)           # (level 2: the split passes would show too)
    assert "invalid argument" in msg and "op_conv1d_x3" in msg, msg
    assert ran == {}, ran


@pytest.mark.gpu
def test_conv_stages_option_takes_only_its_values(option):
    from detail_tts_amd.runtime import DttsError, Runtime
    r = Runtime({}, parts=(), extra={"t.bp": np.zeros(32, np.float32)})
    for bad in (1, 5):
        with pytest.raises(DttsError):
            r.set_option("conv_stages", bad)
    for ok in (2, 3, 4, 0):
        option(r, "conv_stages", ok)
