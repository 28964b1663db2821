"""GPU parity of the exact-fp32 flash attention (csrc/attention.hip: flash_attn_kernel<D, MODE> in all 16 instantiations, and the VITS
relative-position kernels), one launch at a time through Runtime.op_attention / Runtime.op_attention_rel.  Everything that is not the
split-precision trunk runs on this kernel - the GPT prefill and every teacher-forced pass (causal), enc_p (band + ml, with the two rel
kernels), the MelStyleEncoders (plain), the trunk under conv_x3 = 0 (bias table, row stride Ta > T) - and the suite otherwise reaches it
only through whole blocks under the synthetic weights, where a band or bias index off by one, a clamp at 63 or a stale LDS tile moves a
block's output by less than the block gates.

The case table, its planted data, the float64 references and the mutation table are in tests/attn_f32_model.py;
tests/test_host_attn_f32.py shows on the CPU that every gate used here sits a factor 3 below every mutation a case claims.
  * test_attention: every case (ragged batch, NaN in every column >= len of qkv and band) against float64 in the metric
    max |y - ref| / max(1, max |ref|); ml only as ml[0] + log(ml[1]) against the log-sum-exp; outputs finite at t < len; columns >= len
    of y, ml, relk and the guard slab still all-NaN; a second call gives the same bits; every row run alone gives the bits it gave in
    the batch (the kernel has no cross-row state).  The composed entry is compared with the reference's pad / slice / skew attention.
  * test_bad_calls_...: each refused argument set raises DttsError with nothing launched, and a valid call right after it is right.
The measured figures are in profiles/attn_f32_measured_errors.txt (DTTS_TEST_LOG=<file> appends them run by run)."""
import functools

import numpy as np
import pytest

import attn_f32_model as M
from conftest import tol
from conv_tile_probe import launches_of

torch = pytest.importorskip("torch")

IDS = [c["name"] for c in M.CASES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def data_of(name):
    """(data, packed rows, float64 (out, lse) per sample): computed once, shared by the tests, never modified"""
    c = M.BY_NAME[name]
    d = M.make_data(c)
    refs = []
    for bi in range(len(d["lens"])):
        out, lse = M.reference(c, d, bi)
        refs.append((M.rel_reference(c, d, bi) if c["entry"] == "rel" else out, lse))
    return d, M.pack_rows(d["q"], d["k"], d["v"], c["layout"], c["cs"], d["lens"]), refs


@functools.lru_cache(maxsize=None)
def runtime():
    from detail_tts_amd.runtime import Runtime
    return Runtime({}, parts=(), extra={"unused": np.zeros(16, np.float32)})          # neither entry reads a weight


def launch(c, d, x, rows=slice(None)):
    """the case's entry on samples `rows` -> dict of numpy arrays (y, guard, ml, and relk for the composed entry)"""
    rt = runtime()
    lens = d["lens"][rows]
    qkv = dev(x[rows])
    if c["entry"] == "rel":
        y, relk, guard, ml = rt.op_attention_rel(qkv, c["H"], c["D"], dev(d["ek"]), dev(d["ev"]), c["W"], c["scale"], lens=lens, want_ml=True)
        return dict(y=y.cpu().numpy(), guard=guard.cpu().numpy(), ml=ml.cpu().numpy(), relk=relk.cpu().numpy())
    qo, ko, vo, hs = M.layout_args(c["layout"], c["H"], c["D"])
    y, ml, guard = rt.op_attention(qkv, c["H"], c["D"], qo, ko, vo, hs, c["scale"], lens=lens, T=c["T"], want_ml=True,
                                   bias_tab=dev(d["tab"]) if c["mode"] == "bias" else None, causal=c["mode"] == "causal",
                                   band=dev(d["band"][rows]) if c["mode"] == "band" else None, band_w=c["W"])
    return dict(y=y.cpu().numpy(), guard=guard.cpu().numpy(), ml=ml.cpu().numpy())


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("c", M.CASES, ids=IDS)
def test_attention(c):
    d, x, refs = data_of(c["name"])
    H, D, T, lens = c["H"], c["D"], c["T"], d["lens"]
    got = launch(c, d, x)
    y, ml = got["y"], got["ml"]
    assert y.shape == (len(lens), H * D, T) and ml.shape == (len(lens), H, T, 2)
    assert np.isnan(got["guard"]).all(), (c["name"], "guard slab written")
    for bi, L in enumerate(lens):
        assert np.isnan(y[bi, :, L:]).all() and np.isnan(ml[bi, :, L:]).all(), (c["name"], bi, L, "columns >= len must stay untouched")
        assert np.isfinite(y[bi, :, :L]).all() and np.isfinite(ml[bi, :, :L]).all(), (c["name"], bi, L)
        if "relk" in got:
            assert np.isnan(got["relk"][bi, :, L:]).all() and np.isfinite(got["relk"][bi, :, :L]).all(), (c["name"], bi, L)
        if L == 0:
            continue
        ref, lse = refs[bi]
        tol(f"attn_f32_{M.gate_key(c)}_{c['name']}_len{L}", M.rel_err(y[bi, :, :L].astype(np.float64), ref), M.gate(c))
        m, l = ml[bi, :, :L, 0].astype(np.float64), ml[bi, :, :L, 1].astype(np.float64)
        assert (l > 0).all(), (c["name"], bi)
        tol(f"attn_f32_lse_{c['name']}_len{L}", M.rel_err(m + np.log(l), lse), M.LSE_GATE)
    assert same_bits(got, launch(c, d, x)), (c["name"], "two calls differ")
    for bi, L in enumerate(lens):                          # a ragged row equals the same row run alone, bit for bit
        alone = launch(c, d, x, slice(bi, bi + 1))
        assert np.isnan(alone["guard"]).all()
        assert same_bits({k: v[0] for k, v in alone.items() if k != "guard"}, {k: v[bi] for k, v in got.items() if k != "guard"}), (c["name"], bi, L)


# ---- refusals
BASE = M.case("reject_base", "attn", 48, "plain", 2, 100, [100, 50], "head", "prec", std=2.0, claims=())
REL_BASE = M.case("reject_rel_base", "rel", 48, "band", 2, 100, [100, 50], "block", "prec", std=2.0, W=4, claims=())


@functools.lru_cache(maxsize=None)
def base_of(rel):
    c = REL_BASE if rel else BASE
    d = M.make_data(c)
    x = M.pack_rows(d["q"], d["k"], d["v"], c["layout"], c["cs"], d["lens"])
    return c, d, x, [M.rel_reference(c, d, bi) if rel else M.reference(c, d, bi)[0] for bi in range(2)]


def valid_call_is_right(rel):
    c, d, x, refs = base_of(rel)
    got = launch(c, d, x)
    for bi, L in enumerate(d["lens"]):
        e = M.rel_err(got["y"][bi, :, :L].astype(np.float64), refs[bi])
        assert e < M.gate(c) and np.isnan(got["y"][bi, :, L:]).all(), (bi, e)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,says", M.REJECTS, ids=[r[0] for r in M.REJECTS])
def test_bad_calls_are_refused_on_the_host_before_any_launch(name, kw, says):
    from detail_tts_amd.runtime import DttsError
    c, d, x, _ = base_of(False)
    rt = runtime()
    qo, ko, vo, hs = M.layout_args("head", 2, 48)
    a = dict(heads=2, dim=48, q_off=qo, k_off=ko, v_off=vo, head_stride=hs, lens=d["lens"], T=None, causal=False, band_w=0)
    a.update({k: v for k, v in kw.items() if k in a})
    qkv = dev(np.nan_to_num(x))
    tab = dev(np.zeros(kw["bias_shape"])) if "bias_shape" in kw else None
    band = dev(np.zeros(kw["band_shape"])) if "band_shape" in kw else None

    def attempt():
        with pytest.raises(DttsError) as e:
            rt.op_attention(qkv, a["heads"], a["dim"], a["q_off"], a["k_off"], a["v_off"], a["head_stride"], c["scale"], lens=a["lens"], T=a["T"],
                            bias_tab=tab, causal=a["causal"], band=band, band_w=a["band_w"], want_ml=True)
        return str(e.value)
    msg, ran = launches_of(rt, attempt, level=2)
    assert says in msg, msg
    assert ran == {}, ran
    valid_call_is_right(False)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,says", M.REL_REJECTS, ids=[r[0] for r in M.REL_REJECTS])
def test_bad_rel_calls_are_refused_on_the_host_before_any_launch(name, kw, says):
    from detail_tts_amd.runtime import DttsError
    c, d, x, _ = base_of(True)
    rt = runtime()
    a = dict(dim=48, window=4, lens=d["lens"], ek_shape=(9, 48), rows=288)
    a.update(kw)
    qkv = dev(np.nan_to_num(x))[:, : a["rows"]].contiguous()
    ek, ev = dev(np.zeros(a["ek_shape"])), dev(np.zeros((2 * a["window"] + 1, a["dim"])))
    if name == "window_8":
        ek = dev(np.zeros((17, 48)))
    if name == "dim32":
        ek, qkv = dev(np.zeros((9, 32))), qkv[:, :192].contiguous()

    def attempt():
        with pytest.raises(DttsError) as e:
            rt.op_attention_rel(qkv, 2, a["dim"], ek, ev, a["window"], c["scale"], lens=a["lens"])
        return str(e.value)
    msg, ran = launches_of(rt, attempt, level=2)
    assert says in msg, msg
    assert ran == {}, ran
    valid_call_is_right(True)
