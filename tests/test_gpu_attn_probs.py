"""GPU: the attention-probabilities kernel (csrc/attn_probs.hip, one launch at a time through Runtime.op_attn_probs) against float64
NumPy, on the planted and peaked random rows of tests/align_inputs.py (logit std about 5).

Per case (T in 1 .. 200 across the 16-query and 64-key tile seams, both row layouts, B = 3 ragged samples with a length 0, H = 3, so
every launch has several workgroups per sample):
  * HEADS on the case's windows - starting off any multiple of 16, reaching past t (exact zeros) and past len (rows left NaN) - equals
    the float64 causal softmax over ALL keys of the row; everything outside a sample's window and the guard slab stay NaN;
  * HEADS on the whole [T, T]: every live row sums to 1;
  * MEAN equals sum_h w_h HEADS, two calls are bit-equal, and accumulating "layer by layer" (first = False on the previous result)
    equals the float64 sum.
GATE is 20 x the worst error measured on the MI355X (profiles/attn_probs_measured_errors.txt, which also lists what each mutation of
the reference - dropped scale, s < t for s <= t, window-only denominator, key off by one - moves); the test asserts that the gate
stays below a tenth of the smallest of them.  DTTS_TEST_LOG=<file> appends the measured figures run by run."""
import functools

import numpy as np
import pytest

import align_inputs as AI
from conftest import tol

torch = pytest.importorskip("torch")

GATE = 4e-5          # max |P - P64|; about 20 x the worst measured, 1.80e-6 (profiles/attn_probs_measured_errors.txt)
ROWSUM_GATE = 6e-6   # |sum_s P - 1| over up to 200 keys; about 20 x the worst measured, 2.82e-7
CASES = [(T, layout) for T in AI.PROBS_T for layout in ("head", "block")]
WEIGHTS = np.array([0.5, 0.125, 0.375], np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def runtime():
    from detail_tts_amd.runtime import Runtime
    return Runtime({}, parts=(), extra={"unused": np.zeros(16, np.float32)})          # the entry reads no weight


@functools.lru_cache(maxsize=None)
def data_of(T, layout):
    """(case, float64 P [H, len, len] per sample): computed once, shared, never modified"""
    c = AI.probs_case(T, layout)
    return c, [AI.probs_reference(c["q"][b], c["k"][b], c["lens"][b], c["scale"]) if c["lens"][b] else None for b in range(c["B"])]


def launch(c, x=None, **kw):
    a = dict(lens=c["lens"], q0=c["q0"], nq=c["nq"], k0=c["k0"], nk=c["nk"])
    a.update(kw)
    return runtime().op_attn_probs(dev(c["x"]) if x is None else x, c["H"], c["D"], c["q_off"], c["k_off"], c["head_stride"], c["scale"], **a)


def check_window(name, got, P, c, b, combine=None):
    """got [.., nq_max, nk_max] of sample b against the float64 window; NaN exactly where the kernel writes nothing"""
    L, nq, nk = c["lens"][b], c["nq"][b], c["nk"][b]
    if L == 0:
        assert np.isnan(got).all(), (name, b, "a sample of length 0 was written")
        return
    ref = AI.window_of(P, L, c["q0"][b], nq, c["k0"][b], nk)
    if combine is not None:
        ref = combine(ref)
    win = got[..., :nq, :nk]
    assert np.array_equal(np.isnan(win), np.isnan(ref)), (name, b, "written / untouched elements")
    outside = np.ones(got.shape, bool)
    outside[..., :nq, :nk] = False
    assert np.isnan(got[outside]).all(), (name, b, "an element outside the window was written")
    live = ~np.isnan(ref)
    if live.any():
        tol(f"attn_probs_{name}_b{b}", np.abs(win[live].astype(np.float64) - ref[live]).max(), GATE)
    # keys s > t inside the window: exactly 0
    t = c["q0"][b] + np.arange(nq)[:, None]
    s = c["k0"][b] + np.arange(nk)[None, :]
    future = np.broadcast_to((s > t) & (t < L), win.shape)
    assert (win[future] == 0).all(), (name, b, "a key s > t is not exactly 0")


@pytest.mark.gpu
@pytest.mark.parametrize("T,layout", CASES, ids=[f"T{T}_{l}" for T, l in CASES])
def test_heads_windows_full_rows_and_mean(T, layout):
    c, refs = data_of(T, layout)
    B, H = c["B"], c["H"]
    x = dev(c["x"])
    name = f"T{T}_{layout}"
    # ---- HEADS on the windows
    out, guard = launch(c, x)
    heads = out.cpu().numpy()
    assert heads.shape == (B, H, max(c["nq"]), max(c["nk"])) and np.isnan(guard.cpu().numpy()).all(), "guard slab written"
    for b in range(B):
        check_window(name + "_heads", heads[b], refs[b], c, b)
    assert np.array_equal(launch(c, x)[0].cpu().numpy().view(np.uint32), heads.view(np.uint32)), "two calls differ"
    # ---- HEADS on the whole [T, T]: live rows sum to 1
    full, guard = launch(c, x, q0=[0] * B, nq=[T] * B, k0=[0] * B, nk=[T] * B)
    full = full.cpu().numpy()
    assert np.isnan(guard.cpu().numpy()).all()
    for b in range(B):
        L = c["lens"][b]
        assert np.isnan(full[b, :, L:]).all(), (b, "rows t >= len were written")
        if L:
            tol(f"attn_probs_{name}_rowsum_b{b}", np.abs(full[b, :, :L].astype(np.float64).sum(axis=2) - 1.0).max(), ROWSUM_GATE)
            tol(f"attn_probs_{name}_full_b{b}", np.abs(full[b, :, :L, :L].astype(np.float64) - refs[b]).max(), GATE)
            assert (full[b, :, :L, L:] == 0).all()
    # ---- MEAN = sum_h w_h HEADS
    mean, guard = launch(c, x, mode="mean", head_weights=WEIGHTS)
    mean_np = mean.cpu().numpy()
    assert mean_np.shape == (B, max(c["nq"]), max(c["nk"])) and np.isnan(guard.cpu().numpy()).all()
    w64 = WEIGHTS.astype(np.float64)
    for b in range(B):
        check_window(name + "_mean", mean_np[b], refs[b], c, b, combine=lambda r: np.einsum("h,hqk->qk", w64, r))
    from_heads = np.einsum("h,bhqk->bqk", w64, heads.astype(np.float64))
    live = ~np.isnan(from_heads)
    assert np.array_equal(np.isnan(mean_np), ~live)
    if live.any():
        tol(f"attn_probs_{name}_mean_vs_heads", np.abs(mean_np[live] - from_heads[live]).max(), GATE)
    again, _ = launch(c, x, mode="mean", head_weights=WEIGHTS)
    assert np.array_equal(again.cpu().numpy().view(np.uint32), mean_np.view(np.uint32)), "two MEAN calls differ"
    # ---- accumulating launch after launch (the model's layers): first = False adds to what the previous launch left
    acc, _ = launch(c, x, mode="mean", head_weights=WEIGHTS)
    w2 = np.array([0.25, 1.0, 0.0625], np.float32)
    acc, _ = launch(c, x, mode="mean", head_weights=w2, first=False, out=acc)
    acc = acc.cpu().numpy()
    for b in range(B):
        check_window(name + "_accumulated", acc[b], refs[b], c, b,
                     combine=lambda r: np.einsum("h,hqk->qk", w64 + w2.astype(np.float64), r))


def test_the_gate_sits_far_below_every_mutation():
    """CPU: what a wrong kernel would move, in EVERY case the GPU test runs, each case on its own (float64, tests/align_inputs.py).  The
    two T = 1 cases are left out: with a single key P is 1 whatever is done to the score (they test the tile edges, not the values)."""
    tab = AI.probs_mutation_table([data_of(T, layout)[0] for T, layout in CASES if T > 1])
    assert GATE < min(tab.values()) / 10, tab


BAD = [("dim64", dict(dim=64), "head dim 48"), ("query_window", dict(q0=[30, 8, 0]), "query window"),
       ("key_window", dict(k0=[-1, 0, 0]), "key window"), ("lens", dict(lens=[66, 1, 0]), "lengths must lie in [0, T]"),
       ("rows", dict(k_off=400), "rows leave the tensor")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,says", BAD, ids=[b[0] for b in BAD])
def test_bad_calls_are_refused_on_the_host_before_any_launch(name, kw, says):
    from conv_tile_probe import launches_of
    from detail_tts_amd.runtime import DttsError
    c, refs = data_of(65, "block")
    rt = runtime()
    a = dict(dim=c["D"], k_off=c["k_off"], lens=c["lens"], q0=c["q0"], nq=c["nq"], k0=c["k0"], nk=c["nk"])
    a.update(kw)
    x = dev(np.nan_to_num(c["x"]))

    def attempt():
        with pytest.raises(DttsError) as e:
            rt.op_attn_probs(x, c["H"], a["dim"], c["q_off"], a["k_off"], c["head_stride"], c["scale"], a["lens"], a["q0"], a["nq"], a["k0"], a["nk"])
        return str(e.value)
    msg, ran = launches_of(rt, attempt, level=2)
    assert says in msg and ran == {}, (msg, ran)
    out, _ = launch(c, x)                     # a valid call right after it is right
    check_window("after_" + name, out.cpu().numpy()[0], refs[0], c, 0)
