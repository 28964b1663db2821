"""CPU: the model behind tests/test_gpu_gpt_decode.py (tests/gpt_decode_model.py) is itself held to account - no GPU, no library.
  * the case table reaches every path the decode chain has: GEMV shape x NB x prologue, every batch size, column tails, the row clamp,
    every sum_parts body, every key-split count, empty and overshooting key ranges, the PV and score loop edges, in both attention forms;
  * the definitions equal torch's double LayerNorm, softmax and gelu(tanh); the kernel's algebra r (a - mu c) + d equals LayerNorm;
    the per-kernel references, chained, equal the GPT-2 block written in one piece, in the fused and in the split form;
  * every mutation a case claims moves the case's metric to >= 3 x the case's gate, and every mutation of the table is claimed;
  * every gate lies >= MARGIN x above the fp32 evaluation of the same definition (plus what rounding the kernel's inputs to fp32 once
    costs), so that it is fp32 arithmetic and not the kernel's order of summation that the gate allows for."""
import math

import numpy as np
import pytest

import gpt_decode_model as M

IDS = [c["name"] for c in M.ALL_CASES]


def test_case_table_reaches_every_path_of_the_decode_chain():
    reach = M.reached_paths()
    missing = [p for p in M.REQUIRED_PATHS if not reach.get(p)]
    assert not missing, missing
    assert len(set(IDS)) == len(IDS)
    for c in M.GEMV_CASES:                      # the shapes are what the launcher's rule makes of them, tails included
        r = c["rule"]
        assert (r["vec"], r["rpw"]) == {"n64": (1, 8), "n128": (1, 16), "wide": (4, 16)}[c["shape"]], c["name"]
        assert r["nb"] == (8 if c["B"] <= 8 else 16) and r["slices"] * r["rb"] == c["K"], c["name"]
    assert M.gemv_rule(128, 68, 1)["tail_cols"] == 4 and M.gemv_rule(768, 7940, 1)["tail_cols"] == 4
    # the production shapes of the reference config take the shapes the issue names
    assert M.gemv_rule(768, 8196, 8)["shape"] == "wide" and M.gemv_rule(768, 2304, 8)["shape"] == "n128"
    assert M.gemv_rule(3072, 768, 8)["shape"] == "n128" and M.gemv_rule(768, 768, 8)["shape"] == "n64"


def test_key_ranges_cover_every_cached_key_once():
    for nc in M.NC_ALL:
        for KS in range(1, 9):
            got = [s for lo, hi in M.key_ranges(nc, KS) for s in range(lo, hi)]
            assert got == list(range(nc)), (nc, KS)


def test_definitions_equal_torch_in_double():
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(0)
    x, g, b = 0.3 * (1 + rs.randn(5, 96)), rs.randn(96), rs.randn(96)
    t = torch.nn.functional.layer_norm(torch.from_numpy(x), (96,), torch.from_numpy(g), torch.from_numpy(b), M.LN_EPS).numpy()
    assert np.abs(M.layer_norm(x, g, b) - t).max() < 1e-13
    s = 4 * rs.randn(7, 300)
    assert np.abs(M.softmax(s) - torch.softmax(torch.from_numpy(s), -1).numpy()).max() < 1e-15
    z = 3 * rs.randn(4000)
    assert np.abs(M.gelu_new(z) - torch.nn.functional.gelu(torch.from_numpy(z), approximate="tanh").numpy()).max() < 1e-14
    assert np.abs(M.gelu_erf(z) - torch.nn.functional.gelu(torch.from_numpy(z)).numpy()).max() < 1e-14
    assert 1e-4 < np.abs(M.gelu_erf(z) - M.gelu_new(z)).max() < 1e-3            # the two GELUs are different functions


def test_the_layernorm_algebra_is_layernorm():
    """W^T LN(y) + b = r (W^T (gamma . y) - mu c) + d with c = W^T gamma, d = W^T beta + b, (mu, r) from per-slice (sum, sum of squares):
    exact in float64, before any rounding of the kernel's inputs"""
    rs = np.random.RandomState(1)
    y, g, bta, W, b = 0.02 * (1 + rs.randn(3, 192)), 1 + 0.3 * rs.randn(192), rs.randn(192), rs.randn(192, 64), rs.randn(64)
    direct = M.layer_norm(y, g, bta) @ W + b
    S = np.stack([y[:, i * 32:(i + 1) * 32].sum(-1) for i in range(6)]).sum(0)
    Q = np.stack([(y[:, i * 32:(i + 1) * 32] ** 2).sum(-1) for i in range(6)]).sum(0)
    mean = (S / 192)[:, None]
    rstd = 1 / np.sqrt((Q / 192)[:, None] - mean ** 2 + M.LN_EPS)
    assert np.abs(rstd * ((g * y) @ W - mean * (g @ W)) + (bta @ W + b) - direct).max() < 1e-10


def test_per_kernel_references_chained_equal_the_block_in_one_piece():
    d = M.layer_data()
    ref = M.layer_reference(d)
    for split in (False, True):
        k = M.layer_from_kernel_references(d, split=split)
        assert M.rel_err(k["h"], ref["h"]) < 1e-12 and M.rel_err(k["out"], ref["out"]) < 1e-12, split
    f32_fig = M.rel_err(M.layer_reference(d, np.float32)["out"], ref["out"])
    assert M.MARGIN * f32_fig <= M.GATES["layer"], f32_fig
    for m in M.LAYER["claims"]:
        for split in ((True,) if m == "merge_no_rescale" else (False, True)):
            e = M.rel_err(M.layer_from_kernel_references(d, m, split=split)["out"], ref["out"])
            assert e >= 3 * M.GATES["layer"], (m, split, e)


def test_every_mutation_is_claimed():
    claimed = {m for c in M.ALL_CASES for m in c["claims"]} | set(M.LAYER["claims"])
    assert claimed == set(M.MUTATIONS), claimed ^ set(M.MUTATIONS)


@pytest.mark.parametrize("c", M.ALL_CASES, ids=IDS)
def test_gate_sits_between_fp32_and_every_claimed_mutation(c):
    ref = M.reference_of(c)
    g = M.gate(c)
    # above: the definition in plain fp32, times MARGIN, plus the one rounding of the derived inputs (kernel model on the fp32 inputs
    # against the definition on the data they were derived from; 0 where the kernel's inputs ARE the definition's)
    fig = M.f32_figure(c)
    derived = c in M.ATTN_CASES or c.get("pro") == "lnparts"
    alg = M.case_err(c, M.reference_of(c, "algebra"), ref) if derived else 0.0
    assert M.MARGIN * fig + alg <= g, (c["name"], fig, alg, g)
    assert alg < 2e-6, (c["name"], alg)          # a few eps per slice: the kernel model IS the definition
    # below: a factor 3 under every mutation the case claims
    for m in c["claims"]:
        e = M.case_err(c, M.reference_of(c, m), ref)
        assert e >= 3 * g, (c["name"], m, e, g)


def test_planted_nan_sits_where_the_kernels_may_not_read():
    for c in M.GEMV_CASES:
        d = M.gemv_data(c["name"])
        K, B, n = c["K"], c["B"], c["in_slices"]
        if "x" in d:
            assert np.isnan(d["x"][B:]).all() and np.isnan(d["x"][:, K:]).all() and np.isfinite(d["x"][:B, :K]).all()
        if c["pro"] in ("ressum", "lnparts") and n:
            assert np.isnan(d["parts"][n:]).all() and np.isnan(d["parts"][:, :, K:]).all() and np.isfinite(d["parts"][:n, :, :K]).all()
        if c["pro"] == "lnparts":
            assert np.isnan(d["stats_in"][c["stats_slices"]:]).all() and np.isfinite(d["stats_in"][:c["stats_slices"]]).all()
            mean, sd = d["y"].mean(-1), d["y"].std(-1)
            assert (np.abs(mean / sd - 1) < 0.35).all(), c["name"]          # row mean ~ row standard deviation
    for c in M.ATTN_CASES:
        d = M.attn_data(c["name"])
        C, cap = c["C"], c["cap"]
        assert np.isnan(d["part"][c["slices"]:]).all() and np.isnan(d["part"][:, :, 3 * C:]).all() and np.isnan(d["stats"][c["stats_slices"]:]).all()
        for b, nc in enumerate(c["ncs"]):
            Kc, Vc = d["cache"][b, :C * cap].reshape(C, cap), d["cache"][b, C * cap:].reshape(cap, C)
            assert np.isnan(Kc[:, nc:]).all() and np.isnan(Vc[nc:]).all() and np.isfinite(Kc[:, :nc]).all() and np.isfinite(Vc[:nc]).all()
            assert d["lp"][b] + d["step"][b] == nc + 1 and d["lp"][b] >= 1
    ref = M.kv_reference(M.KV_CASE, M.kv_data())
    assert int(np.isfinite(ref).sum()) == 2 * M.KV_CASE["C"] * sum(M.KV_CASE["lens"])


def test_split_magnitudes_are_distinct_and_sum_to_the_total():
    rs = np.random.RandomState(2)
    total = rs.randn(3, 40)
    p = M.split_slices(rs, total, 7)
    assert np.isnan(p[7]).all() and np.abs(p[:7].astype(np.float64).sum(0) - total).max() < 1e-6
    mags = np.abs(p[:7]).mean((1, 2))
    assert (np.diff(mags) > 0).all() and mags[-1] > 2 * mags[0], mags
    assert math.isclose(M.rel_err(np.ones(3), np.ones(3) * 3), 2 / 3)
