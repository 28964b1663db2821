"""GPU parity of the launch-per-GEMV decode chain (csrc/gpt_kernels.hip), one kernel launch at a time through Runtime.op_gemv_block,
op_decode_attention, op_gpt_final_ln, op_ln_fold_vectors and op_kv_to_cache on a handle without weights.  The chain streams every token
when the persistent token kernel is off and serves every session of more than 16 rows, and it is the yardstick test_gpu_gpt.py holds the
token kernels to; sessions reach it only on the reference shape (three GEMV shapes at one (K, CoutP) each, the fused attention, slice
counts 6 / 12 / 16 / 24) and behind a 10-layer tolerance.  Here every kernel is compared with a float64 reference of its definition at
every path its launcher and its loops have.

The case table, the planted data (NaN wherever a kernel may not read), the references, the mutation table and the gates are in
tests/gpt_decode_model.py; tests/test_host_gpt_decode.py shows on the CPU that every gate sits MARGIN x above the fp32 evaluation of the
same definition and a factor 3 below every mutation a case claims.  Per case: outputs within the gate and finite where defined, NaN
everywhere else (guard slabs, slices the launcher does not write, record padding, every cache cell but column pos), the instantiation the
launcher reports is the one the model derives, a second call gives the same bits, and every row run alone (B = 1) gives the bits it gave
in the batch.  Exact, without tolerance: which cells are written, and every cache byte outside column pos.  The k / v values AT pos
are the kernel's fp32 sums and are held to the float64 reference within the case's gate.
The measured figures are in profiles/gpt_decode_measured_errors.txt (DTTS_TEST_LOG=<file> appends them run by run)."""
import functools

import numpy as np
import pytest

import gpt_decode_model as M
from conftest import tol
from conv_tile_probe import launches_of

torch = pytest.importorskip("torch")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return None if t is None else t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def runtime():
    from detail_tts_amd.runtime import Runtime
    return Runtime({}, parts=(), extra={"unused": np.zeros(16, np.float32)})          # no entry here reads a weight


@functools.lru_cache(maxsize=None)
def dev_weight(K, N, tag="w", gain=1.0):
    return dev(M.weight(K, N, tag, gain))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- GEMV
def launch_gemv(c, d, row=None):
    """the case's launch on the whole batch, or on row `row` alone (B = 1) -> dict of numpy arrays + slices + shape"""
    B = c["B"] if row is None else 1
    rsel = slice(None) if row is None else slice(row, row + 1)
    kw = {}
    if "x" in d:                                           # the NaN rows behind the batch stay behind it
        kw["x"] = dev(d["x"] if row is None else np.concatenate([d["x"][rsel], d["x"][c["B"]:]]))
    if c["pro"] == "ressum":
        kw.update(in_bias=dev(d["in_bias"]), gamma=dev(d["gamma"]), in_slices=c["in_slices"])
        if c["in_slices"]:
            kw["parts"] = dev(d["parts"][:, rsel])
    elif c["pro"] == "lnparts":
        kw.update(parts=dev(d["parts"][:, rsel]), in_slices=c["in_slices"], in_act=c["act"], stats_in=dev(d["stats_in"][:, rsel]),
                  stats_slices=c["stats_slices"], K_ln=c["K_ln"], fold_c=dev(d["fold_c"]), fold_d=dev(d["fold_d"]))
    elif c["pro"] == "attn":
        kw.update(parts=dev(d["parts"][rsel]), in_slices=c["in_slices"], head_dim=c["head_dim"])
    r = runtime().op_gemv_block(c["pro"], dev_weight(c["K"], c["CoutP"]), B, **kw)
    return {k: (host(v) if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("c", M.GEMV_CASES, ids=[c["name"] for c in M.GEMV_CASES])
def test_gemv_block(c):
    d = M.gemv_data(c["name"])
    ref = M.gemv_reference(c, d)
    got = launch_gemv(c, d)
    r = c["rule"]
    assert got["shape"] == (r["vec"], r["rpw"], r["nb"]) and got["slices"] == r["slices"], (c["name"], got["shape"], got["slices"], r)
    assert got["part"].shape == (r["slices"], c["B"], c["CoutP"])
    assert np.isnan(got["guard"]).all(), (c["name"], "slices behind the launcher's were written")
    for k in ref:
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (c["name"], k)
        tol(f"gpt_decode_gemv_{c['name']}_{k}", M.rel_err(got[k], ref[k]), M.gate(c))
    if c["pro"] == "ressum":
        assert np.isnan(got["y_guard"]).all() and np.isnan(got["stats_guard"]).all(), c["name"]
    else:
        assert got["y_out"] is None and got["stats_out"] is None
    again = launch_gemv(c, d)
    for k in ref:
        assert same_bits(got[k], again[k]), (c["name"], k, "two calls differ")
    for b in range(c["B"]):                                # every row alone (the 8-row instantiation) gives the bits it gave in the batch
        alone = launch_gemv(c, d, b)
        assert alone["shape"] == (r["vec"], r["rpw"], 8) and np.isnan(alone["guard"]).all()
        assert same_bits(alone["part"][:, 0], got["part"][:, b]), (c["name"], b)
        if c["pro"] == "ressum":
            assert same_bits(alone["y_out"][0], got["y_out"][b]) and same_bits(alone["stats_out"][:, 0], got["stats_out"][:, b]), (c["name"], b)


# ---------------------------------------------------------------------------------------------------------------- attention
def launch_attn(c, d, row=None, **over):
    """-> dict(out, guard, cache) of numpy arrays; the cache is a fresh copy of the planted one, updated in place by the call"""
    rsel = slice(None) if row is None else slice(row, row + 1)
    B = c["B"] if row is None else 1
    cache = dev(d["cache"][rsel])
    kw = dict(ksplit=c["KS"], cap=c["cap"])
    if c["form"] == "fused":
        kw["wproj"] = dev_weight(c["C"], 768, "proj")
    kw.update(over)
    out, guard = runtime().op_decode_attention(dev(d["part"][:, rsel]), c["slices"], dev(d["stats"][:, rsel]), c["stats_slices"], dev(d["fold_c"]),
                                               dev(d["fold_d"]), cache, d["lp"][rsel], d["step"][rsel], B, c["H"], **kw)
    return dict(out=host(out), guard=host(guard), cache=host(cache))


def attn_got(c, r):
    """the launch's outputs in the shape of M.attn_reference's"""
    if c["form"] == "fused":
        return dict(partial=r["out"], cache=r["cache"])
    return dict(rec_m=r["out"][..., 0], rec_l=r["out"][..., 1], rec_o=r["out"][..., 2:2 + M.HEAD_DIM], cache=r["cache"])


def check_attention(c, d, ref, r, rows):
    """everything about one launch (rows = the case's rows it ran) but the bit comparisons"""
    C, cap, H = c["C"], c["cap"], c["H"]
    got = attn_got(c, r)
    assert np.isnan(r["guard"]).all(), (c["name"], "guard slab written")
    # exact: the cells written are column pos of K and row pos of V, every other cell keeps the planted bits
    planted = d["cache"][rows]
    for i, b in enumerate(rows):
        nc = c["ncs"][b]
        mask = np.zeros(2 * C * cap, bool)
        mask[:C * cap].reshape(C, cap)[:, nc] = True
        mask[C * cap:].reshape(cap, C)[nc] = True
        assert np.array_equal(bits(r["cache"][i])[~mask], bits(planted[i])[~mask]), (c["name"], b, "cache bytes outside column pos changed")
        assert np.isfinite(r["cache"][i][mask]).all(), (c["name"], b, "k / v of the new token missing")
    sub = {k: v[:, rows] if k == "partial" else v[rows] for k, v in ref.items()}
    assert M.cache_placement(got["cache"], sub["cache"]) == 0
    if c["form"] == "split":
        assert np.isnan(r["out"][..., 2 + M.HEAD_DIM:]).all(), (c["name"], "record padding written")
        live = np.isfinite(sub["rec_m"])
        assert np.array_equal(np.isneginf(got["rec_m"]), ~live) and np.isfinite(got["rec_m"][live]).all(), (c["name"], "empty key ranges")
        assert (got["rec_l"][~live] == 0).all() and (got["rec_o"][~live] == 0).all() and (got["rec_l"][live] > 0).all()
        assert np.isfinite(got["rec_l"]).all() and np.isfinite(got["rec_o"]).all()
    else:
        assert got["partial"].shape == (H, len(rows), 768) and np.isfinite(got["partial"]).all()
    return got, sub


@pytest.mark.gpu
@pytest.mark.parametrize("c", M.ATTN_CASES, ids=[c["name"] for c in M.ATTN_CASES])
def test_decode_attention(c):
    d = M.attn_data(c["name"])
    ref = M.attn_reference(c, d)
    rows = list(range(c["B"]))
    r = launch_attn(c, d)
    got, sub = check_attention(c, d, ref, r, rows)
    fin = ~np.isnan(sub["cache"])
    tol(f"gpt_decode_attn_{c['name']}_kv_at_pos", M.rel_err(got["cache"][fin], sub["cache"][fin]), M.gate(c))
    if c["form"] == "split":
        live = np.isfinite(sub["rec_m"])
        for k in ("rec_m", "rec_l", "rec_o"):
            tol(f"gpt_decode_attn_{c['name']}_{k}", M.rel_err(got[k][live], sub[k][live]), M.gate(c))
        merged = M.merge_records(got["rec_m"].astype(np.float64), got["rec_l"].astype(np.float64), got["rec_o"].astype(np.float64))
        tol(f"gpt_decode_attn_{c['name']}_merged", M.rel_err(merged.reshape(sub["out"].shape), sub["out"]), M.gate(c))
    else:
        tol(f"gpt_decode_attn_{c['name']}_partial", M.rel_err(got["partial"], sub["partial"]), M.gate(c))
    assert M.attn_err(c, got, sub) < M.gate(c)
    again = launch_attn(c, d)
    assert same_bits(r["out"], again["out"]) and same_bits(r["cache"], again["cache"]), (c["name"], "two calls differ")
    for b in rows:                                         # a ragged row equals the same row run alone, bit for bit
        alone = launch_attn(c, d, b)
        check_attention(c, d, ref, alone, [b])
        a, g = (alone["out"][:, 0], r["out"][:, b]) if c["form"] == "fused" else (alone["out"][0], r["out"][b])
        assert same_bits(a, g) and same_bits(alone["cache"][0], r["cache"][b]), (c["name"], b)


# ---------------------------------------------------------------------------------------------------------------- the small kernels
def launch_final_ln(c, d, row=None):
    rsel = slice(None) if row is None else slice(row, row + 1)
    B = c["B"] if row is None else 1
    lat = runtime()._nan(B + 1, c["C"], c["lat_cs"]) if c["lat_cs"] else None
    y, guard = runtime().op_gpt_final_ln(dev(d["res"][rsel]), dev(d["g1"]), dev(d["b1"]), dev(d["g2"]), dev(d["b2"]),
                                         bias=dev(d["bias"]) if "bias" in d else None, parts=dev(d["parts"][:, rsel]) if c["in_slices"] else None,
                                         in_slices=c["in_slices"], step=c["steps"][rsel], max_steps=c["max_steps"],
                                         latents=None if lat is None else lat[:B])
    return dict(y=host(y), guard=host(guard), lat=host(lat))


@pytest.mark.gpu
@pytest.mark.parametrize("c", M.FINAL_LN_CASES, ids=[c["name"] for c in M.FINAL_LN_CASES])
def test_final_layernorms(c):
    d = M.final_ln_data(c["name"])
    ref = M.final_ln_reference(c, d)["y"]
    got = launch_final_ln(c, d)
    assert got["y"].shape == ref.shape and np.isfinite(got["y"]).all() and np.isnan(got["guard"]).all()
    tol(f"gpt_decode_{c['name']}", M.rel_err(got["y"], ref), M.gate(c))
    if c["lat_cs"]:                                        # column step[b] of the latents holds y[b] when step[b] < max_steps; nothing else is written
        want = np.full((c["B"] + 1, c["C"], c["lat_cs"]), np.nan, np.float32)
        for b, st in enumerate(c["steps"]):
            if st < c["max_steps"]:
                want[b, :, st] = got["y"][b]
        assert np.array_equal(bits(got["lat"]), bits(want)), c["name"]
    assert same_bits(got["y"], launch_final_ln(c, d)["y"])
    for b in range(c["B"]):
        alone = launch_final_ln(c, d, b)
        assert same_bits(alone["y"][0], got["y"][b]) and np.isnan(alone["guard"]).all(), (c["name"], b)


@pytest.mark.gpu
@pytest.mark.parametrize("c", M.FOLD_CASES, ids=[c["name"] for c in M.FOLD_CASES])
def test_ln_fold_vectors(c):
    d = M.fold_data(c["name"])
    ref = M.fold_reference(c, d)

    def run():
        cc, dd, guard = runtime().op_ln_fold_vectors(dev(d["W"]), dev(d["gamma"]), dev(d["beta"]), dev(d["bias"]) if "bias" in d else None)
        return dict(c=host(cc), d=host(dd)), host(guard)
    got, guard = run()
    assert np.isnan(guard).all() and np.isfinite(got["c"]).all() and np.isfinite(got["d"]).all()
    for k in ("c", "d"):
        tol(f"gpt_decode_{c['name']}_{k}", M.rel_err(got[k], ref[k]), M.gate(c))
    again, _ = run()
    assert same_bits(got["c"], again["c"]) and same_bits(got["d"], again["d"])


@pytest.mark.gpu
def test_kv_to_cache_places_every_value_and_nothing_else():
    c = M.KV_CASE
    qkv = M.kv_data()
    ref = M.kv_reference(c, qkv)
    cache, guard = runtime().op_kv_to_cache(dev(qkv), c["lens"], c["cap"])
    assert np.isnan(host(guard)).all()
    assert np.array_equal(bits(host(cache)), bits(ref))          # a copy: exact, NaN cells included
    for b, n in enumerate(c["lens"]):
        alone, g1 = runtime().op_kv_to_cache(dev(qkv[b:b + 1]), [n], c["cap"])
        assert np.array_equal(bits(host(alone)[0]), bits(ref[b])) and np.isnan(host(g1)).all(), b


# ---------------------------------------------------------------------------------------------------------------- refusals
GEMV_BASE = M.GEMV_BY_NAME["plain_n64_B9"]
ATTN_BASE = M.ATTN_BY_NAME["split_ks2"]


def valid_calls_are_right():
    c, d = GEMV_BASE, M.gemv_data(GEMV_BASE["name"])
    assert M.rel_err(launch_gemv(c, d)["part"], M.gemv_reference(c, d)["part"]) < M.gate(c)
    c, d = ATTN_BASE, M.attn_data(ATTN_BASE["name"])
    got, sub = check_attention(c, d, M.attn_reference(c, d), launch_attn(c, d), list(range(c["B"])))
    assert M.attn_err(c, got, sub) < M.gate(c)


@pytest.mark.gpu
@pytest.mark.parametrize("name,entry,kw,says", M.REJECTS, ids=[r[0] for r in M.REJECTS])
def test_bad_calls_are_refused_on_the_host_before_any_launch(name, entry, kw, says):
    from detail_tts_amd.runtime import DttsError
    rt = runtime()
    if entry == "gemv":
        K, N, B = kw.get("K", 128), kw.get("CoutP", 68), kw.get("B", 3)
        W, x = dev(np.zeros((K, N))), dev(np.zeros((B, K)))

        def call():
            rt.op_gemv_block("plain", W, B, x=x)
    else:
        c = ATTN_BASE if "wproj_cols" not in kw else M.ATTN_BY_NAME["fused_small"]
        d = M.attn_data(c["name"])
        cap = kw.get("cap", c["cap"])                      # one row is enough: 16384 columns of cache are 12 MB per row at C = 96
        part, stats = dev(np.nan_to_num(d["part"][:, :1])), dev(np.nan_to_num(d["stats"][:, :1]))
        fc, fd = dev(np.nan_to_num(d["fold_c"])), dev(np.nan_to_num(d["fold_d"]))
        cache = dev(np.zeros((1, 2 * c["C"] * cap)))
        wproj = dev(np.zeros((c["C"], kw["wproj_cols"]))) if "wproj_cols" in kw else None

        def call():
            rt.op_decode_attention(part, c["slices"], stats, c["stats_slices"], fc, fd, cache, d["lp"][:1], d["step"][:1], 1, c["H"],
                                   ksplit=0 if wproj is not None else 2, wproj=wproj, dim=kw.get("dim", 48), cap=cap)

    def attempt():
        with pytest.raises(DttsError) as e:
            call()
        return str(e.value)
    msg, ran = launches_of(rt, attempt, level=2)
    assert says in msg, msg
    assert ran == {}, ran
    # the profiler does see these entries' launches: a valid call shows up in it, and is right
    _, ran = launches_of(rt, valid_calls_are_right, level=2)
    assert ran.get("gemv_block_kernel<1,8,16>") == 1 and ran.get("decode_attention_qkv_kernel<48,split>") == 1, ran


# ---------------------------------------------------------------------------------------------------------------- one whole layer
@pytest.mark.gpu
def test_one_layer_through_the_unit_entries_fused_and_split():
    """A GPT-2 block on the reference shape (C = 768, 16 heads, 3072 inner), 3 ragged rows at up to 300 keys, as gpt_step_launches strings
    the kernels together: K1 ressum GEMV -> attention (fused with its projection, or key-split KS = 2 + the GP_ATTN GEMV) -> K4 ressum GEMV
    -> K5 lnparts GEMV -> the next layer's K1, whose y_out is the block's output.  Both forms against the float64 block, and each other."""
    rt, c, d = runtime(), M.LAYER, M.layer_data()
    ref = M.layer_reference(d)
    C, F, B, H = c["C"], c["F"], c["B"], c["H"]
    Wa, Wp, Wfc, Wfc2 = dev_weight(C, 3 * C, "attn", 1.5), dev_weight(C, 768, "proj"), dev_weight(C, F, "lfc"), dev_weight(F, C, "lfc2")
    g1, b1, g2, b2 = (dev(d[k]) for k in ("g", "b", "g2", "b2"))
    ca, da, _ = rt.op_ln_fold_vectors(Wa, g1, b1, dev(d["bias"]))
    cf, df, _ = rt.op_ln_fold_vectors(Wfc, g2, b2, dev(d["bfc"]))
    outs = {}
    for form in ("fused", "split"):
        k1 = rt.op_gemv_block("ressum", Wa, B, x=dev(d["x"]), gamma=g1)
        assert k1["shape"] == (1, 16, 8) and k1["slices"] == 6
        cache = dev(d["cache"])
        if form == "fused":
            part2, _ = rt.op_decode_attention(k1["part"], 6, k1["stats_out"], 6, ca, da, cache, d["lp"], d["step"], B, H, wproj=Wp, cap=c["cap"])
            n2 = H
        else:
            rec, _ = rt.op_decode_attention(k1["part"], 6, k1["stats_out"], 6, ca, da, cache, d["lp"], d["step"], B, H, ksplit=2, cap=c["cap"])
            k3 = rt.op_gemv_block("attn", Wp, B, parts=rec, in_slices=2, head_dim=M.HEAD_DIM)
            assert k3["shape"] == (1, 8, 8) and k3["slices"] == 12
            part2, n2 = k3["part"], 12
        k4 = rt.op_gemv_block("ressum", Wfc, B, x=k1["y_out"], parts=part2, in_slices=n2, in_bias=dev(d["bproj"]), gamma=g2)
        k5 = rt.op_gemv_block("lnparts", Wfc2, B, parts=k4["part"], in_slices=k4["slices"], in_act=4, stats_in=k4["stats_out"],
                              stats_slices=k4["slices"], K_ln=C, fold_c=cf, fold_d=df)
        assert k5["shape"] == (1, 16, 8) and k5["slices"] == 24
        nxt = rt.op_gemv_block("ressum", Wa, B, x=k4["y_out"], parts=k5["part"], in_slices=24, in_bias=dev(d["bfc2"]), gamma=g1)
        outs[form] = (host(k4["y_out"]), host(nxt["y_out"]))
        assert np.isfinite(outs[form][1]).all()
        tol(f"gpt_decode_layer_{form}_h", M.rel_err(outs[form][0], ref["h"]), M.GATES["layer"])
        tol(f"gpt_decode_layer_{form}_out", M.rel_err(outs[form][1], ref["out"]), M.GATES["layer"])
    tol("gpt_decode_layer_fused_vs_split", M.rel_err(outs["fused"][1], outs["split"][1]), M.GATES["layer"])


# ---------------------------------------------------------------------------------------------------------------- sessions in the split form
@pytest.fixture(scope="module")
def gpt_rt(weights):
    from detail_tts_amd.runtime import Runtime
    return Runtime(weights, folded=True, parts=("gpt",))


@pytest.mark.gpu
def test_sessions_in_the_split_form(gpt_rt, golden):
    """Option gpt_fuse_proj = 0: the chain's attention leaves key-split records and the GP_ATTN GEMV projects them.  The gpt_forced golden
    session stays within 2e-4 of the reference's latents with the same codes, and a ragged 3-row forced session agrees between the two
    forms within the 2e-4 test_token_kernel_equals_the_launch_per_gemv_chain allows between chain and token kernel."""
    rt = gpt_rt
    g = golden("gpt_forced")
    n = g["codes"].shape[1]
    rs = np.random.RandomState(91)
    refer = (rs.randn(3, 128, 90) * 2 - 5).astype(np.float32)
    rl = [90, 71, 55]
    texts = [np.concatenate([rs.randint(3, 255, 5 + 4 * b), [0]]).astype(np.int32) for b in range(3)]
    forced = [rs.randint(0, 8192, 24).astype(np.int32) for _ in range(3)]
    assert rt.get_option("gpt_fuse_proj") == 1
    rt.set_option("gpt_token_kernel", 0)
    try:
        res = {}
        for fuse in (1, 0):
            rt.set_option("gpt_fuse_proj", fuse)
            assert rt.get_option("gpt_fuse_proj") == fuse
            codes, ncodes, lat = rt.gpt_generate(dev(g["refer"]), None, [g["text"][0]], 1, [0], max_generate_length=n + 1, forced_codes=[g["codes"][0]])
            assert np.array_equal(codes[0, :n], g["codes"][0]) and codes[0, n] == 8193 and ncodes[0] == n + 1, fuse
            e = float(np.abs(host(lat)[:, :, :n].astype(np.float64) - g["latent"].transpose(0, 2, 1)).max())
            tol(f"gpt_decode_session_golden_fuse{fuse}", e, 2e-4)
            c3, n3, l3 = rt.gpt_generate(dev(refer), rl, texts, 5, [1, 2, 3], max_generate_length=25, forced_codes=forced)
            res[fuse] = (c3.copy(), n3.copy(), l3.clone())
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        tol("gpt_decode_session_ragged_fuse0_vs_fuse1", float((res[0][2] - res[1][2]).abs().max()), 2e-4)
    finally:
        rt.set_option("gpt_fuse_proj", 1)
        rt.set_option("gpt_token_kernel", 1)
