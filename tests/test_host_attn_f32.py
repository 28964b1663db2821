"""CPU side of tests/test_gpu_attn_f32.py (references, mutations, data and case table: tests/attn_f32_model.py).
  * Every mutation of the float64 reference is claimed by at least one case, and on every claiming case the mutated reference differs
    from the true one by >= 3 x the case's gate in the gate's own metric: so the gates of the GPU test separate a right kernel from each
    of these wrong ones.  The one exception is shown to be one: the band applied at a padded query changes no output (NO_OUTPUT_EFFECT).
  * The pointer data points: >= 10 nats between the chosen key and the runner-up, at the keys the table says.
  * The table covers every production (D, mode) pair, every instantiation, both row layouts, cs == T and cs > T, every length class,
    and launches with more than 8 workgroups of distinct heads.
  * The references agree with a per-query brute-force loop on tiny cases, and the kernels' band formulation of the relative-position
    attention agrees with the reference's pad / slice / skew Python."""
import functools

import numpy as np
import pytest

import attn_f32_model as M

IDS = [c["name"] for c in M.CASES]


@functools.lru_cache(maxsize=None)
def data_of(name):
    return M.make_data(M.BY_NAME[name])


def truth(c, d, bi):
    return M.rel_reference(c, d, bi) if c["entry"] == "rel" else M.reference(c, d, bi)[0]


def test_no_gate_exceeds_the_cap():
    assert all(0 < g <= M.GATE_CAP for g in M.GATES.values()) and 0 < M.LSE_GATE <= M.GATE_CAP


def test_every_mutation_is_claimed_somewhere():
    claimed = set().union(*(c["claims"] for c in M.CASES))
    assert claimed == set(M.MUTATIONS) - set(M.NO_OUTPUT_EFFECT), sorted(set(M.MUTATIONS) - claimed)
    assert not claimed & set(M.NO_OUTPUT_EFFECT)


@pytest.mark.parametrize("c", M.CASES, ids=IDS)
def test_claimed_mutations_land_above_three_gates(c):
    d = data_of(c["name"])
    refs = [truth(c, d, bi) for bi in range(len(d["lens"]))]
    for mut in c["claims"]:
        e = max(M.rel_err(M.reference(c, d, bi, mut)[0], refs[bi]) for bi in range(len(d["lens"])))
        print(f"{c['name']}\t{mut}\t{e:.3e}")
        assert e >= 3 * M.gate(c), (c["name"], mut, e)


@pytest.mark.parametrize("c", [c for c in M.CASES if c["mode"] == "band"], ids=[c["name"] for c in M.CASES if c["mode"] == "band"])
def test_band_at_a_padded_query_changes_no_output(c):
    """with NaN in every band row >= len, as the entries hand them over"""
    d = data_of(c["name"])
    for bi, L in enumerate(d["lens"]):
        a, la = M.reference(c, d, bi, "band_pad_query")
        b, lb = M.reference(c, d, bi)
        assert np.array_equal(a, b) and np.array_equal(la, lb) and np.isfinite(a).all(), (c["name"], bi)


@pytest.mark.parametrize("c", [c for c in M.CASES if c["entry"] == "rel"], ids=[c["name"] for c in M.CASES if c["entry"] == "rel"])
def test_band_formulation_is_the_references_skew(c):
    d = data_of(c["name"])
    for bi in range(len(d["lens"])):
        a, b = M.reference(c, d, bi)[0], M.rel_reference(c, d, bi)
        assert a.shape == b.shape and M.rel_err(a, b) < 1e-12, (c["name"], bi)


@pytest.mark.parametrize("c", [c for c in M.CASES if c["kind"].endswith("_ptr")], ids=[c["name"] for c in M.CASES if c["kind"].endswith("_ptr")])
def test_pointer_margins_hold(c):
    d = data_of(c["name"])
    H, W = c["H"], c["W"]
    for bi, L in enumerate(d["lens"]):
        if L == 0:
            continue
        key = M.pointed_key(c, d, bi)
        t = np.arange(L)
        if c["kind"] == "score_ptr":
            assert M.score_margin(c, d, bi) >= 10.0, (c["name"], bi, M.score_margin(c, d, bi))
            assert np.array_equal(key, np.broadcast_to(M.pointer_targets(L, c["mode"] == "causal"), key.shape)), (c["name"], bi)
            continue
        q, k = np.asarray(d["q"][bi], np.float64), np.asarray(d["k"][bi], np.float64)
        band = c["scale"] * np.einsum("hct,rc->htr", q[:, :, :L], np.asarray(d["ek"], np.float64)) if c["entry"] == "rel" else \
            (d["band"][bi] if "band" in d else None)
        s = np.sort(M.scores64(c, q, k, L, d.get("tab"), band)[0], axis=-1)
        for h in range(H):
            o = c["offsets"][h % len(c["offsets"])] if c["kind"] == "bias_ptr" else (bi * H + h) % (2 * W + 1) - W
            if abs(o) == M.CLIP and c["kind"] == "bias_ptr":
                continue                                  # the shared far bucket: every key beyond +-64 carries the entry, no single target
            hit = (t + o >= 0) & (t + o < L)
            assert np.array_equal(key[h, hit], (t + o)[hit]), (c["name"], bi, h, o)
            if L > 1 and hit.any():
                assert (s[h, hit, -1] - s[h, hit, -2]).min() >= 10.0, (c["name"], bi, h, o)
        if c["kind"] == "band_ptr" and L > 2 * W:          # queries at t < W and t >= len - W lose their target at some offset
            assert any(not ((t + o >= 0) & (t + o < L)).all() for o in range(-W, W + 1))


def test_pointer_offsets_cover_the_table():
    by = M.BY_NAME
    assert set(M.BIAS_OFFSETS) <= set(by["trunk_bias_d48_ptr"]["offsets"][: by["trunk_bias_d48_ptr"]["H"]])
    for name in ("encp_rel_d48_ptr", "band_d48_ptr"):
        c = by[name]
        assert {(bi * c["H"] + h) % (2 * c["W"] + 1) for bi in range(len(c["lens"])) for h in range(c["H"])} == set(range(2 * c["W"] + 1)), name
    # score pointers: key 0, key len - 1, both sides of every 64-key seam, and for causal the diagonal
    for name in ("gpt_causal_d48_ptr", "style_plain_d64_ptr"):
        c = by[name]
        L = c["lens"][0]
        pi = M.pointer_targets(L, c["mode"] == "causal")
        want = {0} | {e for kt in range(1, -(-L // M.KT)) for e in (M.KT * kt - 1, M.KT * kt)}
        assert want <= set(pi.tolist()), (name, sorted(want - set(pi.tolist())))
        if c["mode"] == "causal":
            assert (pi == np.arange(L)).sum() >= L // 8
        else:
            assert L - 1 in set(pi.tolist())


def test_case_table_coverage():
    names = [c["name"] for c in M.CASES]
    assert len(set(names)) == len(names)
    pairs = {(c["D"], c["mode"]) for c in M.CASES}
    assert pairs == {(D, m) for D in M.DIMS for m in M.MODES}                      # all 16 instantiations
    for site, pair in M.PRODUCTION.items():                                          # every production pair, named, in its own layout
        mine = [c for c in M.CASES if c["prod"] == site]
        assert mine and all((c["D"], c["mode"]) == pair for c in mine), site
        assert any(c["layout"] == ("head" if site == "trunk" else "block") for c in mine), site
    assert any(c["prod"] == "trunk" and c["cs"] > c["T"] for c in M.CASES)
    assert any(c["prod"] == "enc_p" and c["entry"] == "rel" and c["W"] == 4 and c["H"] == 4 for c in M.CASES)
    assert {c["layout"] for c in M.CASES} == {"head", "block"}
    assert any(c["cs"] == c["T"] for c in M.CASES) and any(c["cs"] > c["T"] for c in M.CASES)
    for c in M.CASES:
        assert 130 <= c["T"] <= 400 and c["T"] <= c["cs"] and 2 <= len(c["lens"]) <= 4 and max(c["lens"]) == c["lens"][0] == c["T"], c["name"]
        assert set(c["claims"]) <= set(M.MUTATIONS), c["name"]
    lens = {L for c in M.CASES for L in c["lens"]}
    assert {0, 1, 31, 33, 63, 64, 65, 128, 129} <= lens, sorted(lens)
    # a length that leaves idle waves beside active ones in a block; a second query block with a cut causal key loop and a third tile
    assert any(L % M.QPB and L % M.QPB <= M.QPB - M.QPW for L in lens)
    assert any(c["mode"] == "causal" and any(M.QPB < L < 2 * M.QPB for L in c["lens"]) for c in M.CASES)
    assert any(c["D"] <= 96 and max(c["lens"]) > 2 * M.KT for c in M.CASES) and any(c["D"] == 192 and max(c["lens"]) > 2 * M.KT for c in M.CASES)
    # the XCD remap: more than 8 workgroups of distinct heads in one launch
    assert any(c["H"] > 8 for c in M.CASES if c["prod"] in ("gpt", "trunk"))
    kinds = {(c["kind"], c["std"]) for c in M.CASES}
    assert {("prec", 0.6), ("prec", 2.0), ("prec", 5.0), ("ramp", 1.0), ("bias_ptr", 0.0), ("band_ptr", 0.0), ("score_ptr", 0.0)} <= kinds


def test_random_scores_have_the_std_asked_for():
    for c in M.CASES:
        if c["kind"] != "prec":
            continue
        d = data_of(c["name"])
        s = c["scale"] * np.einsum("hct,hcs->hts", d["q"][0].astype(np.float64), d["k"][0].astype(np.float64))
        assert abs(s.std() / c["std"] - 1.0) < 0.1, (c["name"], s.std())


TINY = [M.case(f"tiny_{mode}", "attn", 48, mode, 2, 70, [70, 5, 1], lay, "prec", std=2.0, W=4 if mode == "band" else 0, claims=())
        for mode, lay in zip(M.MODES, ("head", "block", "head", "block"))] + \
       [M.case("tiny_rel", "rel", 48, "band", 2, 70, [70, 5, 1], "block", "prec", std=2.0, W=4, claims=())]


@pytest.mark.parametrize("c", TINY, ids=[c["name"] for c in TINY])
def test_references_agree_with_a_per_query_loop(c):
    d = M.make_data(c)
    for bi in range(len(d["lens"])):
        out, lse = M.reference(c, d, bi)
        bo, bl = M.brute_force(c, d, bi)
        assert M.rel_err(out, bo) < 1e-12 and M.rel_err(lse, bl) < 1e-12, (c["name"], bi)
        if c["entry"] == "rel":
            assert M.rel_err(M.rel_reference(c, d, bi), bo) < 1e-12, (c["name"], bi)


def test_packed_rows_hold_nan_beyond_every_length():
    for c in (M.BY_NAME["trunk_bias_d48_h16"], M.BY_NAME["gpt_causal_d48_h16"]):
        d = data_of(c["name"])
        x = M.pack_rows(d["q"], d["k"], d["v"], c["layout"], c["cs"], d["lens"])
        qo, ko, vo, hs = M.layout_args(c["layout"], c["H"], c["D"])
        assert x.shape == (len(d["lens"]), 3 * c["H"] * c["D"], c["cs"])
        for bi, L in enumerate(d["lens"]):
            assert np.isnan(x[bi, :, L:]).all() and np.isfinite(x[bi, :, :L]).all()
            for h in (0, c["H"] - 1):
                for off, a in ((qo, d["q"]), (ko, d["k"]), (vo, d["v"])):
                    assert np.array_equal(x[bi, off + h * hs: off + h * hs + c["D"], :L], a[bi, h, :, :L])
