"""CPU side of tests/test_gpu_conv_x3.py: on the data of every case of its table (tests/conv_x3_model.py) the numpy emulation of the
split-precision scheme stays below the 2e-5 gate against float64, and every seeded fault - a cross product dropped, the low plane of
one input column at a tile seam zeroed, one tap dropped in one column, the bias of one row omitted - lands above it.  So the gate the
GPU test applies to csrc/conv_x3.hip can tell a right kernel from each of these wrong ones.  The table itself is checked against the
launcher's rule (launch_conv_x3) written out in Python: a case that no longer lands on the variant it names is a table error."""
import numpy as np
import pytest

import conv_x3_model as M

IDS = [c["name"] for c in M.CASES]


def err(a, b):
    return float(np.max(np.abs(a - b)))


def seam_cols(c):
    """columns on both sides of the first tile seam (every case has T > 192)"""
    assert c["T"] > M.BN
    return [M.BN - 1, M.BN]


@pytest.mark.parametrize("c", M.CASES, ids=IDS)
def test_scheme_is_below_the_gate_and_every_seeded_fault_above(c):
    d = M.make_data(c)
    # the scheme, every sample (lengths T, a multiple of the tile, that + 1, 1)
    for bi in range(4):
        ref = M.reference(c, d, bi, rounded=bool(c["p1"]))
        e = err(M.emulate(c, d, bi), ref)
        assert e < M.GATE, (c["name"], bi, e)
        if not c["p1"]:
            assert e < 2e-6, (c["name"], bi, e)          # (the scheme itself: 3 - 6e-7 of O(1) outputs, a tenth of the gate at most)
    # faults, on the full-length sample
    ref = M.reference(c, d, 0, rounded=bool(c["p1"]))
    sch = M.Scheme(c, d, 0)
    faults = {}
    if not c["p1"]:
        faults["no_w0_x1"] = sch.result(terms=((0, 0), (1, 0)))
        faults["no_w1_x0"] = sch.result(terms=((0, 0), (0, 1)))
        for col in seam_cols(c):
            faults[f"low_plane_zero_col{col}"] = sch.result(zero_low_col=col)
    k = c["k"]
    # (k = 3: tap 2 of column 191 reads column 192 - the tile's halo column; tap 0 of column 192 reads the previous tile's last column)
    faults["tap_dropped_col191"] = sch.result(skip=(k - 1, M.BN - 1))
    faults["tap_dropped_col192"] = sch.result(skip=(0, M.BN))
    faults["bias_row_omitted"] = sch.result(skip_bias_row=c["cout"] - 1)
    for name, y in faults.items():
        e = err(y, ref)
        assert e > M.GATE, (c["name"], name, e)
    if c["p1"]:
        # one product against the UNROUNDED reference: above the gate, and above the three-product scheme - what makes the
        # fp16-rounded reference of the GPU test the right one, and its "differs from three products" floor meaningful
        exact = M.reference(c, d, 0)
        e1, e3 = err(sch.result(), exact), err(sch.result(terms=M.ALL_TERMS), exact)
        assert e1 > M.GATE > e3, (c["name"], e1, e3)


def test_the_term_table_equals_a_direct_conv_of_the_planes():
    c = M.CASES[[x["name"] for x in M.CASES].index("epi1_tanh_k3_T388")]
    d = M.make_data(c)
    L = d["lens"][0]
    xs = list(M.split(d["x"][0, :, :L], M.SCALE_X))
    ws = M.split(d["w"], M.SCALE_W)
    xs[1][:, 192] = 0.0
    acc = sum(M.conv64(xs[px], ws[pw], skip=(2, 191)) for pw, px in M.ALL_TERMS)
    direct = M.epilogue64(c, d, 0, acc / (M.SCALE_X * M.SCALE_W))
    assert err(direct, M.emulate(c, d, 0, zero_low_col=192, skip=(2, 191))) < 1e-12


def test_case_table_lands_on_the_variants_it_names_and_covers_every_instantiation():
    names = set()
    for c in M.CASES:
        assert c["name"] not in names
        names.add(c["name"])
        assert M.eligible(c), c
        want = M.expected_variant(c)
        got = {k: c[k] for k in want}
        assert got == want, (c["name"], got, want)
        assert c["cin"] * c["k"] <= 2304 and min(M.lens_of(c)) >= 1 and max(M.lens_of(c)) == c["T"] == M.lens_of(c)[0]
    inst = {(c["epi"], c["k"], c["p1"]) for c in M.CASES}
    # every (epi, k, p1) the launcher can pick outside EPI 2; the GPU test runs each under 2, 3 and 4 stages
    assert inst == {(0, 1, 0), (0, 3, 0), (1, 1, 0), (1, 3, 0), (4, 1, 0), (0, 1, 1), (0, 3, 1), (1, 1, 1), (1, 3, 1)}, inst
    assert {c["ksplit"] for c in M.CASES} == {1, 2, 3, 4}
    # one uneven split: 25 channel blocks over 3, 17 over 2
    assert any(c["ksplit"] == 3 and (c["cin"] // 16) % 3 for c in M.CASES) and any(c["ksplit"] == 2 and (c["cin"] // 16) % 2 for c in M.CASES)
    assert {c["epi_vec"] for c in M.CASES} == {0, 1} and {c["cols"] for c in M.CASES} == {0, 1}
    # K loops shorter than, equal to and longer than every prefetch distance (1 .. 3 steps / channel blocks)
    for k in (1, 3):
        assert {c["cin"] // 16 for c in M.CASES if c["k"] == k and not c["p1"]} >= {1, 2, 3, 4}
        assert {c["cin"] // 32 for c in M.CASES if c["k"] == k and c["p1"]} >= {1, 2, 3}
    for name, kw in M.REJECTS:
        base = M.case(name, 64, 128, 1, 196, epi=0, ksplit=1, epi_vec=1)
        base.update(kw)
        assert not M.eligible(base), name


def test_split_planes_reproduce_the_operand_to_22_bits():
    rs = np.random.RandomState(7)
    a = rs.randn(4096).astype(np.float32)
    h0, h1 = M.split(a, M.SCALE_X)
    v = a.astype(np.float64) * M.SCALE_X
    assert np.all(np.abs(h0 + h1 - v) <= np.abs(v) * 2.0 ** -21 + 2.0 ** -24)
    assert np.array_equal(h0 / M.SCALE_X, M.fp16_rounded(a, M.SCALE_X))
