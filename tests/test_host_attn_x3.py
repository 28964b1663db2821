"""CPU side of tests/test_gpu_attn_x3.py (model, data and case table: tests/attn_x3_model.py).
  * The kernel's per-wave loop plan, restated in Python, has the properties the kernel relies on - for every length <= 1024, every wave
    start and every key range of a 1 .. 4-way split: the four loops are ordered, every 32-key block is visited exactly once, every block
    run by the FAR code lies wholly beyond the +-64 bias window of all 32 queries on one side and wholly inside the length, and every
    table index of a near block stays inside the +-128 extended table.  The restatement can drift from csrc/attention_x3b.hip: it proves
    the ARITHMETIC of the partition and labels the GPU cases; that the kernel computes this partition is what the GPU cases show.
  * The case table as a whole exercises every loop run and empty, every adjacency (jA = jM, jB = jM, e1 = e2), an idle wave beside
    active ones, a single-tile sample, fewer tiles than key ranges, and every seam length.
  * On the data of every case the emulated scheme stays under GATE / 10 and every mutation the case claims lands above 3 GATE, every
    mutation is claimed somewhere: so the 2e-5 gate of the GPU test separates a right kernel from each of these wrong ones.  The
    one-product mode sits between GATE and P1_GATE / 10.
  * The layout code round-trips, agrees with the library's image size, and the entry's refusals are the model's."""
import os

import numpy as np
import pytest

import attn_x3_model as M

IDS = [c["name"] for c in M.CASES]


def test_plan_properties_hold_for_every_length_wave_and_key_range():
    checked = 0
    for L in range(1, 1025):
        for S in (1, 2, 3, 4):
            for jt0, n in M.split_ranges(L, S):
                if n == 0:
                    continue
                boff, nblk = 2 * jt0, 2 * n
                for tq0 in range(0, L, M.QPW):
                    p = M.plan(tq0, L, n, boff)
                    assert 1 <= p["e1"] <= p["e2"] <= p["jM"] <= n, (L, S, jt0, tq0, p)
                    loops = p["loops"]
                    assert loops[0][0] == 1 and loops[-1][1] == n and all(loops[i][1] == loops[i + 1][0] for i in range(3)), (L, S, jt0, tq0, p)
                    seen = [0]
                    for a, b, cls in loops:
                        assert a <= b
                        for j in range(a, b):
                            for blk in (2 * j - 1, 2 * j):
                                seen.append(blk)
                                ab, side = blk + boff, M.block_side(tq0, blk + boff)
                                if cls == M.FAR:
                                    assert side != 0 and 32 * ab + 31 < L, (L, S, jt0, tq0, j, blk)
                                elif side == 0:      # near block: table index s - t + 128 of the extended table [0, 256]
                                    assert 32 * ab - (tq0 + 31) + 128 >= 0 and 32 * ab + 31 - tq0 + 128 <= 256, (L, tq0, ab)
                    seen.append(nblk - 1)
                    assert seen == list(range(nblk)), (L, S, jt0, tq0, seen)
                    checked += 1
    assert checked > 100000


def test_case_table_covers_every_loop_combination_and_seam():
    names = set()
    have = set()
    for c in M.CASES:
        assert c["name"] not in names
        names.add(c["name"])
        assert max(c["lens"]) == c["lens"][0] == c["T"] <= 768 and min(c["lens"]) >= 1 and len(c["lens"]) <= 4
        assert (32 <= c["cin"] <= 96 and 2 <= c["H"] <= 8) or (c["H"], c["cin"]) == (16, 768)
        assert M.eligible(c["cin"], c["H"], c["T"], c["lens"], p1=int(c["p1"]))
        assert set(c["claims"]) <= set(M.MUTATIONS)
        for S in c["ksplit"]:
            assert S == 1 or (len(c["lens"]) <= 2 and M.nt64(c["T"]) >= 2 * S)          # the launcher's conditions for a split
            have |= M.labels(c, S)
    want = {f"loop{i}_{w}" for i in range(4) for w in ("run", "empty")} | {"jA=jM", "jB=jM", "e1=e2", "idle_wave_beside_active", "single_tile",
                                                                            "ntiles_lt_S", "empty_range"}
    assert want <= have, want - have
    lens = {n for c in M.CASES for n in c["lens"]}
    assert lens >= {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193}, lens
    Ts = {c["T"] for c in M.CASES}
    assert any(T % 192 == 0 and T % 128 == 0 for T in Ts) and any(T % 64 == 0 and T % 128 for T in Ts) and any(T % 64 for T in Ts)
    assert {S for c in M.CASES for S in c["ksplit"]} == {1, 2, 3, 4}
    assert any(-(-c["T"] // 128) * c["H"] * len(c["lens"]) % 8 for c in M.CASES)             # a grid that is no multiple of 8
    assert any(M.nt64(c["T"]) % S for c in M.CASES for S in c["ksplit"] if S > 1)             # an uneven split
    offs = {o for c in M.CASES if c["offsets"] for o in c["offsets"]}
    assert offs >= {-64, -63, -33, -32, -1, 0, 1, 31, 32, 63, 64}
    assert any(c["H"] == 16 and 144 * c["H"] // 128 > 6 and (144 * c["H"] // 128) % 6 == 0 for c in M.CASES)      # EPI 2's tile-order remap
    claimed = {m for c in M.CASES for m in c["claims"]}
    assert claimed == set(M.MUTATIONS), set(M.MUTATIONS) - claimed
    assert {c["kind"] for c in M.CASES} == {"bias_ptr", "score_ptr", "prec", "prec_table", "ramp"}
    assert {c["std"] for c in M.CASES if c["kind"].startswith("prec")} >= {0.6, 2.0, 5.0}


@pytest.mark.parametrize("c", M.CASES, ids=IDS)
def test_scheme_is_a_tenth_of_the_gate_and_every_claimed_mutation_three_gates(c):
    d = M.make_data(c)
    n = len(c["lens"])
    refs = [M.reference(d, bi) for bi in range(n)]
    scheme = max(M.rel_err(M.emulate(d, bi), refs[bi]) for bi in range(n))
    print(f"attn_x3_cpu_{c['name']}_scheme\t{scheme:.3e}")
    assert scheme <= M.GATE / 10, (c["name"], scheme)
    if c["fp32_form"]:
        e = max(M.rel_err(M.emulate(d, bi, fp32_form=True), refs[bi]) for bi in range(n))
        assert e <= M.GATE / 10, (c["name"], e)
    if c["kind"] == "score_ptr":
        for bi in range(n):
            assert M.score_margin(d, bi) >= 10.0, (c["name"], bi, M.score_margin(d, bi))
    if c["kind"] == "ramp":
        # the rescale runs at many blocks: some query raises its maximum by more than 2^3 in at least a quarter of the blocks after the first
        q, k, _ = M.qkv64(d["w"], d["b"], d["x"][0])
        s = (np.einsum("hct,hcs->hts", q, k) / np.sqrt(48.0) + np.asarray(d["tab"], np.float64)[:, M.bias_index(c["T"])]) * M.LOG2E
        run, hits = np.full(s.shape[:2], -np.inf), 0
        nb = c["T"] // 32
        for blk in range(nb):
            mx = s[:, :, 32 * blk: 32 * blk + 32].max(-1)
            up = mx > run + 3.0
            hits += int(blk > 0 and up.any())
            run = np.where(up, mx, run)
        assert hits >= nb // 4, (hits, nb)
    for mut in c["claims"]:
        with np.errstate(all="ignore"):
            e = 0.0
            for bi in range(n):                      # (the longest sample first; the first sample that shows it is enough)
                e = max(e, M.rel_err(M.emulate(d, bi, mut=mut), refs[bi]))
                if e >= 3 * M.GATE:
                    break
        print(f"attn_x3_cpu_{c['name']}_{mut}\t{e:.3e}")
        assert e >= 3 * M.GATE, (c["name"], mut, e)
    if c["p1"]:
        e1 = max(M.rel_err(M.emulate(d, bi, p1=True), refs[bi]) for bi in range(n))
        print(f"attn_x3_cpu_{c['name']}_p1\t{e1:.3e}")
        assert M.GATE < e1 <= M.P1_GATE / 10 and e1 > scheme, (c["name"], e1)


def test_image_layout_round_trips_and_matches_the_layout_comment():
    B, H, T = 2, 3, 130
    rs = np.random.RandomState(1)
    raw = rs.randint(0, 65536, M.image_bytes(B, H, T) // 2).astype(np.uint16).tobytes()
    q, k, v = M.decode_image(raw, B, H, T)
    assert q.shape == (B, H, 2, 48, 192) and k.shape == v.shape == (B, H, 2, 48, 192)
    assert M.encode_image(q, k, v, T) == raw
    a = np.frombuffer(raw, np.uint16).reshape(B, H, -1)
    Tq = M.tq(T)
    # Q chunk (plane 1, c8 2, query 70) = channels 16 .. 23 of that query
    assert np.array_equal(a[1, 2, ((1 * 6 + 2) * Tq + 70) * 8:][:8], q[1, 2, 1, 16:24, 70])
    tile1 = a[1, 2, 2 * 6 * Tq * 8 + M.TILE_BYTES // 2:]
    # tile 1: K chunk (plane 0, c8 5, key 3) = channels 40 .. 47 of key 67
    assert np.array_equal(tile1[(5 * 64 + 3) * 8:][:8], k[1, 2, 0, 40:48, 67])
    # tile 1: V chunk (plane 1, u 1, j 0, hh 1, channel 7) = keys 64 + 32 + 4 + {0..3, 8..11} of channel 7
    off = 2 * 6 * 64 * 8 + (1 * 8 * 48 + ((1 * 2 + 0) * 2 + 1) * 48 + 7) * 8
    assert np.array_equal(tile1[off: off + 8], v[1, 2, 1, 7, [100, 101, 102, 103, 108, 109, 110, 111]])
    # every key of a tile is held exactly once
    assert sorted(M.V_KEYS.reshape(-1).tolist()) == list(range(64))


def test_image_size_is_the_library_s():
    from detail_tts_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    for B, H, T in ((1, 1, 1), (2, 3, 64), (4, 16, 65), (3, 8, 768)):
        assert lib.dtts_attn_x3_image_bytes(B, H, T) == M.image_bytes(B, H, T)
    assert lib.dtts_attn_x3_image_bytes(0, 1, 1) == 0


def test_output_planes_decode():
    B, H, T = 1, 2, 5
    Tp = M.x3_tp(T)
    a = np.zeros((B, 6 * H, 2, Tp, 8), np.float16)
    a[0, 7, 0, 3 + 1, 2] = 24.0                          # channel 7 * 8 + 2 = 58, column t = 3: plane 0
    a[0, 7, 1, 3 + 1, 2] = 0.5                           # plane 1
    y, _ = M.decode_out_planes(a.tobytes(), B, H, T)
    assert y.shape == (1, 96, 5) and y[0, 58, 3] == 24.5 / 16 and np.count_nonzero(y) == 1


def test_rejects_are_what_the_model_refuses():
    for name, kw, _ in M.REJECTS:
        base = dict(cin=32, H=2, T=100, lens=[100, 50], p1=0)
        base.update(kw)
        assert not M.eligible(**base), name
    assert M.eligible(cin=32, H=2, T=100, lens=[100, 50])
