"""The DEVICE token sampler (csrc/gpt_kernels.hip: sampler_kernel) on the edge cases of tests/golden/token_sampler_edges.npz - the
reference's HF processors on ties, 64 / 65 candidates, top_k in {1, V-1, V, V+5}, top_p in {1, 1e-6}, a dominant token, flat rows,
penalised negative / arg-max logits, -inf logits, the typical warper, V from 2 to 9217.  For each row the oracle CDF is built in
float64 from the HF-pinned filtered values; the kernel is driven with uniforms swept through it (tests/test_host_token_sampler.py:
make_probes, whose exclusions are capped on the CPU) and must return the oracle's inverse-CDF token EXACTLY.  Through the C ABI."""
import numpy as np
import pytest

import test_host_token_sampler as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS = 16          # GEMV_MAXB: rows of one sampler launch


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def rt(weights):
    from detail_tts_amd.runtime import Runtime
    return Runtime(weights, folded=True, parts=("gpt",))


@pytest.fixture(scope="module")
def edges(golden):
    return golden("token_sampler_edges")


def kwargs_of(params, **extra):
    kw = dict(top_k=int(params["top_k"]), top_p=float(params["top_p"]), temperature=float(params["temp"]),
              repetition_penalty=float(params["rp"]), typical_mass=float(params["mass"]) or None)
    kw.update(extra)
    return kw


def draw(rt, logits_row, hist_row, us, **kw):
    """the device's token for every uniform of `us` on ONE logits row: 16 rows per launch (the row repeated, 16 uniforms)"""
    logits = dev(np.repeat(np.asarray(logits_row, np.float32)[None], ROWS, 0))
    hist = np.repeat(np.asarray(hist_row)[None], ROWS, 0)
    got = []
    for i in range(0, len(us), ROWS):
        chunk = us[i:i + ROWS]
        got.extend(rt.op_sample_logits(logits, hist, dev(np.resize(chunk, ROWS)), **kw).tolist()[:len(chunk)])
    return np.array(got)


def check_row(rt, tag, logits_row, hist_row, filtered, seed, **kw):
    """drawn == the oracle's inverse CDF at every probe; nothing removed is drawn; every wide kept token is drawn; u = 0 -> the first
    kept token, u = nextafter(1, 0) and u = 1 -> the last"""
    pr = H.make_probes(filtered, seed)
    assert pr["n_swept"] >= H.MIN_PROBES and pr["excluded_mass"] <= H.MAX_EXCLUDED_MASS, (tag, pr["n_swept"], pr["excluded_mass"])
    got = draw(rt, logits_row, hist_row, pr["u"], **kw)
    want = pr["want"]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (tag, bad.size, bad[:5], pr["u"][bad[:5]], got[bad[:5]], want[bad[:5]])
    kept = set(np.nonzero(np.isfinite(filtered))[0].tolist())
    assert set(got.tolist()) <= kept, tag
    assert set(pr["wide"].tolist()) <= set(got[:pr["n_swept"]].tolist()), tag
    assert got[-3:].tolist() == [pr["first"], pr["last"], pr["last"]], (tag, got[-3:], pr["first"], pr["last"])
    return pr


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_device_sampler_on_the_edge_cases(rt, edges, name):
    """Every case of the fixture, every row.  In the tie-straddle rows (x_all_equal, and the rows of case a whose cut falls inside a
    tie group) the members the device keeps are the oracle's: ascending (value, id) order, HF's count."""
    logits, hist = H.case_inputs(name)
    assert H.input_hash(logits, hist) == str(edges[name + ".sha1"])
    kw = kwargs_of(H.CASES[name]["params"])
    for r in range(H.CASES[name]["R"]):
        f = H.pinned_filtered(edges, name, r, logits, hist)
        check_row(rt, (name, r), logits[r], hist[r], f, 1000 + r, **kw)


def sixteen_rows():
    """rows of 16 different V = 8194 cases, one each -> (names, logits [16, V], history [16, 8])"""
    names = [n for n in sorted(H.CASES) if H.CASES[n]["V"] == H.V0 and H.CASES[n]["transform"] != "equal"][:ROWS]
    assert len(names) == ROWS
    ins = [H.case_inputs(n) for n in names]
    logits = np.stack([x[0][i % x[0].shape[0]] for i, x in enumerate(ins)])
    hist = np.stack([x[1][i % x[1].shape[0]] for i, x in enumerate(ins)])
    assert len({logits[i].tobytes() for i in range(ROWS)}) == ROWS
    return names, logits, hist


SIXTEEN_PARAMS = (H.DEFAULTS, dict(H.DEFAULTS, top_k=0, top_p=1.0, rp=1.3), dict(H.DEFAULTS, mass=0.9, temp=1.0))
SIXTEEN_DRAWS = 8


def test_sixteen_different_rows_in_one_launch(rt, edges):
    """Rows of 16 different cases (V = 8194) in ONE launch: every row gives the token of its own single-row launch, and the oracle's,
    at the default parameters, with top-k and top-p off, and under the typical warper.  These rows meet parameters their cases were not
    made for, so a row is compared with the oracle only where its cuts keep the margins of test_host_token_sampler.py (CUT_MARGIN,
    KEY_MARGIN), and a draw only where the probe margins hold; the row-alone equality is asserted for every draw.  At least half of
    the 128 draws of every parameter set must have been compared with the oracle (a uniform lands within 1e-5 of an edge, or in an
    interval narrower than 2e-5, far less often than that on any of these rows: the mass of the narrow tokens is capped at 1 %
    for the cases proper, and the margin strips of the at most ~100 wide tokens of a nucleus cover 2e-3 of the unit interval)."""
    from oracle import gpt as G
    names, logits, hist = sixteen_rows()
    rs = np.random.RandomState(77)
    for params in SIXTEEN_PARAMS:
        kw = kwargs_of(params)
        cdfs, sound = [], []
        for i in range(ROWS):
            with np.errstate(all="ignore"):
                f = G.process_logits(logits[i], hist[i], repetition_penalty=params["rp"], temperature=params["temp"],
                                     top_k=params["top_k"] or None, top_p=params["top_p"], typical_mass=params["mass"] or None)
            cdfs.append(H.oracle_cdf(f))
            sound.append(H.row_cut_margin(logits[i], hist[i], params) > H.CUT_MARGIN
                         and H.row_typical_key_gap(logits[i], hist[i], params) > H.KEY_MARGIN)
        compared = 0
        for _ in range(SIXTEEN_DRAWS):
            u = rs.rand(ROWS).astype(np.float32)
            packed = rt.op_sample_logits(dev(logits), hist, dev(u), **kw)
            for i in range(ROWS):
                alone = rt.op_sample_logits(dev(logits[i:i + 1]), hist[i:i + 1], dev(u[i:i + 1]), **kw)
                assert packed[i] == alone[0], (params, names[i], packed[i], alone[0])
                c, lo, _ = cdfs[i]
                v = int(H.inverse_cdf(c, np.float64(u[i])))
                if sound[i] and (c - lo)[v] >= H.MIN_WIDTH and min(u[i] - lo[v], c[v] - u[i]) >= H.EDGE_MARGIN:
                    assert packed[i] == v, (params, names[i], packed[i], v)
                    compared += 1
        print(f"sixteen rows, {params}: {compared} of {SIXTEEN_DRAWS * ROWS} draws compared with the oracle, {sum(sound)} rows sound")
        assert compared >= SIXTEEN_DRAWS * ROWS // 2, (params, compared, sound)


def test_suppress_eos_never_draws_the_last_id(rt):
    """suppress_eos through the unit entry: id V - 1 carries most of the mass of the row, and is never drawn - the draws are the
    oracle's on the row with -inf written there (what generate() does, gpt/model.py's inference with suppress)."""
    from oracle import gpt as G
    rs = np.random.RandomState(310)
    V = H.V0
    for r in range(2):
        x = (rs.randn(V) * 2.0).astype(np.float32)
        x[V - 1] = x.max() + np.float32(10.0)
        hist = rs.randint(0, V - 1, size=8)
        c, lo, _ = H.oracle_cdf(G.process_logits(x, hist))
        assert (c - lo)[V - 1] > 0.9
        got = draw(rt, x, hist, np.array([0.0, 0.3, 0.6, 0.95, 1.0], np.float32))
        assert set(got.tolist()) == {V - 1}                               # without the option the planted id takes everything
        xs = x.copy()
        xs[V - 1] = -np.inf
        f = G.process_logits(xs, hist)
        pr = check_row(rt, ("suppress_eos", r), x, hist, f, 2000 + r, suppress_eos=True)
        assert V - 1 not in pr["want"]


def test_vocabulary_guard_refuses_before_a_launch(rt):
    """The largest V follows from the sampler's LDS budget (static + dynamic); a larger one is refused by the host, nothing is
    launched.  The largest admitted V runs once, at the default parameters, against the oracle."""
    from detail_tts_amd import _lib
    from detail_tts_amd.runtime import DttsError
    from oracle import gpt as G
    vmax = int(_lib.load().dtts_sampler_max_vocab())
    assert 8194 <= vmax < 16384
    for V in (vmax + 1, 16384, 65000):
        with pytest.raises(DttsError):
            rt.op_sample_logits(torch.zeros((1, V), device="cuda"), np.zeros((1, 1), np.int32), dev(np.array([0.5])))
    rs = np.random.RandomState(320)
    x = (rs.randn(vmax) * 2.0).astype(np.float32)
    hist = np.concatenate([rs.randint(0, vmax, size=6), [0, vmax - 1]])
    check_row(rt, "vmax", x, hist, G.process_logits(x, hist), 3000)


@pytest.mark.parametrize("opts", [dict(top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0),
                                  dict(top_k=5, top_p=0.3, temperature=0.5, repetition_penalty=1.5)])
def test_generate_public_options_vs_oracle(rt, weights, opts):
    """dtts_gpt_options' top_k / top_p / temperature / repetition_penalty at non-default values, end to end: B = 2 ragged, 8 tokens."""
    from oracle import gpt as G
    rs = np.random.RandomState(23)
    refer = (rs.randn(2, 128, 50) * 2 - 5).astype(np.float32)
    rl = [50, 36]
    texts = [np.concatenate([rs.randint(3, 255, 8), [0]]), np.concatenate([rs.randint(3, 255, 5), [0]])]
    codes, ncodes, _ = rt.gpt_generate(dev(refer), rl, texts, 6, [41, 42], max_generate_length=8, **opts)
    for b in range(2):
        ref = G.generate(weights, refer[b:b + 1, :, :rl[b]], [rl[b]], texts[b][None], 6, [41 + b], max_generate_length=8,
                         top_k=opts["top_k"] or None, top_p=opts["top_p"], temperature=opts["temperature"],
                         repetition_penalty=opts["repetition_penalty"])
        assert np.array_equal(codes[b, :ref.shape[1]], ref[0]), (opts, b, codes[b], ref)
