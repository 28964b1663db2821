"""Per-row sampling settings and infer_many, the host side (no GPU): resolve_sampling, the dtts_gpt_options / dtts_gpt_row_options
layouts, the row-cap crop of split_session, Voice.cat, infer_many's bookkeeping on a fake model, and the margin bookkeeping of the
sixteen-row GPU case (tests/row_sampling_cases.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 24


def resolve(s, B=3, **kw):
    from detail_tts_amd.gpt.sampling import resolve_sampling
    return resolve_sampling(s, B, **dict(dict(top_k=50, max_generate_length=G, decode_options=None), **kw))


# ------------------------------------------------------------------------------------------------ resolve_sampling
def test_nothing_asked_for_is_the_uniform_session():
    assert resolve(None) is None and resolve({}) is None and resolve([None, None, None]) is None and resolve([{}, None, {}]) is None
    # ... also when the rows spell out what the call decodes under anyway
    assert resolve(dict(temperature=0.8, top_p=0.8, repetition_penalty=2.0, top_k=50, max_generate_length=G)) is None
    assert resolve([dict(no_repeat_ngram_size=3)] * 3, decode_options=dict(no_repeat_ngram_size=3)) is None


def test_a_dict_is_b_copies_and_defaults_fill_from_the_call():
    rows = resolve(dict(temperature=0.6))
    assert rows == resolve([dict(temperature=0.6)] * 3) and len(rows) == 3
    assert rows[0] == dict(top_k=50, top_p=0.8, temperature=0.6, repetition_penalty=2.0, typical_mass=0.0, max_generate_length=G, processors={})
    rows = resolve([None, dict(top_p=0.95, min_new_tokens=6), dict(max_generate_length=9)], top_k=7, decode_options=dict(no_repeat_ngram_size=2))
    assert [r["top_k"] for r in rows] == [7, 7, 7] and [r["max_generate_length"] for r in rows] == [G, G, 9]
    assert rows[0]["processors"] == dict(no_repeat_ngram_size=2) and rows[1]["processors"] == dict(no_repeat_ngram_size=2, min_new_tokens=6)
    assert rows[1]["top_p"] == 0.95 and rows[0]["top_p"] == 0.8
    # a row's own processor key wins over the call's; None means "not given"
    assert resolve([dict(no_repeat_ngram_size=3, temperature=None), None, None], decode_options=dict(no_repeat_ngram_size=2))[0]["processors"] == \
        dict(no_repeat_ngram_size=3)
    from detail_tts_amd.gpt.sampling import repeat_rows, session_cap
    assert session_cap(rows, G) == G and session_cap(None, G) == G and session_cap(resolve(dict(max_generate_length=9)), G) == 9
    assert [r["max_generate_length"] for r in repeat_rows(rows, 2)] == [G, G, G, G, 9, 9] and repeat_rows(None, 2) is None


def test_do_sample_false_is_greedy():
    r = resolve([dict(do_sample=False, temperature=1.3, top_p=0.5, min_p=0.2, min_length=5), None, None])[0]
    assert (r["top_k"], r["temperature"], r["top_p"], r["typical_mass"]) == (1, 1.0, 1.0, 0.0)
    assert r["processors"] == dict(min_length=5)            # the warpers are checked, then dropped, as HF builds none without sampling
    assert r["repetition_penalty"] == 2.0


@pytest.mark.parametrize("bad, names", [
    ([None, dict(temperature=0.0), None], ("sampling[1]", "temperature")),
    ([None, None, dict(temperature=float("inf"))], ("sampling[2]", "temperature")),
    ([dict(top_p=0.0), None, None], ("sampling[0]", "top_p")),
    ([dict(top_p=1.5), None, None], ("sampling[0]", "top_p")),
    ([None, dict(top_k=-1), None], ("sampling[1]", "top_k")),
    ([None, dict(top_k=2.5), None], ("sampling[1]", "top_k")),
    ([None, dict(repetition_penalty=0), None], ("sampling[1]", "repetition_penalty")),
    ([None, dict(typical_mass=1.2), None], ("sampling[1]", "typical_mass")),
    ([None, dict(max_generate_length=0), None], ("sampling[1]", "max_generate_length")),
    ([None, dict(max_generate_length=G + 1), None], ("sampling[1]", "max_generate_length")),       # a cap above the call's
    ([None, dict(do_sample=1), None], ("sampling[1]", "do_sample")),
    ([None, dict(loudness=2), None], ("sampling[1]", "loudness")),                                 # an unknown key
    ([None, dict(num_beams=2), None], ("sampling[1]", "num_beams")),                               # a beam key
    ([None, dict(length_penalty=1.0), None], ("sampling[1]", "length_penalty")),
    ([None, None, dict(no_repeat_ngram_size=17)], ("sampling[2]", "no_repeat_ngram_size")),
    ([None, None, dict(min_p=2.0)], ("sampling[2]", "min_p")),
    ([None, None, dict(suppress_tokens=[9000])], ("sampling[2]", "suppress_tokens")),
    (dict(temperature=-1), ("sampling", "temperature")),
    ([None, None], ("2 rows", "3")),                                                               # a wrong row count
    ("hot", ("sampling",)),
    ([None, 0.5, None], ("sampling[1]",)),
])
def test_refusals_name_the_row_and_the_key(bad, names):
    with pytest.raises(ValueError) as e:
        resolve(bad)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_sampling_with_beams_is_refused():
    with pytest.raises(ValueError, match="num_beams"):
        resolve(dict(temperature=0.6), num_beams=4)
    assert resolve(None, num_beams=4) is None
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    text, tl = torch.zeros((1, 3), dtype=torch.int64), [3]
    refer, rl = torch.zeros((1, 128, 8)), [8]
    for entry in (SynthesizerTrn.infer, SynthesizerTrn.infer_gpt):      # `self` is a bare object: anything later would trip over it
        with pytest.raises(ValueError, match="num_beams"):
            entry(object(), text, tl, refer, rl, sampling=dict(temperature=0.6), decode_options=dict(num_beams=2), seed=1)
        with pytest.raises(ValueError, match=r"sampling\[0\].*top_p"):
            entry(object(), text, tl, refer, rl, sampling=[dict(top_p=3.0)], batch=True, seed=1)
    with pytest.raises(ValueError, match="infer_long"):
        SynthesizerTrn.infer_long(object(), "x", sampling=[dict(temperature=0.6)])
    with pytest.raises(ValueError, match="stream-wide"):
        next(SynthesizerTrn.infer_stream(object(), [], sampling=[dict(temperature=0.6)]))


# ------------------------------------------------------------------------------------------------ the C layouts
def _declarators(hdr, name):
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*(?:,|;)", body)


def test_ctypes_layouts_are_the_headers():
    """The mirror of dtts_gpt_options has the size the library was built with (dtts_gpt_options_init is host-only; the library refuses
    any other struct_size), both structs list the header's declarators in the header's order, and row_options starts NULL."""
    from detail_tts_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "detail_hip.h")).read()
    assert _declarators(hdr, "dtts_gpt_options") == [n for n, _ in _lib.DttsGptOptions._fields_]
    assert _declarators(hdr, "dtts_gpt_row_options") == [n for n, _ in _lib.DttsGptRowOptions._fields_]
    lib = _lib.load()
    o = _lib.DttsGptOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    lib.dtts_gpt_options_init(C.byref(o))
    assert o.struct_size == C.sizeof(_lib.DttsGptOptions)
    assert not o.row_options
    assert _lib.DttsGptOptions.row_seeds.offset < _lib.DttsGptOptions.row_options.offset < _lib.DttsGptOptions.typical_mass.offset
    assert hasattr(lib, "dtts_op_sample_logits_rows")
    # 6 floats + 6 ints, the double on an 8-byte boundary, then (pointer, int) twice
    assert C.sizeof(_lib.DttsGptRowOptions) == 48 + 8 + 2 * 16 and _lib.DttsGptRowOptions.exp_decay_factor.offset == 48


def test_runtime_fills_the_row_records():
    from detail_tts_amd import _lib
    from detail_tts_amd.runtime import Runtime
    o = _lib.DttsGptOptions()
    rows = resolve([dict(do_sample=False), dict(temperature=1.3, top_p=0.95, top_k=0, suppress_tokens=[5, 2]),
                    dict(max_generate_length=9, exponential_decay_length_penalty=(3, 1.5))])
    keep = Runtime._row_options(o, rows, 3, G)
    q = [o.row_options[b] for b in range(3)]
    assert (q[0].top_k, q[0].temperature, q[0].top_p, q[0].max_generate_length) == (1, 1.0, 1.0, G)
    assert q[1].top_k == 0 and abs(q[1].temperature - 1.3) < 1e-6 and [q[1].suppress_tokens[i] for i in range(q[1].n_suppress_tokens)] == [2, 5]
    assert (q[2].max_generate_length, q[2].exp_decay_start, q[2].exp_decay_factor) == (9, 3, 1.5) and keep
    assert Runtime._row_options(_lib.DttsGptOptions(), None, 3, G) is None
    with pytest.raises(ValueError, match="2 records"):
        Runtime._row_options(_lib.DttsGptOptions(), rows[:2], 3, G)
    with pytest.raises(ValueError, match="largest cap"):
        Runtime._row_options(_lib.DttsGptOptions(), [dict(r, max_generate_length=9) for r in rows], 3, G)
    with pytest.raises(ValueError, match=r"rows\[1\].*loud"):
        Runtime._row_options(_lib.DttsGptOptions(), [rows[0], dict(loud=1), rows[2]], 3, G)


# ------------------------------------------------------------------------------------------------ pipeline bookkeeping
def test_split_session_crops_at_the_rows_own_cap():
    from detail_tts_amd.pipeline import Request, merge_rows, split_session
    ncodes = [24, 9, 12, 5]
    assert split_session(ncodes, [2, 2]) == [[23, 8], [11, 4]]
    assert split_session(ncodes, [2, 2], [24, 9, 10, 24]) == [[23, 8], [9, 4]]            # row 2 counts nothing behind its cap of 10
    assert split_session(ncodes, [4], None) == [[23, 8, 11, 4]]
    with pytest.raises(ValueError):
        split_session([3, 1], [2], [24, 24])
    # two requests in one session: each keeps its own rows' settings, a request without any gets the call's written out
    call = dict(top_k=50, max_generate_length=G, decode_options=None)
    a = Request(B=2, rl=[0, 0], seed=1, sids=[0, 1], texts=[], refer=None)
    b = Request(B=1, rl=[0], seed=2, sids=[0], texts=[], refer=None, rows=resolve(dict(temperature=1.3), B=1))
    assert merge_rows([a], call) is None
    rows = merge_rows([a, b], call)
    assert [r["temperature"] for r in rows] == [0.8, 0.8, 1.3] and rows[0] == resolve(None, B=1, always_rows=True)[0]


def voice(S, base=0.0, vq=True):
    from detail_tts_amd.voice import Voice
    g = torch.arange(S * 4, dtype=torch.float32).reshape(S, 4) + base
    return Voice(g, torch.arange(S * 6, dtype=torch.float32).reshape(S, 6) - base, g * 2 if vq else None)


def test_voice_cat_is_the_inverse_of_rows():
    from detail_tts_amd.voice import Voice
    v = voice(5, 0.25)
    back = Voice.cat([v.rows(i) for i in range(5)])
    for k, t in v.members():
        assert torch.equal(getattr(back, k), t) and getattr(back, k).is_contiguous()
    mixed = Voice.cat([v.rows([3, 1]), voice(1, 7.0), v.rows(0)])
    assert mixed.S == 4 and torch.equal(mixed.gpt[:2], v.gpt[[3, 1]]) and torch.equal(mixed.diffusion[3], v.diffusion[0])
    assert Voice.cat([v]) is v
    for bad in ([], [v, voice(1, vq=False)], [v, "x"]):
        with pytest.raises(ValueError):
            Voice.cat(bad)


# ------------------------------------------------------------------------------------------------ infer_many on a fake model
class FakeModel:
    """infer_stream as the host sees it: reads its requests as lazily as pipeline.group_requests does (two ahead), records them, and
    yields wav[b] = sample id + 1 over 1024 (b + 1) samples"""

    def __init__(self):
        self.requests, self.voices, self.kw, self.read_at_yield = [], 0, None, []

    def get_conditioning_latents(self, refer, refer_lengths=None):
        self.voices += 1
        assert tuple(refer.shape[:2]) == (1, 128)
        return voice(1, float(self.voices))

    def infer_stream(self, requests, **kw):
        from detail_tts_amd.pipeline import group_requests
        self.kw = kw
        for (r,) in group_requests(requests):
            self.requests.append(r)
            B = r["text"].shape[0]
            lens = [1024 * (b + 1) for b in range(B)]
            wav = torch.zeros(B, 1, max(lens))
            for b, sid in enumerate(r["sample_ids"]):
                wav[b, 0] = sid + 1
            yield wav, lens


def utterances(n, refer=None):
    refer = torch.zeros(128, 9) if refer is None else refer
    out = []
    for i in range(n):
        u = dict(text=np.arange(3 + i % 3) + 5, speaker=voice(1, float(i))) if i % 2 else dict(text=np.arange(3 + i % 3) + 5, refer=refer)
        out.append(u)
    return out


def test_infer_many_groups_orders_and_cuts():
    from detail_tts_amd.many import infer_many
    m = FakeModel()
    us = utterances(7)
    us[2]["sampling"] = dict(temperature=1.3)
    us[3]["sample_id"] = 40
    us[4]["speed"] = 0.8
    got = list(infer_many(m, us, rows_per_call=3, seed=11, sampling=dict(top_p=0.9), max_generate_length=G))
    assert [r["text"].shape[0] for r in m.requests] == [3, 3, 1]                            # the last request is short
    assert [r["sample_ids"] for r in m.requests] == [[0, 1, 2], [40, 4, 5], [6]]            # default: the utterance's index
    assert {r["seed"] for r in m.requests} == {11}                                          # the ONE seed
    assert [(float(w[0, 0, 0]), n, tuple(w.shape)) for w, n in got] == \
        [(sid + 1.0, 1024 * (b + 1), (1, 1, 1024 * (b + 1))) for r in m.requests for b, sid in enumerate(r["sample_ids"])]      # input order, cut
    assert m.requests[0]["sampling"] == [dict(top_p=0.9), dict(top_p=0.9), dict(temperature=1.3)]      # the call's default, or the row's own
    assert m.requests[1]["speed"] == [1.0, 0.8, 1.0] and "speed" not in m.requests[0]
    assert m.voices == 1                                                                    # one prompt tensor object: ONE voice
    assert m.requests[0]["speaker"].S == 3 and torch.equal(m.requests[0]["speaker"].gpt[1], us[1]["speaker"].gpt[0])
    assert m.requests[0]["text_length"] == [3, 4, 5] and m.requests[0]["text"].shape == (3, 5)
    assert m.kw["max_generate_length"] == G and "sampling" not in m.kw
    # no seed given: drawn once
    m2 = FakeModel()
    list(infer_many(m2, utterances(5), rows_per_call=2))
    assert len({r["seed"] for r in m2.requests}) == 1 and "sampling" not in m2.requests[0]
    assert list(infer_many(FakeModel(), [])) == []


def test_infer_many_reads_lazily():
    """at most two requests are read ahead of the one being handed out"""
    from detail_tts_amd.many import infer_many
    m, taken = FakeModel(), []

    def feed():
        for i, u in enumerate(utterances(12)):
            taken.append(i)
            yield u
    gen = infer_many(m, feed(), rows_per_call=2, seed=1)
    assert taken == []                                       # nothing is read before the first result is asked for
    next(gen)
    assert len(taken) <= 3 * 2                               # the request handed out and two more
    for _ in range(3):
        next(gen)
    assert len(taken) <= 4 * 2
    assert len(list(gen)) == 8 and len(taken) == 12


def test_infer_many_refusals():
    from detail_tts_amd.many import infer_many
    ok = utterances(4)
    for kw, pat in ((dict(rows_per_call=0), "rows_per_call"), (dict(rows_per_call=17), "rows_per_call"), (dict(rows_per_call=2.0), "rows_per_call"),
                    (dict(sampling=[dict()]), "sampling"), (dict(sampling=dict(temperature=0)), "temperature"),
                    (dict(decode_options=dict(num_beams=2)), "num_beams"), (dict(decode_options=dict(min_p=3)), "min_p")):
        with pytest.raises(ValueError, match=pat):           # call-level: before anything starts (no iteration needed)
            infer_many(FakeModel(), ok, **kw)
    v = voice(1)
    bad = [(dict(text=[1, 2]), "speaker"), (dict(text=[1, 2], speaker=v, refer=torch.zeros(128, 4)), "speaker"),
           (dict(text=[[1, 2]], speaker=v), "text"), (dict(text=[], speaker=v), "text"), (dict(speaker=v), "text"),
           (dict(text=[1], speaker=voice(2)), "S = 1"), (dict(text=[1], refer=torch.zeros(2, 128, 4)), "refer"),
           (dict(text=[1], refer=torch.zeros(128, 4), refer_length=5), "refer_length"), (dict(text=[1], speaker=v, sample_id=-1), "sample_id"),
           (dict(text=[1], speaker=v, sampling=[dict()]), "sampling"), (dict(text=[1], speaker=v, sampling=dict(top_p=2)), "top_p"),
           (dict(text=[1], speaker=v, loud=1), "loud"), (dict(text=[1], speaker=v, forced_codes=[[1]]), "forced_codes"),
           (dict(text=[1], speaker=v, sample_id=0), "sample id")]
    for u, pat in bad:
        m = FakeModel()
        gen = infer_many(m, [dict(text=[1], speaker=v), u], rows_per_call=2, seed=1)
        with pytest.raises(ValueError, match=pat) as e:
            next(gen)
        assert "utterances[" in str(e.value) and m.requests == [] and m.voices == 0      # checked before the group starts
    # a bad utterance of the SECOND group: the first group is served
    m = FakeModel()
    gen = infer_many(m, [dict(text=[1], speaker=v), dict(text=[1], speaker=v, sampling=dict(top_k=-2))], rows_per_call=1, seed=1)
    with pytest.raises(ValueError, match=r"utterances\[1\.\.1\].*top_k"):
        list(gen)
    with pytest.raises(ValueError, match="forced_codes"):
        next(infer_many(FakeModel(), [dict(text=[1], speaker=v, forced_codes=[3]), dict(text=[1], speaker=v)], rows_per_call=2, seed=1))


# ------------------------------------------------------------------------------------------------ the sixteen-row case's margins
def test_sixteen_row_case_margin_bookkeeping():
    """The condition of tests/test_gpu_row_sampling.py's first case, established without a GPU: of the 128 (row, draw) pairs at least
    half - exactly row_sampling_cases.COMPARED - sit where the NumPy restatement may be compared (CUT_MARGIN, MIN_WIDTH, EDGE_MARGIN),
    every row has settings of its own, and the settings cover the values the case names."""
    import row_sampling_cases as R
    x, rows, sets, u = R.build()
    want, ok = R.restatement()
    assert int(ok.sum()) == R.COMPARED >= R.ROWS * R.DRAWS // 2, (int(ok.sum()), ok.sum(0))
    assert x.shape == (16, 8194) and u.shape == (8, 16) and want.shape == ok.shape == (8, 16)
    assert len({repr(s) for s in sets}) == 16
    params = [p for p, _ in sets]
    assert {p["top_k"] for p in params} == {0, 1, 5, 50} and {p["top_p"] for p in params} == {1.0, 0.95, 0.8, 0.3}
    assert {p["temp"] for p in params} == {0.5, 0.8, 1.0, 1.7} and {p["rp"] for p in params} == {1.0, 1.3, 2.0}
    assert sum(1 for p in params if p["mass"]) == 4
    opts = [o for _, o in sets]
    assert {o.get("no_repeat_ngram_size", 0) for o in opts} == {0, 2, 3, 16}
    assert len({o["exponential_decay_length_penalty"] for o in opts if "exponential_decay_length_penalty" in o}) == 4
    assert sum("min_p" in o for o in opts) == 3 and sum("epsilon_cutoff" in o for o in opts) == 2
    masks = [("suppress_tokens" in o or "begin_suppress_tokens" in o) for o in opts]
    assert not masks[5] and len(opts[6]["suppress_tokens"]) == 8194 - 3                  # an empty mask beside a full-width one
    lens = [len(r["hist"]) for r in rows]
    assert min(lens) == 6 and max(lens) > 1500
    # the resolver accepts every row as it stands (the GPU test hands these dicts to the runtime)
    recs = resolve([dict(R.row_dict(p, o)["processors"], top_k=p["top_k"], top_p=p["top_p"], temperature=p["temp"], repetition_penalty=p["rp"],
                         typical_mass=p["mass"]) for p, o in sets], B=16)
    assert len(recs) == 16


def test_a_row_cap_below_its_forced_codes_is_refused():
    from detail_tts_amd.gpt.sampling import check_forced_caps
    rows = resolve([None, dict(max_generate_length=4), None])
    check_forced_caps(rows, [[1] * 24, [1] * 4, []])
    check_forced_caps(None, [[1] * 99]), check_forced_caps(rows, None)
    with pytest.raises(ValueError, match=r"sampling\[1\].*forced_codes"):
        check_forced_caps(rows, [[1], [1] * 5, [1]])
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    text, tl, refer, rl = torch.zeros((1, 3), dtype=torch.int64), [3], torch.zeros((1, 128, 8)), [8]
    for entry in (SynthesizerTrn.infer, SynthesizerTrn.infer_gpt):      # before the model is touched
        with pytest.raises(ValueError, match="forced_codes"):
            entry(object(), text, tl, refer, rl, sampling=dict(max_generate_length=2), forced_codes=[np.arange(5)], seed=1)


def test_infer_many_without_a_device_carries_no_event():
    from detail_tts_amd.many import infer_many
    m = FakeModel()
    list(infer_many(m, utterances(3), rows_per_call=2, seed=1))
    assert all("ready" not in r for r in m.requests)
