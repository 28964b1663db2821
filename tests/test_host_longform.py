"""Host side of the long-form path (detail_tts_amd/longform.py): the splitter's rules on planted strings and id lists, the framing of a
chunk, the planning of infer_long over a fake model whose infer_stream records its requests, and the arithmetic of the join.  No GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from detail_tts_amd import longform as L      # noqa: E402
from detail_tts_amd.config import load_config      # noqa: E402
from detail_tts_amd.voice import Voice      # noqa: E402
from longform_ref import edges, join, join_plan, weights      # noqa: E402

STR = dict(sentence_end=L.SENTENCE_END, clause_end=L.CLAUSE_END, space=L.SPACE)


def split(text, max_len, min_len=0, **kw):
    return L.split_units(text, **(kw or STR), max_len=max_len, min_len=min_len)


def check_tiling(text, spans, max_len):
    """contiguous, covering, within max_len, never blank, the last one "end" and only the last"""
    assert spans[0][0] == 0 and spans[-1][1] == len(text)
    for (a, b, _), (c, _, _) in zip(spans, spans[1:]):
        assert b == c
    marks = set(L.SENTENCE_END + L.CLAUSE_END + L.SPACE)
    for a, b, kind in spans:
        assert 0 < b - a <= max_len, (a, b, kind)
        assert any(u not in marks for u in text[a:b]), (a, b, text[a:b])
    assert [k for _, _, k in spans][-1] == "end" and all(k in L.KINDS[:-1] for _, _, k in spans[:-1])
    assert "".join(text[a:b] for a, b, _ in spans) == text


def test_sentences_and_their_kinds():
    text = "ni3 hao3. wo3 men5 lai2 le5!  zai4 jian4"
    spans = split(text, 40)
    check_tiling(text, spans, 40)
    assert [text[a:b] for a, b, _ in spans] == ["ni3 hao3. ", "wo3 men5 lai2 le5!  ", "zai4 jian4"]       # the run and its spaces stay left
    assert [k for _, _, k in spans] == ["sentence", "sentence", "end"]                                    # trailing text without a mark
    assert split("ni3 hao3.", 40) == [(0, 9, "end")]
    # runs of punctuation: one cut behind the whole run; a run that stands alone goes to its left neighbour
    text = "a1 b2?!。 c3 ... ?! d4."
    spans = split(text, 40)
    check_tiling(text, spans, 40)
    assert [text[a:b] for a, b, _ in spans] == ["a1 b2?!。 ", "c3 ... ?! ", "d4."]
    # ... and a leading one to its right neighbour
    assert split("?! a1. b2", 40) == [(0, 7, "sentence"), (7, 9, "end")]


def test_a_sentence_of_max_len_and_one_more():
    body = "ab " * 5 + "abcd"                 # 19 characters, then the mark: exactly 20
    text = body + "." + "x1"
    assert split(text, 20) == [(0, 20, "sentence"), (20, 22, "end")]
    spans = split(text, 19)                   # one more than max_len: cut at the last space that fits
    check_tiling(text, spans, 19)
    assert spans == [(0, 15, "word"), (15, 20, "sentence"), (20, 22, "end")]


def test_an_overlong_sentence_is_cut_at_a_clause_then_a_space_then_hard():
    text = "aaaa bbbb, cccc dddd eeee."      # the comma is at 9: at or before max_len = 12, the space behind it kept
    spans = split(text, 12)
    check_tiling(text, spans, 12)
    assert spans[0] == (0, 11, "clause") and spans[1] == (11, 21, "word") and spans[2] == (21, 26, "end")
    text = "aaaa bbbb cccc dddd"             # spaces only
    assert split(text, 12) == [(0, 10, "word"), (10, 19, "end")]
    text = "a" * 30 + "."                     # neither
    spans = split(text, 12)
    check_tiling(text, spans, 12)
    assert spans == [(0, 12, "hard"), (12, 24, "hard"), (24, 31, "end")]
    # a clause mark beyond max_len does not count; the LAST one at or before it does
    text = "aa, bb, cccccccccc, dd"
    assert split(text, 10)[0] == (0, 8, "clause")
    # a cut never leaves punctuation alone: 12 letters and a mark at max_len = 12 keep a letter for the mark
    text = "a" * 12 + "!"
    spans = split(text, 12)
    check_tiling(text, spans, 12)
    assert spans == [(0, 11, "hard"), (11, 13, "end")]
    with pytest.raises(ValueError, match="run of spaces and punctuation"):
        split("a" + "!" * 30, 12)


def test_min_len_merges_right_and_at_the_end_left():
    text = "a1. bbbb cccc. d2."
    assert [text[a:b] for a, b, _ in split(text, 40)] == ["a1. ", "bbbb cccc. ", "d2."]
    spans = split(text, 40, min_len=5)
    check_tiling(text, spans, 40)
    assert [text[a:b] for a, b, _ in spans] == ["a1. bbbb cccc. d2."]                                 # right, then the last to its left
    assert [text[a:b] for a, b, _ in split(text, 15, min_len=5)] == ["a1. bbbb cccc. ", "d2."]      # the last: left would exceed max_len
    assert [text[a:b] for a, b, _ in split(text, 18, min_len=5)] == ["a1. bbbb cccc. d2."]         # right, then the last to its left
    text = "aaaa bbbb. c3."
    assert [text[a:b] for a, b, _ in split(text, 40, min_len=5)] == ["aaaa bbbb. c3."]              # the last one merges left
    assert [text[a:b] for a, b, _ in split(text, 12, min_len=5)] == ["aaaa bbbb. ", "c3."]          # ... never beyond max_len


def test_blank_texts_and_bad_limits_are_refused():
    for blank in ("", "   ", " .,! ?", "。。"):
        with pytest.raises(ValueError, match="empty or holds only"):
            split(blank, 10)
    with pytest.raises(ValueError, match="max_len"):
        split("a", 0)
    with pytest.raises(ValueError, match="min_len"):
        split("a", 4, min_len=5)
    with pytest.raises(ValueError, match="empty or holds only"):
        L.split_units([7, 7, 9], sentence_end={9}, space={7}, max_len=4)


def test_ids_split_like_strings():
    """the same rules over ids: 90 ends a sentence, 91 a clause, 2 is the space"""
    rs = np.random.RandomState(0)
    text = "".join(rs.choice(list("abcdefg  ,.!"), 400))
    text = "a" + text + "a"
    table = {c: 10 + i for i, c in enumerate("abcdefg")}
    table.update({" ": 2, ",": 91, ".": 90, "!": 92})
    ids = np.array([table[c] for c in text])
    for max_len, min_len in ((7, 0), (16, 0), (16, 6), (50, 20)):
        want = L.split_units(text, sentence_end=".!", clause_end=",", space=" ", max_len=max_len, min_len=min_len)
        got = L.split_units(ids, sentence_end={90, 92}, clause_end=[91], space=(2,), max_len=max_len, min_len=min_len)
        assert got == want
        check_tiling(text, want, max_len)
    assert {k for _, _, k in L.split_units(ids, sentence_end={90, 92}, clause_end=[91], space=(2,), max_len=7)} == set(L.KINDS)


class _Tok:
    """a character tokenizer that remembers what it was asked to encode"""
    def __init__(self):
        self.seen = []

    def encode(self, s):
        self.seen.append(s)
        return [3 + (ord(c) % 200) for c in s]


def test_framing_in_both_forms():
    tok = _Tok()
    ids = L.frame_chunk("  ni3 hao3.  wo3", 0, 13, tokenizer=tok)
    assert tok.seen == [" ni3 hao3. "] and ids.dtype == np.int32 and ids.tolist() == tok.encode(" ni3 hao3. ") + [0]
    seq = np.array([2, 2, 10, 11, 90, 2, 12])
    assert L.frame_chunk(seq, 0, 6, space_id=2).tolist() == [2, 10, 11, 90, 2, 0]
    assert L.frame_chunk(seq, 0, 6).tolist() == [2, 2, 10, 11, 90, 2, 0]
    assert L.frame_chunk(seq, 6, 7, space_id=2).tolist() == [2, 12, 2, 0]
    with pytest.raises(ValueError, match="tokenizer"):
        L.frame_chunk("a", 0, 1)
    chunks = L.plan_chunks("ni3 hao3. wo3 lai2", tokenizer=_Tok(), max_len=40)
    assert [c["span"] for c in chunks] == [(0, 10), (10, 18)] and [c["kind"] for c in chunks] == ["sentence", "end"]
    assert len(chunks[0]["ids"]) == len(" ni3 hao3. ") + 1 and chunks[0]["ids"][-1] == 0
    chunks = L.plan_chunks(np.array([10, 11, 90, 2, 12]), sentence_ids=[90], space_id=2, max_len=40)
    assert [c["ids"].tolist() for c in chunks] == [[2, 10, 11, 90, 2, 0], [2, 12, 2, 0]]
    with pytest.raises(ValueError, match="sentence_ids"):
        L.plan_chunks(np.array([10, 11]))
    with pytest.raises(ValueError, match="1-D integer"):
        L.plan_chunks(np.zeros((2, 2), np.int64), sentence_ids=[90])


def test_a_chunk_beyond_max_text_tokens_is_refused_by_its_span():
    text = "a" * 30 + ". " + "b" * 50
    with pytest.raises(ValueError, match=r"chunk at 32 \.\. 82 .* 53 ids, more than gpt.max_text_tokens = 40"):
        L.plan_chunks(text, tokenizer=_Tok(), max_len=60, max_text_tokens=40)
    assert len(L.plan_chunks(text, tokenizer=_Tok(), max_len=60, max_text_tokens=53)) == 2


# ---------------------------------------------------------------------------------------------------------------- infer_long over a fake
def voice(S=1):
    return Voice(torch.zeros(S, 768), torch.zeros(S, 1536), torch.zeros(S, 768))


class _Fake:
    """what infer_long reads of a model: cfg, get_conditioning_latents, infer_stream (which records its requests and returns ramps of
    1024 * (row + 1) samples) and join_group (the numpy join)"""
    cfg, device = load_config(), "cpu"

    def __init__(self):
        self.requests, self.voices, self.kw = [], 0, None

    @property
    def rt(self):
        raise AssertionError("device work in the host test")

    def get_conditioning_latents(self, refer, refer_lengths=None):
        self.voices += 1
        return voice()

    def infer_stream(self, requests, **kw):
        self.kw = kw
        for r in requests:
            self.requests.append(r)
            B = r["text"].shape[0]
            lens = [1024 * len(c) for c in r["forced_codes"]] if "forced_codes" in r else [1024 * (b + 1) for b in range(B)]
            wav = torch.zeros(B, 1, max(lens))
            for b, sid in enumerate(r["sample_ids"]):
                wav[b, 0, : lens[b]] = sid + 1
            yield wav, lens

    def infer(self, text, text_length, refer, refer_lengths, noise_scale, **kw):
        """the blocking form: one request, recorded with the marker `blocking`"""
        assert refer is None and refer_lengths is None and kw.pop("batch") is True and kw.pop("return_lengths") is True
        req = dict(text=text, text_length=text_length, blocking=True, **{k: kw[k] for k in ("speaker", "seed", "sample_ids", "forced_codes")})
        return next(self.infer_stream([req]))

    def join_group(self, wav, lens, kinds, plan, base=0, complete=True):
        self.complete = complete
        w = wav[:, 0].numpy()
        e = [(0, n) for n in lens] if plan["threshold"] is None else edges(w, lens, threshold=plan["threshold"], keep=plan["keep"])
        begins, counts, offsets, total, rows = L.plan_join(kinds, e, plan["pauses"], base)
        for row, n in zip(rows, lens):
            row["samples"] = n
        return torch.from_numpy(join(w, begins, counts, offsets, total, fade=plan["fade"])), rows


TEXT = "aa bb. cc dd. ee ff. gg hh. ii jj. kk ll. mm"      # 7 chunks


def run_long(fake, **kw):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    kw.setdefault("tokenizer", _Tok())
    if "refer" not in kw:
        kw.setdefault("speaker", voice())
    return SynthesizerTrn.infer_long(fake, TEXT, **kw)


def test_grouping_sample_ids_and_the_one_seed():
    per_rows = {}
    for rows in (2, 5):
        fake = _Fake()
        wav, chunks = run_long(fake, rows_per_call=rows, seed=11, return_chunks=True, trim_db=None, fade_ms=0)
        assert [r["text"].shape[0] for r in fake.requests] == {2: [2, 2, 2, 1], 5: [5, 2]}[rows]
        assert [s for r in fake.requests for s in r["sample_ids"]] == list(range(7))          # chunk k has sample id k
        assert {r["seed"] for r in fake.requests} == {11}
        assert all(r["speaker"] is fake.requests[0]["speaker"] for r in fake.requests) and fake.voices == 0
        assert [c["span"] for c in chunks] == [(0, 7), (7, 14), (14, 21), (21, 28), (28, 35), (35, 42), (42, 44)]
        assert [c["kind"] for c in chunks] == ["sentence"] * 6 + ["end"]
        for r in fake.requests:                                                                # rows padded with 0 behind their own length
            for b, n in enumerate(r["text_length"]):
                assert r["text"][b, n - 1] == 0 and (r["text"][b, n:] == 0).all() and (r["text"][b, : n - 1] != 0).all()
        per_rows[rows] = [r["text"][b, :n].tolist() for r in fake.requests for b, n in enumerate(r["text_length"])]
        # offsets point at the samples they claim: chunk k is a plateau of k + 1
        w = wav[0, 0].numpy()
        for k, c in enumerate(chunks):
            assert (w[c["offset"]: c["offset"] + c["end"] - c["begin"]] == k + 1).all() and c["codes"] == c["samples"] // 1024
            assert (w[c["offset"] + c["end"] - c["begin"]: c["offset"] + c["end"] - c["begin"] + c["pause"]] == 0).all()
        assert chunks[-1]["pause"] == 0 and chunks[0]["pause"] == 9600 and wav.shape[:2] == (1, 1)
        assert wav.shape[2] == sum(c["end"] - c["begin"] + c["pause"] for c in chunks)
    assert per_rows[2] == per_rows[5]
    fake = _Fake()
    run_long(fake, rows_per_call=3)
    assert len({r["seed"] for r in fake.requests}) == 1                                        # a drawn seed is drawn once


def test_a_prompt_mel_becomes_a_voice_once_and_stream_equals_whole():
    fake = _Fake()
    whole = run_long(fake, refer=torch.zeros(1, 128, 8), refer_lengths=[8], rows_per_call=2, seed=1)
    assert fake.voices == 1 and len(fake.requests) == 4 and all(isinstance(r["speaker"], Voice) for r in fake.requests)
    assert "refer" not in fake.requests[0]
    fake = _Fake()
    gen = run_long(fake, rows_per_call=2, seed=1, stream=True, return_chunks=True, max_generate_length=77, diffusion_steps=4)
    assert fake.requests == []                                                                 # nothing has run yet
    piece, chunks = next(gen)
    assert len(fake.requests) == 1 and len(chunks) == 2 and piece.shape[:2] == (1, 1)          # the first audio after the first group
    rest = list(gen)
    assert torch.equal(torch.cat([piece] + [p for p, _ in rest], 2), whole)
    assert fake.kw["max_generate_length"] == 77 and fake.kw["diffusion_steps"] == 4
    assert [c["offset"] for _, cs in rest for c in cs][0] == piece.shape[2]


def test_every_refusal_comes_before_the_first_request():
    ok = dict(speaker=voice(), tokenizer=_Tok())
    bad = [
        (dict(ok, refer=torch.zeros(1, 128, 8)), "both given"),
        (dict(tokenizer=_Tok(), speaker=None), "neither"),
        (dict(ok, rows_per_call=0), "rows_per_call"),
        (dict(ok, rows_per_call=17), "rows_per_call"),
        (dict(ok, rows_per_call=2.5), "rows_per_call"),
        (dict(ok, decode_options=dict(num_beams=2)), "num_beams"),
        (dict(ok, forced_codes=[np.arange(3)] * 6), "one array per chunk"),
        (dict(ok, pauses_ms={"sentence": 1, "clause": 1, "word": 1}), "hard"),
        (dict(ok, pauses_ms={"sentence": -1, "clause": 1, "word": 1, "hard": 0}), "pauses_ms"),
        (dict(ok, speaker=voice(2)), "ONE voice"),
        (dict(tokenizer=_Tok(), refer=torch.zeros(2, 128, 8)), "ONE voice"),
        (dict(speaker=voice(), tokenizer=None), "tokenizer"),
        (dict(ok, max_len=0), "max_len"),
        (dict(ok, sampler="nope"), "sampler"),
        (dict(ok, trim_db=3.0), "trim_db"),
        (dict(ok, fade_ms=-1), "fade_ms"),
    ]
    for kw, match in bad:
        for stream in (False, True):
            fake = _Fake()
            with pytest.raises(ValueError, match=match):
                run_long(fake, stream=stream, **kw)
            assert fake.requests == [] and fake.voices == 0, kw
    fake = _Fake()
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    with pytest.raises(ValueError, match="sentence_ids"):
        SynthesizerTrn.infer_long(fake, np.arange(5), speaker=voice())
    with pytest.raises(ValueError, match="max_text_tokens"):
        SynthesizerTrn.infer_long(fake, "a" * 900, speaker=voice(), tokenizer=_Tok(), max_len=1000)
    assert fake.requests == []


def test_forced_codes_take_the_blocking_infer_group_by_group():
    """one code array per chunk; the groups run as blocking infer(batch=True) calls (infer_stream decodes forced codes through the KV
    cache, which does not give infer's bits), with the same grouping, ids and seed, and the join is told to wait for them"""
    fake = _Fake()
    forced = [np.arange(n) for n in (3, 1, 2, 5, 1, 1, 4)]
    wav, chunks = run_long(fake, rows_per_call=3, seed=2, forced_codes=forced, return_chunks=True, trim_db=None)
    assert all(r.get("blocking") for r in fake.requests) and fake.complete is False
    assert [r["sample_ids"] for r in fake.requests] == [[0, 1, 2], [3, 4, 5], [6]] and {r["seed"] for r in fake.requests} == {2}
    assert [len(c) for r in fake.requests for c in r["forced_codes"]] == [3, 1, 2, 5, 1, 1, 4] == [c["codes"] for c in chunks]
    fake = _Fake()
    run_long(fake, rows_per_call=3, seed=2)
    assert not any(r.get("blocking") for r in fake.requests) and fake.complete is True


# ---------------------------------------------------------------------------------------------------------------- the join's arithmetic
def test_plan_join_offsets_pauses_and_an_empty_chunk():
    pauses = dict(sentence=100, clause=50, word=10, hard=0)
    kinds = ["sentence", "clause", "hard", "word", "end"]
    e = [(5, 25), (0, 0), (3, 4), (0, 7), (2, 12)]             # the second chunk trimmed to nothing: no samples, its pause stays
    begins, counts, offsets, total, rows = L.plan_join(kinds, e, pauses, base=1000)
    assert begins == [5, 0, 3, 0, 2] and counts == [20, 0, 1, 7, 10]
    assert offsets == [0, 120, 170, 171, 188] and total == 198               # no pause behind the last chunk
    assert [r["offset"] for r in rows] == [1000, 1120, 1170, 1171, 1188] and [r["pause"] for r in rows] == [100, 50, 0, 10, 0]
    # a group that is not the text's last keeps the pause of its last row
    assert L.plan_join(kinds[:2], e[:2], pauses)[3] == 170
    wav = np.arange(5 * 30, dtype=np.float32).reshape(5, 30) + 1
    out = join(wav, begins, counts, offsets, total, fade=0)
    assert (out[:20] == wav[0, 5:25]).all() and (out[20:170] == 0).all() and out[170] == wav[2, 3] and (out[188:] == wav[4, 2:12]).all()
    whole, offs = join_plan(list(wav), [30] * 5, kinds, pauses, fade=0, edge_list=e)
    assert whole.tobytes() == out.tobytes() and offs == offsets
    with pytest.raises(ValueError, match="hard"):
        L.check_pauses(dict(sentence=1, clause=1, word=1))
    assert L.ms_to_samples(400, 24000) == 9600 and L.ms_to_samples(5, 24000) == 120


def test_fade_weights_of_the_restatement():
    assert weights(1000, 8)[:8].tolist() == [np.float32(2 * i + 1) / np.float32(16) for i in range(8)]
    assert weights(1000, 8)[-8:].tolist() == weights(1000, 8)[:8].tolist()[::-1] and (weights(1000, 8)[8:-8] == 1).all()
    assert weights(3, 8).tolist() == [0.5, 1.0, 0.5] and weights(1, 8).tolist() == [1.0] and weights(0, 8).tolist() == []
    assert weights(2, 8).tolist() == [0.5, 0.5] and weights(15, 8)[7] == 1 and weights(16, 8)[7] == np.float32(15) / np.float32(16)
    assert (weights(17, 0) == 1).all()


def test_the_kernels_argument_checks():
    ok = dict(begins=[0, 4], counts=[10, 6], offsets=[0, 12], total=18, fade=8, B=2, stride=10)
    b, c, o, total, fade = L.check_join(**ok)
    assert b.dtype == c.dtype == o.dtype == np.int32 and (total, fade) == (18, 8)
    for change, match in ((dict(offsets=[0, 9]), "ascending and disjoint"), (dict(offsets=[12, 0]), "ascending and disjoint"),
                          (dict(counts=[10, 7]), "reads 4 \\+ 7 samples of a row of 10"), (dict(total=17), "beyond total"),
                          (dict(total=2 ** 31), "2\\*\\*31"), (dict(B=17), "B = 17"), (dict(begins=[0, -1]), "begins"),
                          (dict(fade=-1), "fade"), (dict(counts=[10]), "counts")):
        with pytest.raises(ValueError, match=match):
            L.check_join(**dict(ok, **change))
    lens, frame, thr, keep = L.check_edges([0, 5], 2, 5, 256, 0.5, 3)
    assert lens.dtype == np.int32 and (frame, thr, keep) == (256, 0.5, 3)
    for args in (([0, 6], 2, 5, 256, 0.5, 0), ([0], 2, 5, 256, 0.5, 0), ([0, 5], 2, 5, 0, 0.5, 0), ([0, 5], 2, 5, 256, float("nan"), 0),
                 ([0, 5], 2, 5, 256, 0.5, -1), ([0, 5], 2, 5, 256, -0.5, 0)):
        with pytest.raises(ValueError):
            L.check_edges(*args)
