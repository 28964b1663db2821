"""GPU: the long-form path (detail_tts_amd/longform.py, csrc/wav_join.hip).  The two kernels against their numpy restatement
(tests/longform_ref.py) - the edges as exact integers on planted rows, the join bit for bit - and infer_long against the project's own
infer(batch=True) on the same groups, cut and joined by the restatement, bit for bit.  The reference has no long-form path."""
import numpy as np
import pytest

from longform_ref import edges, frame_rms, join, join_plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 5
CODES = (3, 12, 7, 1, 9)
KINDS = ["sentence", "sentence", "sentence", "sentence", "end"]
SENT, SPACE_ID = 250, 2
SR = 24000


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def model(weights):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(dict(weights), folded=True)


# ------------------------------------------------------------------------------------------------------------ 1. wav_edges
def test_wav_edges_against_the_restatement(model):
    """exact integers at B = 4, stride 4100, frame 256 on planted rows: every frame's RMS is at most threshold / 4 or at least 4 threshold
    (asserted on the float64 values), so the kernel's fp32 sums - within ~1.5e-5 relative of the exact ones - decide as float64 does"""
    rt, B, stride, frame, thr = model.rt, 4, 4100, 256, 0.01
    rs = np.random.RandomState(0)
    quiet = lambda n: (rs.randn(n) * thr / 8).astype(np.float32)
    loud = lambda n: (rs.randn(n) * thr * 16 + np.sign(rs.randn(n)) * thr * 8).astype(np.float32)

    def rows(lens, plant):
        w = np.zeros((B, stride), np.float32)
        for b, n in enumerate(lens):
            w[b, :n] = quiet(n)
        plant(w)
        clean = w.copy()
        for b, n in enumerate(lens):                 # beyond a row's length: must not change anything
            w[b, n:] = 1e30
            w[b, n::2] = np.nan
        for b, n in enumerate(lens):                 # every frame decides far from the threshold
            r = frame_rms(clean[b], n, frame)
            assert ((r <= thr / 4) | (r >= 4 * thr)).all(), (b, r)
        return w, clean

    def case_a(w):      # no loud frame | loud from sample 0 to its end | only the single sample of the last, partial frame | a seam
        w[1, :1000] = loud(1000)
        w[2, 256] = 1.0
        w[3, 255], w[3, 256] = 4.0, 4.0

    def case_b(w):      # frames 3 and 13 of 16 (more frames than waves) | len 0 | the very first and the very last frame | a full stride
        w[0, 3 * 256: 4 * 256] = loud(256)
        w[0, 13 * 256: 14 * 256] = loud(256)
        w[2, :256] = loud(256)
        w[2, 3840: 4000] = loud(160)
        w[3, 1024: 2048] = loud(1024)

    for lens, plant, keeps in (([3000, 1000, 257, 3000], case_a, (0, 100)), ([4096, 0, 4000, 4100], case_b, (0, 300, 5000))):
        w, clean = rows(lens, plant)
        for keep in keeps:
            want = edges(clean, lens, frame=frame, threshold=thr, keep=keep)
            got = rt.wav_edges(dev(w), lens, frame=frame, threshold=thr, keep=keep)
            assert got.dtype == np.int32 and got.shape == (B, 2) and np.array_equal(got, want), (lens, keep, got, want)
            assert np.array_equal(rt.wav_edges(dev(w).view(B, 1, stride), lens, frame=frame, threshold=thr, keep=keep), want)
    # what the planted rows are for, spelled out
    w, clean = rows([3000, 1000, 257, 3000], case_a)
    assert rt.wav_edges(dev(w), [3000, 1000, 257, 3000], threshold=thr).tolist() == [[0, 0], [0, 1000], [256, 257], [0, 512]]
    assert rt.wav_edges(dev(w), [3000, 1000, 257, 3000], threshold=thr, keep=100).tolist() == [[0, 0], [0, 1000], [156, 257], [0, 612]]
    w, clean = rows([4096, 0, 4000, 4100], case_b)
    assert rt.wav_edges(dev(w), [4096, 0, 4000, 4100], threshold=thr).tolist() == [[768, 3584], [0, 0], [0, 4000], [1024, 2048]]
    # a frame that is no multiple of 4 and rows that start unaligned (stride 4099): the scalar path, the same integers
    w2 = np.ascontiguousarray(clean[:, :4099])
    lens2 = [4096, 0, 4000, 4099]
    for fr in (250, 4099):
        for b, n in enumerate(lens2):               # frames that straddle a planted edge: still 1e-3 or more away from the threshold
            assert (np.abs(frame_rms(w2[b], n, fr) / thr - 1) > 1e-3).all()
        assert np.array_equal(rt.wav_edges(dev(w2), lens2, frame=fr, threshold=thr, keep=7), edges(w2, lens2, frame=fr, threshold=thr, keep=7))
    # more than 16 rows: launch after launch
    many = np.concatenate([clean] * 5)[:18]
    lens18 = ([4096, 0, 4000, 4100] * 5)[:18]
    assert np.array_equal(rt.wav_edges(dev(many), lens18, threshold=thr), edges(many, lens18, threshold=thr))
    with pytest.raises(ValueError):
        rt.wav_edges(dev(w), [4101, 0, 0, 0], threshold=thr)
    with pytest.raises(ValueError):
        rt.wav_edges(dev(w), [1, 2, 3], threshold=thr)


# ------------------------------------------------------------------------------------------------------------ 2. wav_join
def test_wav_join_against_the_restatement_bit_for_bit(model):
    rt = model.rt
    rs = np.random.RandomState(1)
    stride = 1100
    counts = [0, 1, 2, 3, 15, 16, 17, 1000]
    wav = rs.randn(8, stride).astype(np.float32)
    wav[7, 40:44] = np.array([-0.0, 1e-40, 3e38, -1e-30], np.float32)
    begins = [5, 0, 1099 - 1, 7, 33, 2, 1083, 37]
    for fade in (8, 0, 1, 600):
        for gaps, lead in (([0] * 8, 0), ([3, 0, 1, 0, 250, 0, 7, 5], 0), ([1] * 8, 13)):
            offsets, at = [], lead
            for c, g in zip(counts, gaps):
                offsets.append(at)
                at += c + g
            want = join(wav, begins, counts, offsets, at, fade=fade)
            got = rt.wav_join(dev(wav), begins, counts, offsets, at, fade=fade)
            assert got.shape == (at,) and got.dtype == torch.float32
            assert got.cpu().numpy().tobytes() == want.tobytes(), (fade, gaps, lead)           # the +0.0 of every gap included
            assert rt.wav_join(dev(wav), begins, counts, offsets, at, fade=fade).cpu().numpy().tobytes() == want.tobytes()      # two calls
    # B = 1, a leading offset, a tail that is no multiple of 4; a [B, 1, stride] batch; total = 0
    for total in (1017, 1018, 1019, 1020):
        want = join(wav[7:], [37], [1000], [9], total, fade=8)
        assert rt.wav_join(dev(wav[7:]).view(1, 1, stride), [37], [1000], [9], total, fade=8).cpu().numpy().tobytes() == want.tobytes()
    assert rt.wav_join(dev(wav[:1]), [0], [0], [0], 0, fade=8).shape == (0,)
    assert float(np.abs(join(wav, begins, counts, list(range(0, 8000, 1000)), 8000, fade=8)).max()) > 1
    # refusals, without a launch
    d = dev(wav[:2])
    for args in (([0, 0], [10, 10], [0, 9], 30), ([0, 0], [10, 10], [12, 0], 30), ([1095, 0], [10, 10], [0, 10], 30),
                 ([0, 0], [10, 10], [0, 10], 19), ([0, 0], [10, 10], [0, 10], 2 ** 31)):
        with pytest.raises(ValueError):
            rt.wav_join(d, *args, fade=8)
    with pytest.raises(ValueError, match="B = 17"):
        rt.wav_join(dev(rs.randn(17, 8)), [0] * 17, [1] * 17, list(range(17)), 17, fade=0)
    import ctypes as C
    from detail_tts_amd import _lib
    bad = [np.array(a, np.int32) for a in ([0, 0], [10, 10], [0, 9])]           # the library checks too, before its launch
    out = torch.zeros(30, device="cuda")
    rc = rt.lib.dtts_wav_join(rt.h, C.c_void_p(d.data_ptr()), 2, stride, *(a.ctypes.data_as(_lib.c_int_p) for a in bad), 30, 8,
                              C.c_void_p(out.data_ptr()), rt._stream())
    assert rc != 0 and b"ascending and disjoint" in rt.lib.dtts_last_error(rt.h)


# ------------------------------------------------------------------------------------------------------------ 3 - 5. end to end
@pytest.fixture(scope="module")
def job(model):
    """a text of five chunks as ids, a prompt mel and its voice, the forced codes, and the yardstick: the three infer(batch=True) calls
    on the groups of rows_per_call = 2, every row cut to its length (computed once, shared, left unchanged)"""
    from detail_tts_amd import longform as L
    rs = np.random.RandomState(31)
    text = np.concatenate([np.concatenate([rs.randint(3, 200, n), [SENT, SPACE_ID]]) for n in (4, 6, 3, 5, 4)])[:-2]
    refer = torch.from_numpy((rs.randn(1, 128, 50) * 2 - 5).astype(np.float32))
    voice = model.get_conditioning_latents(refer, [50])
    forced = [rs.randint(0, 8192, n) for n in CODES]
    chunks = L.plan_chunks(text, sentence_ids=[SENT], space_id=SPACE_ID)
    assert [c["kind"] for c in chunks] == KINDS
    wavs = []
    for req in L.plan_requests(chunks, 2, SEED, voice, forced):
        w = model.infer(req["text"], req["text_length"], None, None, batch=True, speaker=voice, seed=SEED, sample_ids=req["sample_ids"],
                        forced_codes=req["forced_codes"], diffusion_steps=4)
        wavs += [w[b, 0, : 1024 * len(c)].cpu().numpy().copy() for b, c in enumerate(req["forced_codes"])]
    kw = dict(sentence_ids=[SENT], space_id=SPACE_ID, seed=SEED, forced_codes=forced, diffusion_steps=4)
    return dict(text=text, refer=refer, voice=voice, forced=forced, wavs=wavs, kw=kw)


def pauses(model):
    from detail_tts_amd import longform as L
    return {k: L.ms_to_samples(v, SR) for k, v in L.PAUSES_MS.items()}


def test_infer_long_equals_infer_joined_by_the_restatement(model, job):
    lens = [1024 * n for n in CODES]
    want, offsets = join_plan(job["wavs"], lens, KINDS, pauses(model), fade=120)
    kw = dict(job["kw"], speaker=job["voice"], rows_per_call=2, trim_db=None)
    got, chunks = model.infer_long(job["text"], return_chunks=True, **kw)
    assert got.shape == (1, 1, len(want)) and float(np.abs(want).max()) > 1e-4
    assert got[0, 0].cpu().numpy().tobytes() == want.tobytes()
    # the pieces of stream=True, concatenated
    pieces = [p.clone() for p in model.infer_long(job["text"], stream=True, **kw)]
    assert len(pieces) == 3 and torch.equal(torch.cat(pieces, 2).view(torch.int32), got.view(torch.int32))
    # the chunk dicts point at the samples they claim
    w = got[0, 0].cpu().numpy()
    assert [c["offset"] for c in chunks] == offsets and [c["codes"] for c in chunks] == list(CODES)
    for k, c in enumerate(chunks):
        assert (c["begin"], c["end"], c["samples"], c["kind"]) == (0, lens[k], lens[k], KINDS[k])
        n = c["end"] - c["begin"]
        assert np.array_equal(w[c["offset"] + 120: c["offset"] + n - 120], job["wavs"][k][120: n - 120])
        assert c["pause"] == (0 if k == 4 else 9600) and not w[c["offset"] + n: c["offset"] + n + c["pause"]].any()
    assert [c["span"] for c in chunks] == [(0, 6), (6, 14), (14, 19), (19, 26), (26, 30)]
    # a prompt mel in the place of the voice: the same bits
    again = model.infer_long(job["text"], job["refer"], [50], rows_per_call=2, trim_db=None, **job["kw"])
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


def test_the_pipelined_path_equals_infer_as_well(model, job):
    """without forced codes the groups go through infer_stream (group i + 1 decodes under group i's diffusion): sampled codes at a
    fixed length of 6 (suppress_eos), against the blocking infer(batch=True) calls on the same groups joined by the restatement"""
    from detail_tts_amd import longform as L
    G = 6
    kw = dict(sentence_ids=[SENT], space_id=SPACE_ID, seed=SEED, diffusion_steps=4, max_generate_length=G, suppress_eos=True)
    chunks = L.plan_chunks(job["text"], sentence_ids=[SENT], space_id=SPACE_ID)
    wavs = []
    for req in L.plan_requests(chunks, 2, SEED, job["voice"]):
        w = model.infer(req["text"], req["text_length"], None, None, batch=True, speaker=job["voice"], seed=SEED, sample_ids=req["sample_ids"],
                        diffusion_steps=4, max_generate_length=G, suppress_eos=True)
        wavs += [w[b, 0].cpu().numpy().copy() for b in range(w.shape[0])]
    assert all(len(w) == 1024 * (G - 1) for w in wavs)
    want, offsets = join_plan(wavs, [len(w) for w in wavs], KINDS, pauses(model), fade=120)
    got, chunks = model.infer_long(job["text"], speaker=job["voice"], rows_per_call=2, trim_db=None, return_chunks=True, **kw)
    assert got[0, 0].cpu().numpy().tobytes() == want.tobytes() and [c["offset"] for c in chunks] == offsets
    pieces = [p.clone() for p in model.infer_long(job["text"], speaker=job["voice"], rows_per_call=2, trim_db=None, stream=True, **kw)]
    assert len(pieces) == 3 and torch.equal(torch.cat(pieces, 2).view(torch.int32), got.view(torch.int32))


def test_infer_long_with_trimming_on(model, job):
    """the threshold sits in the geometric middle of the widest relative gap between the sorted frame RMS values of the chunks' own
    waveforms (float64), so the kernel's fp32 sums decide as the restatement does; a gap of 1e-3 or less fails the test"""
    lens = [1024 * n for n in CODES]
    rms = np.sort(np.concatenate([frame_rms(w, n) for w, n in zip(job["wavs"], lens)]))
    rms = rms[rms > 0]
    ratio = rms[1:] / rms[:-1]
    i = int(np.argmax(ratio))
    print(f"long_trim_gap {ratio[i] - 1:.3e} between frame rms {rms[i]:.4e} and {rms[i + 1]:.4e} ({i + 1} of {len(rms)} frames below)")
    assert ratio[i] - 1 > 1e-3, "the frame RMS values of the planted codes leave no gap for a threshold: plant other codes"
    thr = float(np.sqrt(rms[i] * rms[i + 1]))
    trim_db, keep = 20 * np.log10(thr), 480
    e = edges(np.stack([np.pad(w, (0, max(lens) - len(w))) for w in job["wavs"]]), lens, threshold=10.0 ** (trim_db / 20.0), keep=keep)
    want, offsets = join_plan(job["wavs"], lens, KINDS, pauses(model), fade=120, edge_list=e)
    got, chunks = model.infer_long(job["text"], speaker=job["voice"], rows_per_call=2, trim_db=trim_db, keep_ms=20, return_chunks=True,
                                   **job["kw"])
    assert [(c["begin"], c["end"]) for c in chunks] == [tuple(r) for r in e.tolist()]
    assert [c["offset"] for c in chunks] == offsets
    assert got[0, 0].cpu().numpy().tobytes() == want.tobytes()


def test_rows_per_call_two_against_five(model, job):
    """the same chunks and code counts under another grouping; a chunk's waveform across batch shapes is NOT promised equal: the
    relative rms difference is printed for the record, with no gate on it"""
    kw = dict(job["kw"], speaker=job["voice"], trim_db=None, return_chunks=True)
    w2, c2 = model.infer_long(job["text"], rows_per_call=2, **kw)
    w5, c5 = model.infer_long(job["text"], rows_per_call=5, **kw)
    assert len(c2) == len(c5) == 5 and [c["codes"] for c in c2] == [c["codes"] for c in c5] == list(CODES)
    assert [c["span"] for c in c2] == [c["span"] for c in c5] and w2.shape == w5.shape
    for k, (a, b) in enumerate(zip(c2, c5)):
        x = w2[0, 0, a["offset"]: a["offset"] + a["end"] - a["begin"]].double()
        y = w5[0, 0, b["offset"]: b["offset"] + b["end"] - b["begin"]].double()
        print(f"long_rows_2_vs_5_chunk{k}_relrms {float((x - y).pow(2).mean().sqrt() / x.pow(2).mean().sqrt()):.3e}")
