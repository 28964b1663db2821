"""Per-row sampling settings on the DEVICE (csrc/gpt_kernels.hip sampler_kernel reads its settings at [blockIdx.x]) and what is built on
them: dtts_op_sample_logits_rows, decode sessions whose rows differ (every decode form), the per-row cap latch, the public `sampling=`
and infer_many.  Every comparison is bit for bit."""
import numpy as np
import pytest

import processor_cases as P
import row_sampling_cases as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS = 16


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def rt(weights):
    from detail_tts_amd.runtime import Runtime
    return Runtime(weights, folded=True, parts=("gpt",))


@pytest.fixture(scope="module")
def synth(weights):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(weights, folded=True)


# ------------------------------------------------------------------------------------------------ 1, 2: the unit entry
def test_sixteen_rows_sixteen_settings_one_launch(rt):
    """Every row under its own top-k / top-p / temperature / penalty / typical mass and its own processors, in ONE launch: row r draws
    what the single-row launch under row r's settings as UNIFORM settings draws, and what the NumPy restatement draws wherever the probe
    margins hold - R.COMPARED of the 128 pairs, counted without a GPU in test_host_row_sampling.py."""
    x, rows, sets, us = R.build()
    want, ok = R.restatement()
    recs = [R.row_dict(p, o) for p, o in sets]
    hist, fills, pl = [r["hist"] for r in rows], [r["fills"] for r in rows], [r["prompt_len"] for r in rows]
    compared = 0
    for d in range(R.DRAWS):
        u = us[d]
        packed = rt.op_sample_logits_rows(dev(x), hist, fills, pl, dev(u), recs)
        for i in range(ROWS):
            alone = rt.op_sample_logits_opts(dev(x[i:i + 1]), [hist[i]], [fills[i]], [pl[i]], dev(u[i:i + 1]), **recs[i])
            assert packed[i] == alone[0], (d, i, packed[i], alone[0], sets[i])
            if ok[d, i]:
                assert packed[i] == want[d, i], (d, i, packed[i], want[d, i], sets[i])
                compared += 1
    assert compared == R.COMPARED >= R.DRAWS * ROWS // 2


def test_uniform_rows_are_the_plain_entries(rt):
    """sixteen rows at ONE setting draw what dtts_op_sample_logits_opts draws; at the defaults, what dtts_op_sample_logits draws"""
    rs = np.random.RandomState(91)
    x = (rs.randn(ROWS, P.V0) * 2.0).astype(np.float32)
    hist = rs.randint(2, P.V0, size=(ROWS, 8))
    kw = dict(top_k=20, top_p=0.9, temperature=1.2, repetition_penalty=1.5,
              processors=dict(no_repeat_ngram_size=2, min_new_tokens=3, suppress_tokens=[7, 9], exponential_decay_length_penalty=(1, 1.3), min_p=0.01))
    for _ in range(2):
        u = rs.rand(ROWS).astype(np.float32)
        got = rt.op_sample_logits_rows(dev(x), list(hist), [3] * ROWS, [4] * ROWS, dev(u), [dict(kw) for _ in range(ROWS)])
        assert np.array_equal(got, rt.op_sample_logits_opts(dev(x), list(hist), [3] * ROWS, [4] * ROWS, dev(u), **kw))
        got = rt.op_sample_logits_rows(dev(x), list(hist), [3] * ROWS, [4] * ROWS, dev(u), [{} for _ in range(ROWS)])
        assert np.array_equal(got, rt.op_sample_logits(dev(x), np.concatenate([np.ones((ROWS, 1), np.int64), hist], 1), dev(u)))
    with pytest.raises(Exception, match=r"row_options\[3\].*temperature"):
        rt.op_sample_logits_rows(dev(x), list(hist), [3] * ROWS, [4] * ROWS, dev(u), [dict(temperature=0.0 if i == 3 else 1.0) for i in range(ROWS)])


# ------------------------------------------------------------------------------------------------ 3, 4: sessions
KINDS = (dict(do_sample=False), dict(temperature=1.3, top_p=0.95, top_k=0), dict(no_repeat_ngram_size=2, min_new_tokens=6),
         dict(max_generate_length=9))


def session_inputs(B, seed=5):
    rs = np.random.RandomState(seed)
    refer = dev(rs.randn(B, 128, 64) * 2 - 5)
    texts = [np.concatenate([rs.randint(3, 255, 7), [0]]).astype(np.int32) for _ in range(B)]          # 8 ids
    return refer, [64] * B, texts, 17, [30 + b for b in range(B)]


def records(sampling, B, G):
    from detail_tts_amd.gpt.sampling import resolve_sampling
    return resolve_sampling(sampling, B, top_k=50, max_generate_length=G, decode_options=None, always_rows=True)


def uniform_kw(rec):
    """a row record as the scalar keywords of a uniform session"""
    return dict(max_generate_length=rec["max_generate_length"], top_k=rec["top_k"], top_p=rec["top_p"], temperature=rec["temperature"],
                repetition_penalty=rec["repetition_penalty"], typical_mass=rec["typical_mass"], processors=rec["processors"] or None)


def check_rows_against_uniform(rt, B, G, **extra):
    """row b of the mixed session (row b under KINDS[b % 4]) == row b of the uniform session of the same rows under that kind: codes,
    ncodes and the latent columns [0, ncodes_b).  -> (mixed codes, the all-defaults session's codes)"""
    inp = session_inputs(B)
    recs = records([KINDS[b % 4] for b in range(B)], B, G)
    codes, ncodes, lat = rt.gpt_generate(*inp, max_generate_length=G, rows=recs, **extra)
    lat = lat.cpu().numpy()
    for k in range(min(4, B)):
        kw = uniform_kw(recs[k])
        rc, rn, rl = rt.gpt_generate(*inp, **kw, **extra)
        rl = rl.cpu().numpy()
        cap = kw["max_generate_length"]
        for b in range(k, B, 4):
            assert ncodes[b] == rn[b] <= cap, (k, b, ncodes[b], rn[b])
            assert np.array_equal(codes[b, :cap], rc[b]) and (codes[b, cap:] == 8193).all(), (k, b, codes[b], rc[b])
            n = int(ncodes[b])
            assert np.array_equal(lat[b, :, :n], rl[b, :, :n]), (k, b)
    plain, _, _ = rt.gpt_generate(*inp, max_generate_length=G, **extra)
    return codes, plain


@pytest.mark.parametrize("form", ["token", "chain", "graph"])
def test_a_mixed_session_decodes_every_row_under_its_own_settings(rt, form):
    """B = 4: (greedy), (temperature 1.3, top-p 0.95, top-k 0), (defaults + no_repeat_ngram_size 2 + min_new_tokens 6), (defaults, cap 9)
    in ONE session against four uniform sessions; on the token kernel, on the 53-launch chain and replayed from the captured graphs."""
    opt = dict(token=None, chain=("gpt_token_kernel", 0, 1), graph=("gpt_graph", 1, 0))[form]
    if opt:
        rt.set_option(opt[0], opt[1])
    try:
        codes, plain = check_rows_against_uniform(rt, 4, 24)
    finally:
        if opt:
            rt.set_option(opt[0], opt[2])
    assert not np.array_equal(codes[0], plain[0]) and not np.array_equal(codes[1], plain[1])      # the settings act on the session
    assert np.array_equal(codes[3, :9], plain[3, :9])                                              # ... and a cap alone changes no draw


@pytest.mark.parametrize("B, wgs", [(8, 128), (8, 64), (16, 0)])
def test_wide_sessions(rt, B, wgs):
    check_rows_against_uniform(rt, B, 12, token_wgs=wgs)


def test_a_replayed_session_keeps_the_rows_settings(rt):
    """the record a session is replayed from on the chain (the token kernel's timeout path, reached through the existing test hook
    that raises its error flag) keeps the per-row settings and their id lists: the replay returns the chain's mixed session"""
    G, inp = 12, session_inputs(4)
    recs = records([dict(KINDS[0], suppress_tokens=[3, 4]), KINDS[1], dict(KINDS[2], begin_suppress_tokens=[8193]), KINDS[3]], 4, G)
    try:
        rt.set_option("gpt_token_kernel", 0)
        c_chain, n_chain, l_chain = rt.gpt_generate(*inp, max_generate_length=G, rows=recs)
        rt.set_option("gpt_token_kernel", 1)
        rt.set_option("gpt_token_fault", 7)
        c1, n1, l1 = rt.gpt_generate(*inp, max_generate_length=G, rows=recs)
    finally:
        rt.set_option("gpt_token_kernel", 1)         # clears the latch
    assert np.array_equal(c1, c_chain) and np.array_equal(n1, n_chain)
    for b in range(4):
        assert torch.equal(l1[b, :, : int(n1[b])], l_chain[b, :, : int(n1[b])]), b


# ------------------------------------------------------------------------------------------------ 5: the cap latch
def test_a_row_is_finished_at_its_own_cap(rt):
    """B = 2: row 0 is forced to stop after two codes, row 1 (which cannot draw the stop token: min_new_tokens) has a cap of 8 inside a
    call cap of 64.  The session is finished once 8 steps are done - not before, and without running on to 64 - and row 1 reports 8 codes
    and 8193 behind them."""
    G = 64
    inp = session_inputs(2)
    recs = records([None, dict(max_generate_length=8, min_new_tokens=G)], 2, G)
    rt.gpt_prefill(*inp, max_generate_length=G, rows=recs, forced_codes=[[5, 6, 8193], []], forced_fill=-1)
    seen = []
    while rt.gpt_steps() < G and not rt.gpt_all_finished():
        seen.append(rt.gpt_steps())
        rt.gpt_decode(1)
    assert seen == list(range(1, 8)) and rt.gpt_steps() == 8 and rt.gpt_all_finished()
    rt.gpt_decode(3)                                               # steps past the latch change nothing the host reads
    codes, ncodes, _ = rt.gpt_finish()
    assert ncodes.tolist() == [3, 8]
    assert codes[0, :3].tolist() == [5, 6, 8193] and (codes[0, 3:] == 8193).all()
    assert (codes[1, :8] != 8193).all() and (codes[1, 8:] == 8193).all()
    ref, rn, _ = rt.gpt_generate(*inp, max_generate_length=8, processors=dict(min_new_tokens=G))
    assert rn[1] == 8 and np.array_equal(codes[1, :8], ref[1])    # what a uniform session with max_generate_length = 8 reports


# ------------------------------------------------------------------------------------------------ 6, 7: the public path
def public_request(B=2, seed=3):
    rs = np.random.RandomState(seed)
    text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, 7)), np.zeros((B, 1), np.int64)], 1))          # 8 ids
    refer = torch.from_numpy((rs.randn(B, 128, 40) * 2 - 5).astype(np.float32))
    return text, torch.tensor([8] * B), refer, torch.tensor([40] * B)


def test_public_sampling(synth):
    text, tl, refer, rl = public_request()
    kw = dict(batch=True, seed=9, sample_ids=[21, 22], max_generate_length=8, diffusion_steps=2)
    w0 = synth.infer(text, tl, refer, rl, **kw)
    for s in (None, {}, [None, None]):
        assert torch.equal(synth.infer(text, tl, refer, rl, sampling=s, **kw), w0)
    cool = dict(temperature=0.6)
    w1 = synth.infer(text, tl, refer, rl, sampling=cool, **kw)
    assert torch.equal(synth.infer(text, tl, refer, rl, sampling=[dict(cool), dict(cool)], **kw), w1)
    assert not torch.equal(w1, w0)
    mixed = [dict(temperature=1.3, top_p=0.95, top_k=0), dict(do_sample=False, max_generate_length=6)]
    w2, n2 = synth.infer(text, tl, refer, rl, sampling=mixed, return_lengths=True, **kw)
    assert n2[1] <= 1024 * 5                                       # row 1 ran into its own cap of 6: five codes in front of the last
    req = dict(text=text, text_length=tl, refer=refer, refer_lengths=rl, seed=9, sample_ids=[21, 22], sampling=mixed)
    (ws, ns), = list(synth.infer_stream(iter([req]), max_generate_length=8, diffusion_steps=2))
    assert torch.equal(ws, w2) and list(ns) == list(n2)
    (ws, _), = list(synth.infer_stream(iter([dict(req, sampling=None)]), max_generate_length=8, diffusion_steps=2, sampling=cool))
    assert torch.equal(ws, w1)                                     # the stream-wide default
    wc = synth.infer(text, tl, refer, rl, sampling=mixed, num_candidates=2, choose=[0, 0], **kw)
    assert torch.equal(wc, w2)                                     # candidate 0 IS the N = 1 call; the settings repeat with the rows


def test_infer_many_is_the_blocking_call_row_by_row(synth):
    """5 utterances - three voices, one prompt mel used twice, different `sampling`, one at speed 0.8 - at 2 rows per call: every
    yielded (wav, length) is that row of the blocking infer on the same group, cut at its length, in input order."""
    from detail_tts_amd.voice import Voice
    rs = np.random.RandomState(12)
    mel = torch.from_numpy((rs.randn(128, 40) * 2 - 5).astype(np.float32))
    va, vb = (synth.get_conditioning_latents(torch.from_numpy((rs.randn(1, 128, 30 + 10 * i) * 2 - 5).astype(np.float32))) for i in range(2))
    texts = [np.concatenate([rs.randint(3, 255, 5 + i % 3), [0]]) for i in range(5)]
    us = [dict(text=texts[0], refer=mel, sampling=dict(temperature=0.6)),
          dict(text=texts[1], speaker=va, sampling=dict(do_sample=False), sample_id=70),
          dict(text=texts[2], speaker=vb, speed=0.8),
          dict(text=texts[3], refer=mel, sampling=dict(top_k=0, top_p=0.95, max_generate_length=6)),
          dict(text=texts[4], speaker=va)]
    kw = dict(max_generate_length=8, diffusion_steps=2)
    got = list(synth.infer_many(iter(us), rows_per_call=2, seed=4, **kw))
    assert len(got) == 5
    vm = synth.get_conditioning_latents(mel[None])
    voices = [vm, va, vb, vm, va]
    sids = [0, 70, 2, 3, 4]
    for g0 in range(0, 5, 2):
        idx = list(range(g0, min(g0 + 2, 5)))
        lt = max(len(texts[i]) for i in idx)
        text = torch.zeros((len(idx), lt), dtype=torch.int64)
        for b, i in enumerate(idx):
            text[b, : len(texts[i])] = torch.from_numpy(texts[i])
        extra = dict(speed=[us[i].get("speed", 1.0) for i in idx]) if any("speed" in us[i] for i in idx) else {}
        wav, lens = synth.infer(text, [len(texts[i]) for i in idx], None, None, batch=True, speaker=Voice.cat([voices[i] for i in idx]),
                                sampling=[us[i].get("sampling") for i in idx], seed=4, sample_ids=[sids[i] for i in idx],
                                return_lengths=True, **extra, **kw)
        for b, i in enumerate(idx):
            assert got[i][1] == lens[b] and tuple(got[i][0].shape) == (1, 1, lens[b]), (i, got[i][1], lens[b])
            assert torch.equal(got[i][0], wav[b:b + 1, :, : lens[b]]), i


# ------------------------------------------------------------------------------------------------ the other entries that take sampling
def decoded(m, call):
    """the (codes, ncodes) of every decode session `call` runs (rt.gpt_generate and rt.gpt_finish spied on)"""
    seen, orig_g, orig_f = [], m.rt.gpt_generate, m.rt.gpt_finish

    def spy(orig):
        def f(*a, **k):
            out = orig(*a, **k)
            seen.append((np.array(out[0]), np.array(out[1])))
            return out
        return f
    m.rt.gpt_generate, m.rt.gpt_finish = spy(orig_g), spy(orig_f)
    try:
        call()
    finally:
        m.rt.gpt_generate, m.rt.gpt_finish = orig_g, orig_f
    return seen


MIXED = [dict(temperature=1.3, top_p=0.95, top_k=0), dict(do_sample=False, max_generate_length=6)]


def assert_row_of(mixed, uniform, b, cap):
    """row b of a mixed session is row b of the uniform session under row b's settings"""
    (mc, mn), (uc, un) = mixed, uniform
    assert mn[b] == un[b] <= cap and np.array_equal(mc[b, :cap], uc[b, :cap]) and (mc[b, cap:] == 8193).all(), (b, mc[b], uc[b])


def test_infer_gpt_sampling(synth):
    text, tl, refer, rl = public_request()
    kw = dict(batch=True, seed=9, sample_ids=[21, 22], max_generate_length=8)
    mixed, = decoded(synth, lambda: synth.infer_gpt(text, tl, refer, rl, sampling=MIXED, **kw))
    for b, cap in ((0, 8), (1, 6)):
        uni, = decoded(synth, lambda: synth.infer_gpt(text, tl, refer, rl, sampling=MIXED[b], **kw))
        assert_row_of(mixed, uni, b, cap)
    plain, = decoded(synth, lambda: synth.infer_gpt(text, tl, refer, rl, **kw))
    assert not np.array_equal(mixed[0][0], plain[0][0]) and not np.array_equal(mixed[0][1, :6], plain[0][1, :6])


def test_paired_requests_keep_their_own_rows(synth):
    """infer_stream(pair_stage_a=True): two requests of two rows decode as ONE session of four; each request's waveform is its own
    blocking infer's, under its own rows' settings (the second request carries none and takes the stream's default)"""
    text, tl, refer, rl = public_request()
    t2, l2, r2, rl2 = public_request(seed=4)
    cool = dict(temperature=0.6)
    reqs = [dict(text=text, text_length=tl, refer=refer, refer_lengths=rl, seed=9, sample_ids=[21, 22], sampling=MIXED),
            dict(text=t2, text_length=l2, refer=r2, refer_lengths=rl2, seed=10, sample_ids=[5, 6])]
    kw = dict(max_generate_length=8, diffusion_steps=2)
    got = []
    sessions = decoded(synth, lambda: got.extend((w.clone(), list(n)) for w, n in synth.infer_stream(iter(reqs), pair_stage_a=True, sampling=cool, **kw)))
    assert len(got) == 2 and len(sessions) == 1 and sessions[0][0].shape[0] == 4          # one session of four rows
    for r, s, (w, n) in zip(reqs, (MIXED, cool), got):
        want, lens = synth.infer(r["text"], r["text_length"], r["refer"], r["refer_lengths"], batch=True, seed=r["seed"],
                                 sample_ids=r["sample_ids"], sampling=s, return_lengths=True, **kw)
        assert n == lens
        for b in range(2):
            assert torch.equal(w[b, :, : n[b]], want[b, :, : n[b]]), b


def test_more_than_sixteen_rows_slice_the_row_options(rt):
    """dtts_gpt_generate with 18 rows: the second group of 2 decodes under ITS slice of the records"""
    G, B = 10, 18
    inp = session_inputs(B)
    recs = records([KINDS[b % 4] if b < 16 else (KINDS[1], dict(max_generate_length=5))[b - 16] for b in range(B)], B, G)
    codes, ncodes, _ = rt.gpt_generate(*inp, max_generate_length=G, rows=recs)
    refer, rl, texts, seed, sids = inp
    tail = (refer[16:].contiguous(), rl[16:], texts[16:], seed, sids[16:])
    for b in (16, 17):
        kw = uniform_kw(recs[b])
        rc, rn, _ = rt.gpt_generate(*tail, **kw)
        cap = kw["max_generate_length"]
        assert ncodes[b] == rn[b - 16] <= cap and np.array_equal(codes[b, :cap], rc[b - 16]) and (codes[b, cap:] == 8193).all(), b
    plain, _, _ = rt.gpt_generate(*tail, max_generate_length=G)
    assert not np.array_equal(codes[16], plain[0])


def test_the_mirror_takes_the_list_form(rt):
    """UnifiedVoice.inference_speech_tortoise / _valle(sampling=[...]): row against the uniform call under that row's keywords; a
    missing key is the call's own value; with num_return_sequences = 2 the settings repeat with the rows"""
    from detail_tts_amd.config import load_config
    from detail_tts_amd.gpt.model import UnifiedVoice
    uv = UnifiedVoice(rt, load_config()["gpt"])
    refer, _, texts, seed, _ = session_inputs(2)
    text = torch.from_numpy(np.stack(texts).astype(np.int64))
    G = 10
    common = dict(max_generate_length=G, seed=seed, do_sample=True, top_p=0.8, temperature=0.8, repetition_penalty=2.0)
    rows = [dict(temperature=1.3, top_k=0), dict(do_sample=False, max_generate_length=6)]
    prompt = np.random.RandomState(2).randint(0, 8192, (2, 5))

    def padded(out, n):
        out = out.cpu().numpy()
        return np.concatenate([out, np.full((n, G - out.shape[1]), 8193, out.dtype)], 1)
    for call, extra in ((uv.inference_speech_tortoise, ()), (uv.inference_speech_valle, (prompt,))):
        for nrs in (1, 2):
            ids = [40, 50] if nrs == 1 else [40, 41, 50, 51]
            mixed = padded(call(refer, None, text, *extra, num_return_sequences=nrs, sample_ids=ids, sampling=rows, **common), 2 * nrs)
            hot = padded(call(refer, None, text, *extra, num_return_sequences=nrs, sample_ids=ids, **dict(common, temperature=1.3, top_k=0)), 2 * nrs)
            greedy = padded(call(refer, None, text, *extra, num_return_sequences=nrs, sample_ids=ids, **dict(common, do_sample=False, max_generate_length=6)), 2 * nrs)
            assert np.array_equal(mixed[:nrs], hot[:nrs]), (call.__name__, nrs)
            assert np.array_equal(mixed[nrs:, :6], greedy[nrs:, :6]) and (mixed[nrs:, 6:] == 8193).all(), (call.__name__, nrs)
    with pytest.raises(ValueError, match="forced_uniforms"):
        uv.inference_speech_tortoise(refer, None, text, sampling=dict(max_generate_length=6), forced_uniforms=torch.zeros((2, G), device="cuda"), **common)
    with pytest.raises(ValueError, match="input_tokens"):
        uv.inference_speech_tortoise(refer[:1], None, text[:1], sampling=dict(max_generate_length=2), input_tokens=np.array([[3, 4, 5]]), **common)


def test_infer_long_hands_the_dict_to_its_groups(synth):
    """infer_long(sampling=dict): every chunk is the row of the blocking infer(batch=True, sampling=dict) on its group (away from the
    join's fades), and not the default decode's"""
    from detail_tts_amd import longform as L
    SENT, SPACE = 250, 2
    rs = np.random.RandomState(31)
    text = np.concatenate([np.concatenate([rs.randint(3, 200, n), [SENT, SPACE]]) for n in (4, 6, 3)])[:-2]
    voice = synth.get_conditioning_latents(torch.from_numpy((rs.randn(1, 128, 50) * 2 - 5).astype(np.float32)), [50])
    torch.cuda.synchronize()           # (infer_stream reads a request's tensors on its own stream: they have to be complete)
    hot = dict(temperature=1.4, top_k=0, top_p=0.95)
    kw = dict(seed=5, diffusion_steps=2, max_generate_length=6, suppress_eos=True)
    got, chunks = synth.infer_long(text, speaker=voice, rows_per_call=2, trim_db=None, return_chunks=True, sentence_ids=[SENT], space_id=SPACE,
                                   sampling=hot, **kw)
    w = got[0, 0].cpu().numpy()
    plan = L.plan_chunks(text, sentence_ids=[SENT], space_id=SPACE)
    k, differs = 0, False
    for req in L.plan_requests(plan, 2, 5, voice):
        args = (req["text"], req["text_length"], None, None)
        want = synth.infer(*args, batch=True, speaker=voice, sample_ids=req["sample_ids"], sampling=hot, **kw).cpu().numpy()
        plain = synth.infer(*args, batch=True, speaker=voice, sample_ids=req["sample_ids"], **kw).cpu().numpy()
        for b in range(want.shape[0]):
            c = chunks[k]
            n = c["end"] - c["begin"]
            assert n == 1024 * 5 and np.array_equal(w[c["offset"] + 120: c["offset"] + n - 120], want[b, 0, 120: n - 120]), k
            differs = differs or not np.array_equal(want[b, 0, :n], plain[b, 0, :n])
            k += 1
    assert k == 3 and differs


def test_unit_entries_check_a_callers_row_options(rt):
    """dtts_op_sample_logits_opts validates row_options it is handed; dtts_op_beam_step refuses them (a beam session is uniform)"""
    import ctypes as C
    from detail_tts_amd import _lib
    o = _lib.DttsGptOptions()
    rt.lib.dtts_gpt_options_init(C.byref(o))
    rows = (_lib.DttsGptRowOptions * 2)()
    for q in rows:
        q.temperature, q.top_p, q.repetition_penalty, q.top_k, q.max_generate_length = 1.0, 1.0, 1.0, 0, 1
    rows[1].temperature = -1.0
    o.row_options = rows
    x = dev(np.zeros((2, 64)))
    u = dev(np.array([0.5, 0.5]))
    ints = lambda *v: np.array(v, np.int32)      # noqa: E731
    hl, fl, pl, out = ints(0, 0), ints(1, 1), ints(1, 1), ints(0, 0)
    ip = lambda a: a.ctypes.data_as(_lib.c_int_p)      # noqa: E731
    rc = rt.lib.dtts_op_sample_logits_opts(rt.h, C.c_void_p(x.data_ptr()), 2, 64, C.byref(o), None, 0, ip(hl), ip(fl), ip(pl),
                                           C.c_void_p(u.data_ptr()), ip(out), rt._stream())
    assert rc != 0 and b"row_options[1]" in rt.lib.dtts_last_error(rt.h)
    rows[1].temperature = 1.0
    rc = rt.lib.dtts_op_sample_logits_opts(rt.h, C.c_void_p(x.data_ptr()), 2, 64, C.byref(o), None, 0, ip(hl), ip(fl), ip(pl),
                                           C.c_void_p(u.data_ptr()), ip(out), rt._stream())
    assert rc == 0
    o.num_beams, o.max_generate_length = 2, 4
    z = np.zeros(64, np.int32)
    zf = np.zeros(64, np.float32)
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)      # noqa: E731
    rc = rt.lib.dtts_op_beam_step(rt.h, C.c_void_p(x.data_ptr()), 1, 64, C.byref(o), 0, None, 0, ip(z), fp(zf), ip(z), fp(zf), ip(z), ip(z), ip(z),
                                  ip(z), ip(z), ip(z), fp(zf), ip(z), ip(z), rt._stream())
    assert rc != 0 and b"row_options" in rt.lib.dtts_last_error(rt.h)
