"""GPU: speaking-rate control in stage B (detail_tts_amd/duration.py, csrc/frame_map.hip).  The two map kernels against their numpy
restatement (tests/duration_ref.py) as exact integers; the planned code embedding against the reference's own
DiffusionTts.timestep_independent at other frame counts (tests/golden/duration_emb.npz) and, bit for bit, against the x4 embedding's
columns; and infer / infer_stream / infer_long under a plan against the manual composition of the same launches, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import duration_ref as R
from conftest import tol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 11
N_CODES = (14, 26, 6)            # a ragged batch of B = 3
STEPS = 3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def model(weights):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(dict(weights), folded=True)


@pytest.fixture(scope="module")
def job():
    """a ragged request of B = 3 with forced codes (computed once, shared, left unchanged)"""
    rs = np.random.RandomState(17)
    B = len(N_CODES)
    text = torch.from_numpy(np.concatenate([rs.randint(3, 200, (B, 6)), np.full((B, 1), 2), rs.randint(3, 200, (B, 4)), np.zeros((B, 1), np.int64)],
                                           1).astype(np.int32))
    tl = [12, 10, 12]
    text[1, 9:] = 0
    refer = torch.from_numpy((rs.randn(B, 128, 48) * 2 - 5).astype(np.float32))
    rl = [48, 41, 45]
    codes = [rs.randint(0, 8192, n) for n in N_CODES]
    return dict(args=(text, tl, refer, rl), codes=codes, kw=dict(batch=True, seed=SEED, sample_ids=[3, 4, 9], diffusion_steps=STEPS))


def compose(model, job, *, frames, durations=None):
    """stage by stage, by hand: the teacher-forced latents of the forced codes -> the planned embedding -> diff_sample_ex -> vocoder
    with the plan's lengths, as infer() chains them -> (wav, code_emb)"""
    from detail_tts_amd.pipeline import normalize_request
    from detail_tts_amd.vqvae.model_24k import NOISE_SCALE, sampling_args
    rt = model.rt
    text, tl, refer, rl = job["args"]
    st = normalize_request(text, tl, refer, rl, job["kw"]["seed"], job["kw"]["sample_ids"], job["codes"])
    refer = st.refer.to(model.device, torch.float32).contiguous()
    lat = rt.gpt_latents(refer, st.rl, st.texts, job["codes"])
    emb = rt.diff_timestep_independent(lat, rt.diff_conditioning(refer, st.rl), list(N_CODES), frames=frames, durations=durations)
    sched_ts, sampler_id, eta = sampling_args(STEPS, "p", 0.0)
    mel = rt.diff_sample_ex(emb, st.seed, st.sids, sched=rt.sampler_schedule(sched_ts, sampler_id), sampler=sampler_id, eta=eta,
                            lens=list(frames), denorm=True)
    return rt.vocoder(mel, st.seed, st.sids, lens=list(frames), noise_scale=NOISE_SCALE), emb


def assert_rows_equal(wav, want, frames):
    """the rows up to their own lengths, bit for bit.  Beyond a row's length stage C writes nothing - the waveform is allocated
    uninitialised, with a plan as without one - so nothing can be asserted there"""
    assert wav.shape == want.shape == (len(frames), 1, 256 * max(frames))
    for b, T in enumerate(frames):
        assert torch.equal(bits(wav[b, 0, : 256 * T]), bits(want[b, 0, : 256 * T])), b
        assert bool(torch.isfinite(wav[b, 0, : 256 * T]).all()) and float(wav[b, 0, : 256 * T].pow(2).mean().sqrt()) > 1e-6


# ------------------------------------------------------------------------------------------------------------ 1. the map kernels
def test_frame_map_uniform_against_the_restatement(model):
    rt = model.rt
    for n, T in R.HARD_PAIRS + ((12, 48), (1, 4), (26, 104), (300, 1296)):
        got = rt.op_frame_map([n], [T]).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == (1, T) and np.array_equal(got[0], R.uniform_map(n, T)), (n, T)
    for (n, T), frames in R.HARD_FRAMES.items():                      # where an integer floor would land one code further
        got = rt.op_frame_map([n], [T]).cpu().numpy()[0]
        assert all(got[t] == t * n // T - 1 for t in frames), (n, T)
    ns, Ts = [p[0] for p in R.HARD_PAIRS], [p[1] for p in R.HARD_PAIRS]
    got = rt.op_frame_map(ns, Ts).cpu().numpy()                        # one ragged batch: more than one block along t, -1 beyond a row
    assert got.shape == (5, 148) and np.array_equal(got, R.padded_maps([R.uniform_map(n, T) for n, T in R.HARD_PAIRS], 148))
    got = rt.op_frame_map(ns, Ts, nmax=40, Tmax=600).cpu().numpy()     # a wider rectangle than the rows need: three blocks along t
    assert np.array_equal(got, R.padded_maps([R.uniform_map(n, T) for n, T in R.HARD_PAIRS], 600))


def test_frame_map_durations_against_the_restatement(model):
    rt = model.rt
    rs = np.random.RandomState(3)
    rows = [[0, 0, 3, 0, 0, 5, 2, 0, 0, 2], [4] * 8, [0, 0, 0, 0, 0, 0, 16, 0, 0], [7, 0, 0, 0, 0, 1], [1] * 12]
    lens = [len(d) for d in rows]
    frames = [sum(d) for d in rows]
    assert all(f % 4 == 0 for f in frames)
    got = rt.op_frame_map(lens, frames, rows).cpu().numpy()
    assert got.shape == (5, 32) and np.array_equal(got, R.padded_maps([R.durations_map(d) for d in rows], 32))
    for d in rows:                                                     # every row alone
        assert np.array_equal(rt.op_frame_map([len(d)], [sum(d)], [d]).cpu().numpy()[0], np.repeat(np.arange(len(d)), d))
    # nmax beyond one scan chunk of 256 codes: runs that straddle the chunk seams, zeros on either side of them, a chunk of zeros alone
    big = []
    for n in (257, 600, 1406):
        d = rs.randint(0, 4, n)
        d[rs.rand(n) < 0.4] = 0
        d[250:262] = [0, 3, 0, 0, 0, 2, 5, 0, 0, 0, 0, 1][: max(0, min(12, n - 250))]
        if n > 800:
            d[512:768] = 0
        d[-1] += (-int(d.sum())) % 4
        big.append(d)
    for d in big:
        got = rt.op_frame_map([len(d)], [int(d.sum())], [d]).cpu().numpy()[0]
        assert np.array_equal(got, R.durations_map(d)), len(d)
    frames = [int(d.sum()) for d in big]
    got = rt.op_frame_map([len(d) for d in big], frames, big, Tmax=max(frames) + 8).cpu().numpy()
    assert np.array_equal(got, R.padded_maps([R.durations_map(d) for d in big], max(frames) + 8))
    one = np.zeros(300, np.int64)
    one[299] = 1000                                                    # one code, in the second chunk, owns every frame
    assert np.array_equal(rt.op_frame_map([300], [1000], [one]).cpu().numpy()[0], np.full(1000, 299))


def test_frame_plan_refusals_come_with_a_message(model):
    from detail_tts_amd import _lib
    from detail_tts_amd.runtime import DttsError
    rt = model.rt
    for args, what in ((([6], [10]), "multiple of 4"), (([6], [8], [[1, 1, 1, 1, 1, 1]]), "sum to frames"),
                       (([6], [8], [[9, -1, 0, 0, 0, 0]]), "durations >= 0")):
        with pytest.raises(DttsError, match=what):
            rt.op_frame_map(*args)
    for frames in ([8, 16], [0, 8]):
        with pytest.raises(DttsError, match=r"frames\[b\] in 1 .. Tmax"):
            rt.op_frame_map([6, 6], frames, Tmax=12)
    with pytest.raises(ValueError):
        rt.op_frame_map([6, 6], [8])
    # the embedding entry refuses the same, before any launch, and says why
    lat, cond = torch.zeros((1, 768, 6), device="cuda"), torch.zeros((1, 1536), device="cuda")
    out = torch.zeros((1, 768, 16), device="cuda")
    fr, du = np.array([16], np.int32), np.array([4, 4, 4, 1, 1, 1], np.int32)
    call = lambda f, d, Tmax: rt.lib.dtts_diff_timestep_independent_ex(  # noqa: E731
        rt.h, C.c_void_p(lat.data_ptr()), None, 1, 6, C.c_void_p(cond.data_ptr()), f.ctypes.data_as(_lib.c_int_p),
        None if d is None else d.ctypes.data_as(_lib.c_int_p), Tmax, C.c_void_p(out.data_ptr()), rt._stream())
    assert call(fr, du, 16) != 0 and b"sum to frames" in rt.lib.dtts_last_error(rt.h)
    assert call(np.array([20], np.int32), None, 16) != 0 and b"frames[b] in 1 .. Tmax" in rt.lib.dtts_last_error(rt.h)
    assert call(np.array([14], np.int32), None, 14) != 0 and b"multiple of 4" in rt.lib.dtts_last_error(rt.h)
    assert not bool(out.any())


# ------------------------------------------------------------------------------------------------------------ 2. the embedding
def test_planned_embedding_against_the_reference_and_the_x4_columns(model, golden):
    """the gate is the one tests/test_gpu_diffusion.py::test_conditioning_and_code_emb_golden holds the x4 embedding to (2e-4 against
    the reference's CPU result); the placement is held bit for bit: column t of the planned embedding is column 4 m[t] of the x4
    embedding of the same input (the affine is per element)"""
    rt, g = model.rt, golden("duration_emb")
    cs, cond = int(g["ch_stride"]), dev(g["cond_latent"])
    lat = {n: dev(g[f"latent_{n}"].transpose(0, 2, 1)) for n in (14, 26, 12)}
    x4 = {n: rt.diff_timestep_independent(lat[n], cond) for n in lat}
    for n, T in [tuple(c) for c in g["cases"].tolist()]:
        got = rt.diff_timestep_independent(lat[n], cond, frames=[T])
        assert got.shape == (1, 768, T)
        tol(f"duration_emb_{n}_{T}", np.abs(got[:, ::cs].cpu().numpy().astype(np.float64) - g[f"emb_{n}_{T}"]).max(), 2e-4)
        assert torch.equal(bits(got), bits(x4[n][:, :, 4 * torch.from_numpy(R.uniform_map(n, T)).cuda()])), (n, T)
    # durations: np.repeat of the unexpanded (12, 12) embedding
    for k, d in enumerate(([0, 7, 0, 0, 1, 3, 3, 0, 9, 0, 1, 0], [4] * 12, [0] * 11 + [8])):
        T = sum(d)
        got = rt.diff_timestep_independent(lat[12], cond, frames=[T], durations=[d])
        want = np.repeat(g["emb_12_12"], d, axis=2)
        assert got.shape == (1, 768, T) and want.shape == (1, 768 // cs, T)
        tol(f"duration_emb_12_durations{k}", np.abs(got[:, ::cs].cpu().numpy().astype(np.float64) - want).max(), 2e-4)
        assert torch.equal(bits(got), bits(x4[12][:, :, 4 * torch.from_numpy(R.durations_map(d)).cuda()]))
    # one ragged batch of the three: rows against the fixture under the same gate, and against the BATCH's x4 columns bit for bit
    batch = torch.zeros((3, 768, 26), device="cuda")
    for b, n in enumerate((14, 26, 12)):
        batch[b, :, :n] = lat[n][0]
    ln, frames = [14, 26, 12], [92, 44, 148]
    x4b = rt.diff_timestep_independent(batch, cond.expand(3, -1).contiguous(), ln)
    got = rt.diff_timestep_independent(batch, cond.expand(3, -1).contiguous(), ln, frames=frames)
    assert got.shape == (3, 768, 148)
    for b, (n, T) in enumerate(zip(ln, frames)):
        tol(f"duration_emb_batch_{n}_{T}", np.abs(got[b, ::cs, :T].cpu().numpy().astype(np.float64) - g[f"emb_{n}_{T}"][0]).max(), 2e-4)
        assert torch.equal(bits(got[b, :, :T]), bits(x4b[b][:, 4 * torch.from_numpy(R.uniform_map(n, T)).cuda()]))
        assert not bool(got[b, :, T:].any())                          # beyond a row's frames: the caller's zeros
    # the DiffusionTts surface: any positive multiple of 4 with lengths=None is the uniform expansion, as the reference's
    emb = model.diffusion.timestep_independent(lat[14].permute(0, 2, 1), cond, 92)
    assert torch.equal(bits(emb), bits(rt.diff_timestep_independent(lat[14], cond, frames=[92])))
    with pytest.raises(ValueError, match="frames="):
        model.diffusion.timestep_independent(batch.permute(0, 2, 1), cond.expand(3, -1), 148, lengths=ln)
    with pytest.raises(ValueError):
        model.diffusion.timestep_independent(lat[14].permute(0, 2, 1), cond, 90)


# ------------------------------------------------------------------------------------------------------------ 3. frames = 4 n
def test_four_frames_per_code_is_the_old_entry_bit_for_bit(model, job):
    rt = model.rt
    rs = np.random.RandomState(5)
    lat, cond = dev(rs.randn(3, 768, 26)), dev(rs.randn(3, 1536) * 0.1)
    old = rt.diff_timestep_independent(lat, cond, list(N_CODES))
    new = rt.diff_timestep_independent(lat, cond, list(N_CODES), frames=[4 * n for n in N_CODES])
    dur = rt.diff_timestep_independent(lat, cond, list(N_CODES), frames=[4 * n for n in N_CODES], durations=[[4] * n for n in N_CODES])
    assert old.shape == new.shape == dur.shape == (3, 768, 104)
    assert torch.equal(bits(old), bits(new)) and torch.equal(bits(old), bits(dur)) and float(old.abs().max()) > 0.1
    # ... and through the model: speed = 1.0 is no plan at all
    plain, lens = model.infer(*job["args"], forced_codes=job["codes"], return_lengths=True, **job["kw"])
    same, lens1 = model.infer(*job["args"], forced_codes=job["codes"], return_lengths=True, speed=1.0, **job["kw"])
    assert lens == lens1 == [1024 * n for n in N_CODES]
    assert_rows_equal(same, plain, [4 * n for n in N_CODES])


# ------------------------------------------------------------------------------------------------------------ 4. speed
@pytest.mark.parametrize("speed", [0.6, 1.7])
def test_infer_with_speed_equals_the_manual_composition(model, job, speed):
    frames = [R.speed_frames(n, speed) for n in N_CODES]
    assert frames == {0.6: [92, 172, 40], 1.7: [32, 60, 16]}[speed]
    wav, lens = model.infer(*job["args"], forced_codes=job["codes"], return_lengths=True, speed=speed, **job["kw"])
    assert lens == [256 * T for T in frames]
    want, _ = compose(model, job, frames=frames)
    assert_rows_equal(wav, want, frames)
    per_row, lens = model.infer(*job["args"], forced_codes=job["codes"], return_lengths=True, speed=[speed] * 3, **job["kw"])
    assert lens == [256 * T for T in frames]
    assert_rows_equal(per_row, want, frames)


# ------------------------------------------------------------------------------------------------------------ 5. durations, span_rates
def test_infer_with_durations_and_span_rates_equals_the_manual_composition(model, job):
    rs = np.random.RandomState(9)
    durs = [rs.randint(0, 7, n) for n in N_CODES]
    durs[0][:2], durs[1][-3:], durs[2][2] = 0, 0, 0                   # leading, trailing and inner zeros
    padded = [R.pad_durations(d)[0] for d in durs]
    frames = [int(d.sum()) for d in padded]
    assert any(int(d.sum()) % 4 for d in durs) and all(f % 4 == 0 for f in frames)
    wav, lens = model.infer(*job["args"], forced_codes=job["codes"], return_lengths=True, durations=durs, **job["kw"])
    assert lens == [256 * T for T in frames]
    want, emb = compose(model, job, frames=frames, durations=padded)
    assert_rows_equal(wav, want, frames)
    # span_rates from a real alignment of a first call, as it hands the spans out (inclusive, disjoint): the first two spans of the
    # first row at half speed, the first span of the second row at double speed, the third row untouched
    _, al = model.infer(*job["args"], forced_codes=job["codes"], return_alignment=True, align_options=dict(space_id=2), **job["kw"])
    own = [[s for s in a["spans"] if s is not None] for a in al]
    spans = [[(a, b, 0.5) for a, b in own[0][:2]], [(own[1][0][0], own[1][0][1], 2.0)], []]
    assert spans[0] and al[2]["path"].size == N_CODES[2]
    durs = [R.span_durations(n, s) for n, s in zip(N_CODES, spans)]
    padded = [R.pad_durations(d)[0] for d in durs]
    frames = [int(d.sum()) for d in padded]
    assert frames[2] == 4 * N_CODES[2] and frames[0] > 4 * N_CODES[0] and int(durs[1].sum()) < 4 * N_CODES[1]
    wav, lens = model.infer(*job["args"], forced_codes=job["codes"], return_lengths=True, span_rates=spans, **job["kw"])
    assert lens == [256 * T for T in frames]
    want, _ = compose(model, job, frames=frames, durations=padded)
    assert_rows_equal(wav, want, frames)
    with pytest.raises(ValueError, match="forced_codes"):               # before any launch
        model.infer(*job["args"], span_rates=spans, **job["kw"])


# ------------------------------------------------------------------------------------------------------------ 6. infer_stream
def test_a_streamed_request_with_speed_equals_the_blocking_call(model, job):
    text, tl, refer, rl = job["args"]
    kw = dict(max_generate_length=7, suppress_eos=True, diffusion_steps=STEPS)
    speeds = [0.6, 1.7, 1.0]
    reqs = [dict(text=text, text_length=tl, refer=refer, refer_lengths=rl, seed=SEED, sample_ids=[3, 4, 9], speed=s) for s in (speeds, 1.7, None)]
    outs = list(model.infer_stream(iter(reqs), **kw))
    assert len(outs) == 3
    for r, (wav, lens) in zip(reqs, outs):
        s = r["speed"]
        frames = [R.speed_frames(6, v) for v in (s if isinstance(s, list) else [s or 1.0] * 3)]
        want, wlens = model.infer(text, tl, refer, rl, batch=True, seed=SEED, sample_ids=[3, 4, 9], return_lengths=True, speed=s, **kw)
        assert lens == wlens == [256 * T for T in frames]
        assert_rows_equal(wav, want, frames)
    assert outs[0][1] == [256 * 40, 256 * 16, 256 * 24]


# ------------------------------------------------------------------------------------------------------------ 7. infer_long
def test_infer_long_with_speed_equals_infer_on_its_groups(model):
    from detail_tts_amd import longform as L
    from longform_ref import join_plan
    rs = np.random.RandomState(31)
    sent, space, codes, speed = 250, 2, (7, 12, 6), 1.7
    text = np.concatenate([np.concatenate([rs.randint(3, 200, n), [sent, space]]) for n in (4, 6, 3)])[:-2]
    voice = model.get_conditioning_latents(torch.from_numpy((rs.randn(1, 128, 50) * 2 - 5).astype(np.float32)), [50])
    forced = [rs.randint(0, 8192, n) for n in codes]
    chunks = L.plan_chunks(text, sentence_ids=[sent], space_id=space)
    frames = [R.speed_frames(n, speed) for n in codes]
    wavs = []
    for req in L.plan_requests(chunks, 2, SEED, voice, forced):
        w, lens = model.infer(req["text"], req["text_length"], None, None, batch=True, speaker=voice, seed=SEED, sample_ids=req["sample_ids"],
                              forced_codes=req["forced_codes"], diffusion_steps=STEPS, speed=speed, return_lengths=True)
        wavs += [w[b, 0, :n].cpu().numpy().copy() for b, n in enumerate(lens)]
    assert [len(w) for w in wavs] == [256 * T for T in frames]
    pauses = {k: L.ms_to_samples(v, 24000) for k, v in L.PAUSES_MS.items()}
    want, offsets = join_plan(wavs, [len(w) for w in wavs], ["sentence", "sentence", "end"], pauses, fade=120)
    kw = dict(sentence_ids=[sent], space_id=space, seed=SEED, forced_codes=forced, diffusion_steps=STEPS, speaker=voice, rows_per_call=2,
              trim_db=None)
    got, info = model.infer_long(text, return_chunks=True, speed=speed, **kw)
    assert got.shape == (1, 1, len(want)) and got[0, 0].cpu().numpy().tobytes() == want.tobytes()
    assert [c["offset"] for c in info] == offsets and [c["frames"] for c in info] == frames and all(c["codes"] is None for c in info)
    plain, info = model.infer_long(text, return_chunks=True, speed=1.0, **kw)          # 1.0: the path and the dicts of before
    assert [c["codes"] for c in info] == list(codes) and all("frames" not in c for c in info)
    assert torch.equal(bits(plain), bits(model.infer_long(text, **kw)))
    with pytest.raises(ValueError):
        model.infer_long(text, speed=5.0, **kw)


# ------------------------------------------------------------------------------------------------------------ 8. alignment times
def test_alignment_times_follow_the_map(model, job):
    opts = dict(return_alignment=True, align_options=dict(space_id=2))
    _, plain = model.infer(*job["args"], forced_codes=job["codes"], **opts, **job["kw"])
    rs = np.random.RandomState(2)
    durs = [rs.randint(0, 6, n) for n in N_CODES]
    durs[0][3:6] = 0
    cases = [(dict(speed=[0.6, 1.7, 2.4]), [R.uniform_map(n, R.speed_frames(n, s)) for n, s in zip(N_CODES, (0.6, 1.7, 2.4))]),
             (dict(durations=durs), [R.durations_map(R.pad_durations(d)[0]) for d in durs])]
    for kw, maps in cases:
        _, lens, al = model.infer(*job["args"], forced_codes=job["codes"], return_lengths=True, **kw, **opts, **job["kw"])
        assert lens == [256 * len(m) for m in maps]
        for b, m in enumerate(maps):
            assert np.array_equal(al[b]["path"], plain[b]["path"]) and al[b]["spans"] == plain[b]["spans"]      # the codes' alignment is the same
            assert al[b]["times"] == [R.span_time(m, s) for s in al[b]["spans"]]
            assert al[b]["token_times"] == [R.span_time(m, s) for s in al[b]["token_spans"]]
            assert [w["time"] for w in al[b]["words"]] == [R.span_time(m, w["span"]) for w in al[b]["words"]]
            ends = [t[1] for t in al[b]["times"] if t is not None]
            assert max(ends) == len(m) * (256 / 24000)                # the last code's end is the row's length
