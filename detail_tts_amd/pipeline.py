"""The request pipeline under SynthesizerTrn.infer / infer_stream / infer_gpt (vqvae/model_24k.py), every stage written once.

Host bookkeeping (normalize_request, group_requests, merge_session, split_session: pure functions on lists and arrays, no device,
no library) and the stages' launch sequences (drain_session, stage_b, stage_c, stream_stage_a), which take the runtime / model they
launch on.  Nothing here synchronises beyond what a decode session's results need (gpt_finish, on stage A's stream)."""
from __future__ import annotations

import itertools
import time
from dataclasses import dataclass

import numpy as np
import torch

SESSION_ROWS = 16       # utterances one decode session holds
PAIR_ROWS = 8           # ... and the most a request may have to share one with its neighbour (infer_stream(pair_stage_a=True))


@dataclass
class Request:
    """one request batch: what the caller gave, normalised (host values; `refer` as given until stage A moves it to the device),
    then what stage A leaves for stages B and C"""
    B: int
    rl: list
    seed: int
    sids: list
    texts: list
    refer: object
    forced: object = None
    lat: object = None          # stage A: latents [B,768,max(n)], code counts n, the event stage B waits on
    n: list = None
    a_done: object = None
    tr: dict = None             # this request's entry of SynthesizerTrn.stream_trace
    voice: object = None        # the request's speaker as a Voice (voice.py) in the place of refer: S = 1 or B until stage A expands it
    rate: dict = None           # the request's speed / durations / span_rates, checked (duration.check_request); None: no frame plan
    plan: object = None         # stage B: the FramePlan it ran under (duration.py), None on the x4 path
    ready: object = None        # an event stage A's stream waits for before it reads the request's device tensors (None: they are complete)
    rows: list = None           # the request's per-row sampling records (gpt/sampling.py resolve_sampling); None: the uniform session


def normalize_request(text, text_length, refer, refer_lengths, seed=None, sample_ids=None, forced_codes=None, *, batch=True,
                      speaker=None, dims=None, speed=None, durations=None, span_rates=None):
    """the arguments of infer() / one request dict of infer_stream() -> Request: B, integer rl, a drawn seed when none is given,
    default sample ids range(B), per-row int32 text arrays cut at their own lengths.  batch=False keeps the first row only (the
    reference: text = text[0].unsqueeze(0) ..., vqvae/model_24k.py:775-778).  No device transfer: refer stays where it is.
    speaker: a Voice in the place of (refer, refer_lengths), which are then None (voice.check_speaker: ValueError otherwise, and on
    S not in {1, B} or widths other than the model's `dims`); the Request carries it as `voice`, refer = None and rl = zeros.
    speed / durations / span_rates: the speaking-rate keywords (duration.check_request: at most one, the last two with forced_codes;
    ValueError here, before any launch); the Request carries them as `rate`, None when they ask for nothing (speed None or 1.0)."""
    text = torch.as_tensor(text)
    tl = torch.as_tensor(text_length).reshape(-1).tolist()
    if speaker is not None or refer is None:
        from .voice import check_speaker
        check_speaker(speaker, refer, refer_lengths, text.shape[0] if batch else 1, dims)
        rl = [0] * text.shape[0]
    else:
        refer = torch.as_tensor(refer)
        rl = [int(v) for v in torch.as_tensor(refer_lengths).reshape(-1).tolist()]
    if not batch:
        text, refer, tl, rl = text[:1], None if refer is None else refer[:1], tl[:1], rl[:1]
        if forced_codes is not None:
            forced_codes = forced_codes[:1]
        durations = None if durations is None else durations[:1]
        span_rates = None if span_rates is None else span_rates[:1]
        if isinstance(speed, (list, tuple, np.ndarray)) or (hasattr(speed, "dim") and speed.dim() > 0):
            speed = speed[:1]
    B = text.shape[0]
    rate = None
    if speed is not None or durations is not None or span_rates is not None:
        from .duration import check_request
        rate = check_request(speed, durations, span_rates, forced_codes, B)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    sids = list(range(B)) if sample_ids is None else list(sample_ids)
    texts = [text[b, : int(tl[b])].cpu().numpy().astype(np.int32) for b in range(B)]
    return Request(B=B, rl=rl, seed=seed, sids=sids, texts=texts, refer=refer, forced=forced_codes, voice=speaker, rate=rate)


def group_requests(requests, pair=False):
    """requests -> stage-A groups (lists of one or two request dicts), reading at most two requests ahead of the group it yields.
    With `pair`, two consecutive requests of <= 8 utterances each share one decode session; every other request is alone."""
    it, held = iter(requests), []
    while True:
        held += itertools.islice(it, 2 - len(held))
        if not held:
            return
        nrows = [torch.as_tensor(r["text"]).shape[0] for r in held]
        take = 2 if pair and len(held) == 2 and nrows[0] <= PAIR_ROWS and nrows[1] <= PAIR_ROWS else 1
        yield [held.pop(0) for _ in range(take)]


def merge_session(sts):
    """the Requests of one decode session -> (rl, texts, sample ids, seeds, forced codes), rows concatenated in order; seeds is the
    request's own seed for one request, else one seed per row"""
    seeds = sts[0].seed if len(sts) == 1 else [st.seed for st in sts for _ in range(st.B)]
    forced = None
    if any(st.forced is not None for st in sts):
        assert all(st.forced is not None for st in sts), "forced_codes: all requests of a shared session or none"
        forced = [c for st in sts for c in st.forced]
    return [v for st in sts for v in st.rl], [t for st in sts for t in st.texts], [v for st in sts for v in st.sids], seeds, forced


def merge_rows(sts, samp):
    """the per-row sampling records of one decode session, the requests' rows concatenated in order -> None when no request of it
    carries any (the uniform session), else one record per row: a request without its own gets the call's settings written out.
    samp: dict(top_k, max_generate_length, decode_options) of the call (resolve_sampling's keywords)."""
    if all(st.rows is None for st in sts):
        return None
    from .gpt.sampling import resolve_sampling
    return [r for st in sts for r in (st.rows if st.rows is not None else resolve_sampling(None, st.B, always_rows=True, **samp))]


def split_session(ncodes, sizes, caps=None):
    """a session's code counts (stop token included) -> per request of `sizes` rows its n = ncodes - 1 (codes = codes[:, :-1],
    vqvae/model_24k.py:795).  caps: None or one cap per row (per-row max_generate_length): a row counts no code behind its own cap."""
    out, r0 = [], 0
    if caps is not None:
        ncodes = [min(int(c), int(k)) for c, k in zip(ncodes, caps)]
    for B in sizes:
        n = [int(c) - 1 for c in ncodes[r0:r0 + B]]
        if min(n) < 1:
            raise ValueError("an utterance produced no mel codes (stop token first)")
        out.append(n)
        r0 += B
    return out


def merge_refer(sts, dev):
    """the session's prompt batch: one request's own, or one zero-padded batch (every kernel takes the per-row length)"""
    if len(sts) == 1:
        return sts[0].refer
    refer = torch.zeros((sum(st.B for st in sts), sts[0].refer.shape[1], max(st.refer.shape[2] for st in sts)), device=dev, dtype=torch.float32)
    r0 = 0
    for st in sts:
        refer[r0:r0 + st.B, :, : st.refer.shape[2]] = st.refer
        r0 += st.B
    return refer


def merge_cond(rt, sts):
    """the session's conditioning latents [rows, 768] when a request of it carries a voice: its gpt member; a request that carries a
    prompt mel gets the conditioning encoder's own launch on its rectangle (no request carries a voice: None, and merge_refer serves)"""
    if all(st.voice is None for st in sts):
        return None
    conds = [st.voice.gpt if st.voice is not None else rt.mel_style("gpt.conditioning_encoder", st.refer, st.rl) for st in sts]
    return conds[0] if len(conds) == 1 else torch.cat(conds, 0).contiguous()


def split_latents(lat, sts, ns):
    """each request's rows of the session's decode-time latents (== the return_latent pass), cut at its longest utterance"""
    r0 = 0
    for st, n in zip(sts, ns):
        st.lat, st.n = lat[r0:r0 + st.B, :, : max(n)].contiguous(), n
        r0 += st.B


def drain_session(rt, max_generate_length, suppress_eos):
    """the decode session after its prefill: 16-token chunks, finish flags polled per chunk -> gpt_finish()'s (codes, ncodes, latents)"""
    while rt.gpt_steps() < max_generate_length:
        if not suppress_eos and rt.gpt_all_finished():
            break
        rt.gpt_decode(16)
    return rt.gpt_finish()


def stage_b(model, st, sampler_id, eta, prec, *, sched=None, sched_ts=None, mark=lambda name: None):
    """stage B of one request on the current stream (vqvae/model_24k.py:802-804) -> (mel, lens_t).  sched None: the schedule of
    `sched_ts` is looked up (built on first use) between the embedding and the sampling launches.  A request with a rate (speed /
    durations / span_rates) runs under its frame plan (duration.make_plan, kept as st.plan): the embedding through the plan's maps,
    lens_t the plan's frame counts; without one, the x4 launch and 4 frames per code."""
    rt = model.rt
    cond = st.voice.diffusion if st.voice is not None else rt.diff_conditioning(st.refer, st.rl)
    if st.rate is None:
        code_emb = rt.diff_timestep_independent(st.lat, cond, st.n)
        lens_t = [4 * v for v in st.n]
    else:
        from .duration import make_plan
        st.plan = make_plan(st.n, st.rate)
        code_emb = rt.diff_timestep_independent(st.lat, cond, st.n, frames=st.plan.frames, durations=st.plan.durations)
        lens_t = list(st.plan.frames)
    mark("diff_cond")
    if sched is None:
        sched = rt.sampler_schedule(sched_ts, sampler_id)
    with model._trunk_precision(prec):
        mel = rt.diff_sample_ex(code_emb, st.seed, st.sids, sched=sched, sampler=sampler_id, eta=eta, lens=lens_t, denorm=True)
    return mel, lens_t


def stage_c(rt, stream, home, mel, st, lens_t, noise_scale, chunk, *, wait=True, tr=None):
    """stage C of one request on `stream` (vqvae/model_24k.py:805-809) -> (wav, its completion event, its range-check ticket).
    `home` is the stream that made `mel` and reads the waveform; wait=False when mel is known complete (a re-run)."""
    if wait:
        ready = torch.cuda.Event()
        ready.record(home)
        if tr:
            tr["ev_b1"].record(home)
    with torch.cuda.stream(stream):
        if wait:
            stream.wait_event(ready)
        wav = rt.vocoder(mel, st.seed, st.sids, lens=lens_t, noise_scale=noise_scale, stream_chunk=int(chunk or 0))
        ticket = rt.vocoder_ticket()
        mel.record_stream(stream)
        done = torch.cuda.Event()
        done.record(stream)
        if tr:
            tr["ev_c1"].record(stream)
            tr["host_b1"] = time.perf_counter()
    wav.record_stream(home)
    return wav, done, ticket


def stream_stage_a(rt, sa, group, kw, token_wgs, trace=None, dims=None, samp=None):
    """infer_stream's stage A of one group on stream `sa` -> its Requests, with refer on the device and lat / n / a_done set.

    One request, or TWO requests of <= 8 utterances each as ONE decode session (<= 16 rows, per-row Philox seeds): the 308 MB of GPT
    weights stream once per token for both, and the chain of ~12 400 dependent launches is paid once.  A request of more than 16
    rows is decoded session after session (gpt_generate).  `kw`: the sampling arguments; next(token_wgs): a session's token-kernel width.
    samp: None, or dict(default, top_k, max_generate_length, decode_options): a request's `sampling` (else the stream's default) is
    resolved per request (gpt/sampling.py) and every row keeps its own settings, also next to another request's rows in one session."""
    dev = rt.device
    sts = [normalize_request(r["text"], r["text_length"], r.get("refer"), r.get("refer_lengths"), r.get("seed"), r.get("sample_ids"),
                             r.get("forced_codes"), speaker=r.get("speaker"), dims=dims, speed=r.get("speed"),
                             durations=r.get("durations"), span_rates=r.get("span_rates")) for r in group]
    caps = None
    if samp is not None:
        from .gpt.sampling import resolve_sampling, session_cap
        call = {k: v for k, v in samp.items() if k != "default"}
        for st, r in zip(sts, group):
            st.rows = resolve_sampling(samp["default"] if r.get("sampling") is None else r["sampling"], st.B, **call)
        rows = merge_rows(sts, call)
        if rows is not None:
            from .gpt.sampling import check_forced_caps
            r0 = 0
            for st in sts:          # (ValueError before any launch: a row cap below the row's forced codes)
                check_forced_caps(rows[r0:r0 + st.B], st.forced)
                r0 += st.B
            kw = dict(kw, rows=rows, max_generate_length=session_cap(rows, kw["max_generate_length"]))
            caps = [r["max_generate_length"] for r in rows]
    tr = None
    if trace is not None:
        tr = dict(host_a0=time.perf_counter(), ev_a0=torch.cuda.Event(enable_timing=True), ev_a1=torch.cuda.Event(enable_timing=True))
    with torch.cuda.stream(sa):
        if tr:
            tr["ev_a0"].record(sa)
        for st, r in zip(sts, group):
            st.ready = r.get("ready")
            if st.ready is not None:                       # the request's tensors were made on another stream: ordered before stage A
                sa.wait_event(st.ready)
                if st.voice is not None:
                    for _, t in st.voice.members():
                        t.record_stream(sa)
        for st in sts:
            if st.voice is not None:
                st.voice = st.voice.for_batch(st.B)
            else:
                st.refer = st.refer.to(dev, torch.float32).contiguous()
            if tr:
                st.tr = dict(tr, ev_b0=torch.cuda.Event(enable_timing=True), ev_b1=torch.cuda.Event(enable_timing=True),
                             ev_c1=torch.cuda.Event(enable_timing=True))
                trace.append(st.tr)
        session = sum(st.B for st in sts) <= SESSION_ROWS
        if session:
            rl, texts, sids, seeds, forced = merge_session(sts)
            cond = merge_cond(rt, sts)
            rt.gpt_prefill(merge_refer(sts, dev) if cond is None else None, rl, texts, seeds, sids, forced_codes=forced, **kw,
                           token_wgs=next(token_wgs), cond=cond)
            if kw["suppress_eos"]:                         # fixed length: the whole decode is enqueued without a host round trip
                rt.gpt_decode(kw["max_generate_length"])
        else:                                              # more than one decode session: group after group, on this thread / stream
            st = sts[0]
            _, ncodes, lat = rt.gpt_generate(st.refer, st.rl, st.texts, st.seed, st.sids, forced_codes=st.forced, **kw,
                                             cond=None if st.voice is None else st.voice.gpt)
        for st in sts:
            if st.tr:
                st.tr["host_a1"] = time.perf_counter()
        if session:
            _, ncodes, lat = drain_session(rt, kw["max_generate_length"], kw["suppress_eos"])      # waits for stream A only
        split_latents(lat, sts, split_session(ncodes, [st.B for st in sts], caps))
        done = torch.cuda.Event()
        done.record(sa)
        for st in sts:
            st.a_done = done
            if st.tr:
                st.tr["ev_a1"].record(sa)
                st.tr["host_a2"] = time.perf_counter()
    return sts
