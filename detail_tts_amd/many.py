"""SynthesizerTrn.infer_many: single utterances in, single waveforms out, batched in between.

A server holds single utterances, each with its own voice and its own sampling settings; the throughput of the machine is in the batch.
infer_many takes an iterable of utterance dicts, forms requests of `rows_per_call` consecutive utterances - each request carries
speaker = Voice.cat(the rows' voices), per-row `sampling`, the call's one seed and the utterances' sample ids - and sends them through
infer_stream AS IT IS (request i + 1 decodes under request i's diffusion).  Every row is then cut from the batch waveform at its own
returned length, and the results come back in input order.

This module is host bookkeeping only (lists, dicts, checks): every launch is infer_stream's or get_conditioning_latents'.

Batch-wide by construction: the diffusion schedule (diffusion_steps, sampler, eta), the trunk precision and noise_scale are one per
call.  Out of scope: reordering utterances by length, per-utterance seeds through stages B and C, cancellation."""
from __future__ import annotations

import collections

import numpy as np
import torch

from .voice import Voice

UTTERANCE_KEYS = ("text", "speaker", "refer", "refer_length", "sample_id", "sampling", "speed", "forced_codes")
ROWS_MAX = 16           # a decode session's rows (pipeline.SESSION_ROWS)


def check_rows_per_call(rows_per_call):
    if isinstance(rows_per_call, bool) or not isinstance(rows_per_call, (int, np.integer)) or not 1 <= int(rows_per_call) <= ROWS_MAX:
        raise ValueError(f"rows_per_call has to be an integer in 1 .. {ROWS_MAX}, but is {rows_per_call!r}")
    return int(rows_per_call)


def check_utterance(u, index, mel_channels=128):
    """one utterance dict -> (text ids int64 [n], sample id); ValueError naming the utterance and the key"""
    where = f"utterances[{index}]"
    if not hasattr(u, "items"):
        raise ValueError(f"{where}: an utterance has to be a dict, not {type(u).__name__}")
    for k in u:
        if k not in UTTERANCE_KEYS:
            raise ValueError(f"{where}: unknown key `{k}` (served: {', '.join(UTTERANCE_KEYS)})")
    if "text" not in u:
        raise ValueError(f"{where}: no `text`")
    text = torch.as_tensor(u["text"])
    if text.dim() != 1 or text.numel() < 1 or text.dtype.is_floating_point:
        raise ValueError(f"{where}: `text` has to be a 1-D array of at least one id, but is {tuple(text.shape)} {text.dtype}")
    sp, rf = u.get("speaker"), u.get("refer")
    if (sp is None) == (rf is None):
        raise ValueError(f"{where}: exactly one of `speaker` and `refer` names the voice")
    if sp is not None:
        if not isinstance(sp, Voice) or sp.S != 1:
            raise ValueError(f"{where}: `speaker` has to be a Voice of S = 1")
        if u.get("refer_length") is not None:
            raise ValueError(f"{where}: `refer_length` belongs to `refer`")
    else:
        shape = tuple(torch.as_tensor(rf).shape)
        if not (len(shape) == 2 and shape[0] == mel_channels) and not (len(shape) == 3 and shape[:2] == (1, mel_channels)):
            raise ValueError(f"{where}: `refer` has to be [{mel_channels}, Tr] or [1, {mel_channels}, Tr], but is {shape}")
        rl = u.get("refer_length")
        if rl is not None and not 1 <= int(rl) <= shape[-1]:
            raise ValueError(f"{where}: `refer_length` {rl} outside 1 .. {shape[-1]}")
    sid = u.get("sample_id", index)
    if isinstance(sid, bool) or not isinstance(sid, (int, np.integer)) or sid < 0:
        raise ValueError(f"{where}: `sample_id` has to be an integer >= 0, but is {sid!r}")
    s = u.get("sampling")
    if s is not None and not hasattr(s, "items"):
        raise ValueError(f"{where}: `sampling` has to be a dict (one utterance is one row)")
    fc = u.get("forced_codes")
    if fc is not None and np.asarray(fc).ndim != 1:
        raise ValueError(f"{where}: `forced_codes` has to be 1-D")
    return text.to(torch.int64), int(sid)


def group_request(model, group, first, seed, sampling, voices, resolve, side=None):
    """`group`: consecutive utterances (index first ..) -> one request dict of infer_stream.  Everything is checked here, for all of
    the group's utterances, before the request is handed on.  voices: the call's cache {id(prompt tensor): (tensor, length, Voice,
    event)}.

    Stream order.  This runs on the caller's thread between two requests' stage B / C launches, and stage A reads the request's voice
    on a stream of its own, so the request carries an event (`ready`) that stage A waits for.  A prompt mel's encoders have to run
    on the caller's stream (they use the scratch arena the diffusion uses) - once per distinct tensor, behind whatever that stream
    holds; its event is kept with the voice.  The join (Voice.cat, a plain copy) runs on the side stream `side`, behind the events
    of the voices it reads and NOT behind the previous request's diffusion, so stage A of request i + 1 still starts under stage B
    of request i.  A `speaker` handed in gets an event on the caller's stream the first time it is seen (it may have been made a
    moment ago), which every later request reuses.  side None (no device): no events."""
    texts, sids, speakers, samp, speeds, forced = [], [], [], [], [], []
    for k, u in enumerate(group):
        text, sid = check_utterance(u, first + k)
        texts.append(text)
        sids.append(sid)
        samp.append(u.get("sampling", sampling))
        speeds.append(u.get("speed"))
        forced.append(u.get("forced_codes"))
    if len(set(sids)) != len(sids):
        raise ValueError(f"utterances[{first}..{first + len(group) - 1}]: two rows of one request share sample id(s) {sids}")
    if any(f is not None for f in forced) and any(f is None for f in forced):
        raise ValueError(f"utterances[{first}..{first + len(group) - 1}]: `forced_codes` on some rows of one request only (all rows of a "
                         "request, or none)")
    resolve(samp, len(group), first)                                  # (ValueError naming the row and the key)
    events = []
    for u in group:                                                   # voices last: the only step that launches anything
        if u.get("speaker") is not None:
            sp = u["speaker"]
            speakers.append(sp)
            if side is not None:        # a Voice seen for the first time may still be pending on the caller's stream: its event is
                hit = voices.get(id(sp))                          # taken once, there, and serves every later request (complete by then)
                if hit is None or hit[0] is not sp:
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(side.device))
                    hit = voices[id(sp)] = (sp, None, sp, ev)
                if hit[3] not in events:
                    events.append(hit[3])
            continue
        rf, rl = u["refer"], u.get("refer_length")
        hit = voices.get(id(rf))
        if hit is None or hit[0] is not rf or hit[1] != rl:
            t = torch.as_tensor(rf)
            t = t[None] if t.dim() == 2 else t
            v = model.get_conditioning_latents(t, None if rl is None else [int(rl)])
            ev = None
            if side is not None:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(side.device))
            hit = (rf, rl, v, ev)
            voices[id(rf)] = hit
        speakers.append(hit[2])
        if hit[3] is not None and hit[3] not in events:
            events.append(hit[3])
    lt = max(int(t.numel()) for t in texts)
    text = torch.zeros((len(group), lt), dtype=torch.int64)
    for b, t in enumerate(texts):
        text[b, : t.numel()] = t
    if side is None:
        speaker, ready = Voice.cat(speakers), None
    else:
        with torch.cuda.stream(side):
            for ev in events:
                side.wait_event(ev)
            speaker = Voice.cat(speakers)
            ready = torch.cuda.Event()
            ready.record(side)
    req = dict(text=text, text_length=[int(t.numel()) for t in texts], speaker=speaker, seed=seed, sample_ids=sids)
    if ready is not None:
        req["ready"] = ready
    if any(s is not None for s in samp):
        req["sampling"] = samp
    if any(s is not None for s in speeds):
        req["speed"] = [1.0 if s is None else s for s in speeds]
    if forced[0] is not None:
        req["forced_codes"] = [np.asarray(f) for f in forced]
    return req


def infer_many(model, utterances, *, rows_per_call=8, seed=None, sampling=None, noise_scale=None, **stream_kw):
    """see SynthesizerTrn.infer_many.  Call-level checks run here, before anything starts; the generator it returns reads the
    utterances lazily (at most two requests ahead of the one being handed out, as infer_stream reads its requests)."""
    from .gpt.decode_options import beam_request
    from .gpt.sampling import resolve_sampling
    rows_per_call = check_rows_per_call(rows_per_call)
    if sampling is not None and not hasattr(sampling, "items"):
        raise ValueError("infer_many: the call's `sampling` has to be None or a dict (an utterance carries its own)")
    processors, _ = beam_request(stream_kw.get("decode_options"), stream=True)
    call = dict(top_k=stream_kw.get("top_k", 50), decode_options=processors)
    if "max_generate_length" in stream_kw:
        call["max_generate_length"] = stream_kw["max_generate_length"]
    else:
        from .config import MAX_GENERATE_LENGTH
        call["max_generate_length"] = MAX_GENERATE_LENGTH
    resolve_sampling(sampling, 1, **call)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())          # ONE seed for the call, drawn once
    if noise_scale is not None:
        stream_kw["noise_scale"] = noise_scale

    def resolve(samp, B, first):
        try:
            resolve_sampling(samp, B, **call)
        except ValueError as e:
            raise ValueError(f"utterances[{first}..{first + B - 1}]: {e}") from None

    def run():
        sizes, voices = collections.deque(), {}
        dev = getattr(model, "device", None)
        side = torch.cuda.Stream(dev) if dev is not None and torch.device(dev).type == "cuda" else None

        def requests():
            it, first = iter(utterances), 0
            while True:
                group = []
                for u in it:
                    group.append(u)
                    if len(group) == rows_per_call:
                        break
                if not group:
                    return
                req = group_request(model, group, first, seed, sampling, voices, resolve, side)
                sizes.append(len(group))
                first += len(group)
                yield req

        for wav, lens in model.infer_stream(requests(), **stream_kw):
            B = sizes.popleft()
            for b in range(B):
                n = int(lens[b])
                yield wav[b:b + 1, :, :n], n

    return run()
