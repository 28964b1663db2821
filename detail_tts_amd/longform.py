"""Long texts: split into chunks, synthesise the chunks as rows of request batches, join their waveforms on the device.

A row of infer / infer_stream is one utterance, bounded by the GPT (max_generate_length codes, gpt.max_text_tokens ids).  infer_long
(vqvae/model_24k.py; the logic is here) cuts a text at sentence ends, feeds the chunks through infer_stream AS IT IS - a chunk is a
complete utterance through the stages exactly as they are - and lays each group's waveforms end to end with the two kernels of
csrc/wav_join.hip: the loud span of every row (Runtime.wav_edges), then the spans with a pause behind each (Runtime.wav_join).

Host side, pure (no device, no library): split_units, frame_chunk, plan_chunks, plan_requests, plan_join and the argument checks of
the two kernels.  run() drives a model.  The defaults (max_len, pauses, trim threshold, kept margin, fade) are the maintainer's choice:
their effect on audio is UNMEASURED - there is no trained checkpoint - and so is the number of codes a chunk of max_len units needs."""
from __future__ import annotations

import math

import numpy as np

SENTENCE_END = "。！？!?."
CLAUSE_END = "，,；;、：:"
SPACE = " "
KINDS = ("sentence", "clause", "word", "hard", "end")
PAUSES_MS = {"sentence": 400, "clause": 200, "word": 60, "hard": 0}
JOIN_ROWS = 16          # rows one wav_join launch takes
FRAME = 256             # samples per energy frame of the trim


# ---------------------------------------------------------------------------------------------------------------- the splitter
def split_units(seq, *, sentence_end, clause_end=(), space=(), max_len, min_len=0):
    """One greedy splitter over a sequence of units (the characters of a string, or ids) -> [(start, stop, kind)], contiguous spans that
    cover `seq` exactly.  In this order:

    * a cut falls after a run of sentence-end units; the run and the spaces behind it stay with the left chunk ("sentence");
    * a sentence shorter than `min_len` is merged into its right neighbour (the last one into its left), never beyond `max_len`;
    * a sentence longer than `max_len` is cut again: after the last clause unit at or before `max_len` ("clause", the spaces behind
      it kept while they fit), else after the last space ("word"), else at `max_len` ("hard");
    * the last chunk has kind "end".

    A chunk always holds a unit that is none of the three sets: a span of spaces and punctuation alone is attached to a neighbour
    (a cut that would leave one is not taken).  An empty or all-blank `seq` is a ValueError, and so is a run of spaces and punctuation
    too long for any cut to keep every chunk within `max_len`."""
    units = list(seq) if isinstance(seq, str) else [int(u) for u in np.asarray(seq).reshape(-1)]
    as_set = lambda s: set(s) if isinstance(s, str) else {int(u) for u in s}
    sent, clause, blank = as_set(sentence_end), as_set(clause_end), as_set(space)
    max_len, min_len = int(max_len), int(min_len)
    if max_len < 1 or not 0 <= min_len <= max_len:
        raise ValueError(f"split_units: max_len has to be >= 1 and min_len in 0 .. max_len, but they are {max_len} and {min_len}")
    n = len(units)
    content = np.zeros(n + 1, np.int64)          # content[i]: units before i that are neither a space nor a mark
    for i, u in enumerate(units):
        content[i + 1] = content[i] + (u not in sent and u not in clause and u not in blank)
    has = lambda a, b: content[b] > content[a]
    if not has(0, n):
        raise ValueError("split_units: the text is empty or holds only spaces and punctuation")
    # 1. sentences
    pieces, start, i = [], 0, 0
    while i < n:
        if units[i] in sent:
            while i < n and units[i] in sent:
                i += 1
            while i < n and units[i] in blank:
                i += 1
            pieces.append([start, i])
            start = i
        else:
            i += 1
    if start < n:
        pieces.append([start, n])
    merged = []                                   # a piece without content joins its left neighbour, the first one its right
    for p in pieces:
        if merged and (not has(*p) or not has(*merged[-1])):
            merged[-1][1] = p[1]
        else:
            merged.append(p)
    # 2. short sentences
    pieces, i = [], 0
    while i < len(merged):
        a, b = merged[i]
        i += 1
        while b - a < min_len and i < len(merged) and merged[i][1] - a <= max_len:
            b = merged[i][1]
            i += 1
        pieces.append([a, b])
    if len(pieces) > 1 and pieces[-1][1] - pieces[-1][0] < min_len and pieces[-1][1] - pieces[-2][0] <= max_len:
        last = pieces.pop()
        pieces[-1][1] = last[1]
    # 3. long sentences
    out = []
    for a, b in pieces:
        pos = a
        while b - pos > max_len:
            lim, cut, kind = pos + max_len, None, None
            ok = lambda c: has(pos, c) and has(c, b)
            for c in range(lim, pos, -1):
                if units[c - 1] in clause and ok(c):
                    cut, kind = c, "clause"
                    while cut < lim and units[cut] in blank and ok(cut + 1):
                        cut += 1
                    break
            if cut is None:
                cut = next((c for c in range(lim, pos, -1) if units[c - 1] in blank and ok(c)), None)
                kind = "word"
            if cut is None:
                cut = next((c for c in range(lim, pos, -1) if ok(c)), None)
                kind = "hard"
            if cut is None:
                raise ValueError(f"split_units: units {pos} .. {b} hold a run of spaces and punctuation longer than max_len = {max_len} allows")
            out.append((pos, cut, kind))
            pos = cut
        out.append((pos, b, "sentence"))
    out[-1] = (out[-1][0], out[-1][1], "end")
    return out


def frame_chunk(seq, start, stop, *, tokenizer=None, space=SPACE, space_id=None):
    """the ids of chunk seq[start:stop] as the reference frames a whole text (api.py:22-25): edge spaces stripped, then
    " " + chunk + " " -> tokenizer.encode -> one trailing 0 for a string; [space_id] + ids + [space_id, 0] for ids, or ids + [0]
    with space_id = None -> int32 array"""
    if isinstance(seq, str):
        if tokenizer is None:
            raise ValueError("a text given as a string needs `tokenizer` (an object with .encode)")
        body = seq[start:stop].strip(space if isinstance(space, str) else "".join(space))
        return np.asarray(list(tokenizer.encode(" " + body + " ")) + [0], np.int32)
    ids = [int(u) for u in np.asarray(seq).reshape(-1)[start:stop]]
    if space_id is not None:
        while ids and ids[0] == space_id:
            ids.pop(0)
        while ids and ids[-1] == space_id:
            ids.pop()
        ids = [int(space_id)] + ids + [int(space_id)]
    return np.asarray(ids + [0], np.int32)


def plan_chunks(text, *, tokenizer=None, sentence_ids=None, clause_ids=(), space_id=None, max_len=160, min_len=0, max_text_tokens=800):
    """text (a pinyin string, or a 1-D array of text ids) -> [dict(span, kind, ids)], one per chunk, in order.  A string is split at
    the default marks and needs `tokenizer`; ids need `sentence_ids` (whether a BPE vocabulary keeps punctuation as tokens of its own
    is the vocabulary's business).  A framed chunk of more than `max_text_tokens` ids is a ValueError that names its span."""
    if isinstance(text, str):
        if tokenizer is None:
            raise ValueError("a text given as a string needs `tokenizer` (an object with .encode)")
        spans = split_units(text, sentence_end=SENTENCE_END, clause_end=CLAUSE_END, space=SPACE, max_len=max_len, min_len=min_len)
    else:
        text = np.asarray(text)
        if text.ndim != 1 or text.dtype.kind not in "iu":
            raise ValueError(f"a text given as ids has to be a 1-D integer array, but is {text.dtype} {text.shape}")
        if sentence_ids is None:
            raise ValueError("a text given as ids needs `sentence_ids` (the ids that end a sentence)")
        spans = split_units(text, sentence_end=sentence_ids, clause_end=clause_ids, space=() if space_id is None else (space_id,),
                            max_len=max_len, min_len=min_len)
    chunks = []
    for a, b, kind in spans:
        ids = frame_chunk(text, a, b, tokenizer=tokenizer, space_id=space_id)
        if len(ids) > max_text_tokens:
            raise ValueError(f"the chunk at {a} .. {b} of the text frames to {len(ids)} ids, more than gpt.max_text_tokens = {max_text_tokens}: "
                             f"lower max_len")
        chunks.append(dict(span=(a, b), kind=kind, ids=ids))
    return chunks


# ---------------------------------------------------------------------------------------------------------------- requests
def check_rows_per_call(rows_per_call):
    if isinstance(rows_per_call, bool) or int(rows_per_call) != rows_per_call or not 1 <= int(rows_per_call) <= JOIN_ROWS:
        raise ValueError(f"rows_per_call has to be an integer in 1 .. {JOIN_ROWS}, but is {rows_per_call!r}")
    return int(rows_per_call)


def check_pauses(pauses_ms):
    """-> {kind: ms}; a key for every kind a chunk that is not the last can have"""
    missing = [k for k in KINDS[:-1] if k not in pauses_ms]
    if missing:
        raise ValueError(f"pauses_ms has no entry for {missing}: it needs one for each of {list(KINDS[:-1])}")
    out = {k: float(pauses_ms[k]) for k in KINDS[:-1]}
    if any(not (math.isfinite(v) and v >= 0) for v in out.values()):
        raise ValueError(f"pauses_ms has to hold finite values >= 0, but is {pauses_ms}")
    return out


def check_forced(forced_codes, nchunks):
    if forced_codes is None:
        return None
    forced = [np.asarray(c).reshape(-1) for c in forced_codes]
    if len(forced) != nchunks:
        raise ValueError(f"forced_codes holds {len(forced)} code arrays, the text splits into {nchunks} chunks: one array per chunk")
    if any(len(c) < 1 for c in forced):
        raise ValueError("forced_codes: every chunk needs at least one code")
    return forced


def plan_requests(chunks, rows_per_call, seed, speaker, forced_codes=None, speed=None):
    """chunk k is row k % rows_per_call of request k // rows_per_call, with sample id k - its random streams do not depend on
    rows_per_call - and every request carries the call's one seed -> the request dicts of infer_stream"""
    import torch
    reqs = []
    for r0 in range(0, len(chunks), rows_per_call):
        rows = chunks[r0: r0 + rows_per_call]
        lt = max(len(c["ids"]) for c in rows)
        text = np.zeros((len(rows), lt), np.int64)
        for b, c in enumerate(rows):
            text[b, : len(c["ids"])] = c["ids"]
        req = dict(text=torch.from_numpy(text), text_length=[len(c["ids"]) for c in rows], speaker=speaker, seed=seed,
                   sample_ids=list(range(r0, r0 + len(rows))))
        if forced_codes is not None:
            req["forced_codes"] = forced_codes[r0: r0 + len(rows)]
        if speed is not None:
            req["speed"] = speed
        reqs.append(req)
    return reqs


# ---------------------------------------------------------------------------------------------------------------- the join
def ms_to_samples(ms, sample_rate):
    return int(round(float(ms) * sample_rate / 1000.0))


def plan_join(kinds, edges, pauses, base=0):
    """One group's layout.  kinds [B]; edges [B][2] = every row's (begin, end); pauses {kind: samples}; base = the group's first
    sample in the whole output -> (begins, counts, offsets inside the piece, the piece's sample count, per-row dicts with begin, end,
    offset in the WHOLE output and pause).  A chunk's pause follows it; the text's last chunk (kind "end") has none.  A chunk trimmed
    to nothing contributes no samples and keeps its pause."""
    begins, counts, offsets, rows, at = [], [], [], [], 0
    for kind, (b, e) in zip(kinds, edges):
        b, e = int(b), int(e)
        if not 0 <= b <= e:
            raise ValueError(f"plan_join: edges ({b}, {e})")
        pause = 0 if kind == "end" else int(pauses[kind])
        begins.append(b); counts.append(e - b); offsets.append(at)
        rows.append(dict(begin=b, end=e, offset=base + at, pause=pause))
        at += e - b + pause
    return begins, counts, offsets, at, rows


def _int_rows(a, B, name):
    arr = np.asarray(a)
    if arr.shape != (B,) or arr.dtype.kind not in "iu" or (arr.size and (arr.min() < 0 or arr.max() >= 2 ** 31)):
        raise ValueError(f"{name} has to hold B = {B} integers in 0 .. 2**31 - 1, but is {a!r}")
    return np.ascontiguousarray(arr, np.int32)


def check_edges(lens, B, stride, frame, threshold, keep):
    """the arguments of Runtime.wav_edges -> (lens int32 [B], frame, threshold, keep); ValueError before the launch"""
    lens = _int_rows(lens, B, "wav_edges: lens")
    if lens.size and lens.max() > stride:
        raise ValueError(f"wav_edges: lens {lens.tolist()} reach beyond the rows' stride {stride}")
    frame, keep, threshold = int(frame), int(keep), float(threshold)
    if frame < 1 or keep < 0 or not (math.isfinite(threshold) and 0 <= threshold < 1e15):
        raise ValueError(f"wav_edges: frame >= 1, keep >= 0 and a finite threshold >= 0 are needed, not {frame}, {keep}, {threshold}")
    return lens, frame, threshold, keep


def check_join(begins, counts, offsets, total, fade, B, stride):
    """the arguments of Runtime.wav_join -> (begins, counts, offsets int32 [B], total, fade); ValueError before the launch"""
    if not 1 <= B <= JOIN_ROWS:
        raise ValueError(f"wav_join: B = {B} rows, one launch takes 1 .. {JOIN_ROWS}")
    begins, counts, offsets = (_int_rows(a, B, "wav_join: " + n) for a, n in ((begins, "begins"), (counts, "counts"), (offsets, "offsets")))
    total, fade = int(total), int(fade)
    if not 0 <= total < 2 ** 31:
        raise ValueError(f"wav_join: total = {total} is not in 0 .. 2**31 - 1")
    if not 0 <= fade <= 2 ** 23:
        raise ValueError(f"wav_join: fade = {fade} is not in 0 .. 2**23")
    at = 0
    for b in range(B):
        if int(begins[b]) + int(counts[b]) > stride:
            raise ValueError(f"wav_join: row {b} reads {int(begins[b])} + {int(counts[b])} samples of a row of {stride}")
        if int(offsets[b]) < at:
            raise ValueError(f"wav_join: the span of row {b} starts at {int(offsets[b])}, before the end {at} of the row in front of it: "
                             f"the spans have to be ascending and disjoint")
        at = int(offsets[b]) + int(counts[b])
    if at > total:
        raise ValueError(f"wav_join: the last span ends at {at}, beyond total = {total}")
    return begins, counts, offsets, total, fade


# ---------------------------------------------------------------------------------------------------------------- the driver
def prepare(model, text, refer=None, refer_lengths=None, *, speaker=None, tokenizer=None, sentence_ids=None, clause_ids=(),
            space_id=None, max_len=160, min_len=0, rows_per_call=8, seed=None, pauses_ms=None, trim_db=-40.0, keep_ms=20, fade_ms=5,
            forced_codes=None, decode_options=None, speed=None):
    """every check and all the planning of infer_long, before anything runs on the device but the prompt's encoders (once) ->
    dict(chunks, requests, pauses, threshold, keep, fade)"""
    import torch
    from .gpt.decode_options import beam_request
    if (speaker is None) == (refer is None and refer_lengths is None):
        raise ValueError("give the speaker as a Voice (`speaker`) or as a prompt mel (`refer`, `refer_lengths`): " +
                         ("neither is given" if speaker is None else "both given"))
    rows_per_call = check_rows_per_call(rows_per_call)
    pauses_ms = check_pauses(PAUSES_MS if pauses_ms is None else pauses_ms)
    beam_request(decode_options, stream=True)                # beams are refused as infer_stream refuses them
    if speed is not None:                                     # one rate for all chunks (duration.py); 1.0 is no plan at all
        from .duration import check_speed
        if isinstance(speed, (list, tuple, np.ndarray)):
            raise ValueError("infer_long takes ONE speed for all chunks")
        speed = None if check_speed(speed, 1) is None else float(speed)
    if trim_db is not None and not (math.isfinite(float(trim_db)) and float(trim_db) <= 0):
        raise ValueError(f"trim_db has to be None (no trimming) or a level <= 0 dB relative to full scale, but is {trim_db}")
    if not (math.isfinite(float(keep_ms)) and keep_ms >= 0 and math.isfinite(float(fade_ms)) and fade_ms >= 0):
        raise ValueError(f"keep_ms and fade_ms have to be finite and >= 0, but are {keep_ms} and {fade_ms}")
    cfg = model.cfg
    chunks = plan_chunks(text, tokenizer=tokenizer, sentence_ids=sentence_ids, clause_ids=clause_ids, space_id=space_id, max_len=max_len,
                         min_len=min_len, max_text_tokens=cfg["gpt"]["max_text_tokens"])
    forced = check_forced(forced_codes, len(chunks))
    if speaker is None:
        refer = torch.as_tensor(refer)
        if refer.dim() != 3 or refer.shape[0] != 1:
            raise ValueError(f"infer_long speaks with ONE voice: the prompt mel has to be [1, 128, Tr], but is {tuple(refer.shape)}")
    else:
        from .voice import Voice
        if not isinstance(speaker, Voice):
            raise ValueError(f"`speaker` has to be a Voice (get_conditioning_latents), but is {type(speaker).__name__}")
        if speaker.S != 1:
            raise ValueError(f"infer_long speaks with ONE voice: S has to be 1, but is {speaker.S}")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    if speaker is None:                                       # the prompt's latents, once: no prompt encoder runs per group
        speaker = model.get_conditioning_latents(refer, refer_lengths)
    sr = cfg["data"]["sampling_rate"]
    return dict(chunks=chunks, requests=plan_requests(chunks, rows_per_call, int(seed), speaker, forced, speed), speed=speed,
                pauses={k: ms_to_samples(v, sr) for k, v in pauses_ms.items()},
                threshold=None if trim_db is None else 10.0 ** (float(trim_db) / 20.0),
                keep=ms_to_samples(keep_ms, sr), fade=ms_to_samples(fade_ms, sr))


def join_group(model, wav, lens, kinds, plan, base=0, complete=True):
    """one group's waveform batch -> (its piece, cuda [n], the per-row dicts of plan_join + samples).  The kernels run on a stream of
    their own - the calling stream already holds the next group's diffusion, and the first audio is due after the first group -
    which the calling stream then waits on.  complete: infer_stream waited for the waveform; False (a blocking infer's result, the
    last work on the calling stream): the join stream waits for the calling stream first.  The read-back of the edges is the only
    host wait; without trimming there is none."""
    import torch
    rt, cur = model.rt, torch.cuda.current_stream(model.device)
    if getattr(model, "_join_stream", None) is None:
        model._join_stream = torch.cuda.Stream(model.device)
    if not complete:
        ready = torch.cuda.Event()
        ready.record(cur)
        model._join_stream.wait_event(ready)
    with torch.cuda.stream(model._join_stream):
        wav.record_stream(model._join_stream)
        if plan["threshold"] is None:
            edges = [(0, int(n)) for n in lens]
        else:
            edges = rt.wav_edges(wav, lens, frame=FRAME, threshold=plan["threshold"], keep=plan["keep"])
        begins, counts, offsets, total, rows = plan_join(kinds, edges, plan["pauses"], base)
        piece = rt.wav_join(wav, begins, counts, offsets, total, fade=plan["fade"])
        done = torch.cuda.Event()
        done.record(model._join_stream)
    cur.wait_event(done)                                     # the caller reads the piece on its own stream
    piece.record_stream(cur)
    for row, n in zip(rows, lens):
        row["samples"] = int(n)
    return piece, rows


def group_waveforms(model, plan, stream_kw, pipelined=True):
    """the plan's requests -> (wav [B,1,1024 n_max], lengths) per group.  pipelined: through
    model.infer_stream as it is.  Otherwise a loop of blocking model.infer(batch=True) calls on the same requests - what a request with
    forced codes takes: infer_stream feeds forced codes through the KV-cache decode, whose latents differ in the last bits from the
    teacher-forced pass infer() runs on them (2e-8 on waveforms of rms 6e-3 under the synthetic weights), and infer() is the yardstick;
    no decode runs on forced codes, so there is nothing for the next group to overlap."""
    if pipelined:
        yield from model.infer_stream(iter(plan["requests"]), **stream_kw)
        return
    kw = dict(stream_kw)
    noise_scale = kw.pop("noise_scale")
    for r in plan["requests"]:
        rate = {} if r.get("speed") is None else dict(speed=r["speed"])
        yield model.infer(r["text"], r["text_length"], None, None, noise_scale, batch=True, speaker=r["speaker"], seed=r["seed"],
                          sample_ids=r["sample_ids"], forced_codes=r.get("forced_codes"), return_lengths=True, **rate, **kw)


def run(model, plan, stream_kw, pipelined=True):
    """the generator under infer_long: every group's waveform (group_waveforms) joined (model.join_group) as it is handed out ->
    (piece [1, 1, n], its chunks' dicts)"""
    chunks, base, k = plan["chunks"], 0, 0
    for wav, lens in group_waveforms(model, plan, stream_kw, pipelined):
        rows = chunks[k: k + len(lens)]
        piece, infos = model.join_group(wav, lens, [c["kind"] for c in rows], plan, base, complete=pipelined)
        for c, info in zip(rows, infos):
            info.update(span=c["span"], kind=c["kind"], codes=info["samples"] // 1024)
            if plan.get("speed") is not None:             # under a rate the samples no longer count the codes
                info.update(codes=None, frames=info["samples"] // 256)
        base += piece.numel()
        k += len(lens)
        yield piece.view(1, 1, -1), infos
