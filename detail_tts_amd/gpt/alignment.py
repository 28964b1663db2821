"""What is made of a text-to-audio alignment path, on the host (pure functions on lists and arrays: no device, no library).

The device side (Runtime.gpt_text_alignment, Runtime.op_monotone_path) gives, per utterance, `path`: for each of its n mel codes the
text COLUMN it sits on.  Columns are those of the GPT's text span [255, text ..., 0]: column 0 is the start-text token, column 1 + k
the caller's text id k (a trailing 0 the caller passes included), the last column the stop-text token, tl = len(text) + 2 in all.
The path is monotone (it never goes back) but free otherwise: it may stay on a column, jump ahead, and need not reach the last one.
Code j covers waveform samples [samples_per_code * j, samples_per_code * (j + 1)).

Alignment QUALITY is unmeasured: no trained checkpoint is at hand, and which layers and heads carry the alignment is the caller's
knowledge (`layers` / `head_weights` of SynthesizerTrn.align)."""
from __future__ import annotations

import numpy as np


def spans_from_path(path, n, tl):
    """path (ints, at least n of them) -> a list of tl entries, per text column (first, last) code index (inclusive) or None for a
    column that owns no code.  ValueError on a path that leaves [0, tl) or goes back."""
    n, tl = int(n), int(tl)
    p = np.asarray(path, np.int64).reshape(-1)[:n]
    if p.size != n:
        raise ValueError(f"the path holds {p.size} codes, not {n}")
    spans = [None] * tl
    if n == 0:
        return spans
    if p.min() < 0 or p.max() >= tl or (np.diff(p) < 0).any():
        raise ValueError("the path has to be monotone and inside [0, tl)")
    for j, c in enumerate(p.tolist()):
        spans[c] = (j, j) if spans[c] is None else (spans[c][0], j)
    return spans


def token_times(spans, samples_per_code, sampling_rate):
    """spans -> per entry (start, end) in seconds, or None: code j covers samples [samples_per_code j, samples_per_code (j + 1))"""
    k = float(samples_per_code) / float(sampling_rate)
    return [None if s is None else (s[0] * k, (s[1] + 1) * k) for s in spans]


def token_times_frames(spans, bounds, samples_per_frame, sampling_rate):
    """token_times under a frame plan (duration.py: speed / durations / span_rates): code j covers mel frames
    [bounds[j], bounds[j + 1]) - bounds[j] the first frame whose code is >= j - each frame samples_per_frame samples; a span whose codes
    own no frame gets an empty interval (start == end)"""
    k = float(samples_per_frame) / float(sampling_rate)
    return [None if s is None else (int(bounds[s[0]]) * k, int(bounds[s[1] + 1]) * k) for s in spans]


def group_words(ids, spans, space_id):
    """The caller's text ids and THEIR spans (spans_from_path(...)[1:1 + len(ids)]) -> a list of words: the runs of tokens between
    `space_id` ids, each dict(tokens=[indices into ids], span=(first, last) over its tokens that own a code, or None).  The space
    tokens themselves belong to no word; empty runs (two spaces in a row, a leading space) give no word."""
    ids = [int(v) for v in np.asarray(ids).reshape(-1)]
    if len(spans) != len(ids):
        raise ValueError(f"{len(spans)} spans for {len(ids)} text ids")
    words, cur = [], []

    def close():
        if cur:
            own = [spans[k] for k in cur if spans[k] is not None]
            words.append(dict(tokens=list(cur), span=(min(s[0] for s in own), max(s[1] for s in own)) if own else None))
            cur.clear()

    for k, v in enumerate(ids):
        if v == int(space_id):
            close()
        else:
            cur.append(k)
    close()
    return words


def alignment_stats(path, n, n_text, text_mass=None):
    """Health figures of one utterance's alignment, for noticing a decode that skipped or repeated text:
    coverage (share of the caller's n_text text tokens - columns 1 .. n_text - that own at least one code; 1.0 for an empty text),
    skipped (their indices into the caller's ids), longest_stay (the longest run of codes on one column, any column), mean_text_mass
    (the mean over codes of the attention mass on the text span; None without text_mass)."""
    n, n_text = int(n), int(n_text)
    spans = spans_from_path(path, n, n_text + 2)
    skipped = [k for k in range(n_text) if spans[1 + k] is None]
    stay = max((s[1] - s[0] + 1 for s in spans if s is not None), default=0)
    mass = None
    if text_mass is not None and n > 0:
        mass = float(np.asarray(text_mass, np.float64).reshape(-1)[:n].mean())
    return dict(coverage=1.0 if n_text == 0 else (n_text - len(skipped)) / n_text, skipped=skipped, longest_stay=int(stay), mean_text_mass=mass)


def describe(path, n, ids, text_mass, samples_per_code, sampling_rate, space_id=None, frame_bounds=None):
    """One utterance's alignment as SynthesizerTrn.align returns it: dict(path, spans, times (per column), token_spans / token_times
    (per caller's id), words (with `space_id`; each with its time), stats).  frame_bounds (a planned infer: FramePlan.code_bounds, with
    samples_per_code / 4 samples per frame): every time follows the plan's map (token_times_frames); None: the fixed 4 frames per code."""
    ids = np.asarray(ids).reshape(-1)
    p = np.asarray(path, np.int64).reshape(-1)[: int(n)]
    spans = spans_from_path(p, n, ids.size + 2)
    tok = spans[1:1 + ids.size]
    times_of = lambda sp: token_times(sp, samples_per_code, sampling_rate)  # noqa: E731
    if frame_bounds is not None:
        times_of = lambda sp: token_times_frames(sp, frame_bounds, samples_per_code // 4, sampling_rate)  # noqa: E731
    out = dict(path=p.astype(np.int32), spans=spans, times=times_of(spans), token_spans=tok,
               token_times=times_of(tok), stats=alignment_stats(p, n, ids.size, text_mass))
    if space_id is not None:
        words = group_words(ids, tok, space_id)
        for w, t in zip(words, times_of([w["span"] for w in words])):
            w["time"] = t
        out["words"] = words
    return out
