"""Host side of mel inpainting (SynthesizerTrn.inpaint_mel): the argument checks, code spans -> frame mask, and splice_codes.  Pure
functions on tensors and lists: no device, no library."""
from __future__ import annotations

import numpy as np
import torch

from .utils.diffusion import check_keep

FRAMES_PER_CODE = 4


def spans_to_keep(spans, B, T):
    """spans: per row a list of inclusive code spans (first, last) - the form SynthesizerTrn.align hands out under "spans",
    "token_spans" and each word's "span"; None entries (a token that owns no code) are skipped - or one such list for all rows.
    Frames 4 first .. 4 last + 3 of every span are to be regenerated -> keep, bool [B,T], False there.  ValueError: a span outside
    [0, T / 4), reversed, not a pair of integers, or overlapping another span of its row."""
    n = T // FRAMES_PER_CODE
    if not isinstance(spans, (list, tuple)):
        raise ValueError("spans must be a list per row of (first, last) code spans")
    rows = list(spans)
    is_span = lambda s: s is None or (isinstance(s, (list, tuple)) and len(s) == 2 and all(isinstance(v, (int, np.integer)) for v in s))  # noqa: E731
    if all(is_span(s) for s in rows):            # one list of spans: every row's
        rows = [rows] * B
    if len(rows) != B:
        raise ValueError(f"spans has {len(rows)} rows for a batch of {B}")
    keep = torch.ones((B, T), dtype=torch.bool)
    for b, row in enumerate(rows):
        if not isinstance(row, (list, tuple)):
            raise ValueError(f"spans[{b}] must be a list of (first, last) code spans")
        for s in row:
            if s is None:
                continue
            if not is_span(s) or isinstance(s[0], bool) or isinstance(s[1], bool):
                raise ValueError(f"spans[{b}]: {s!r} is not a (first, last) pair of code indices")
            first, last = int(s[0]), int(s[1])
            if not 0 <= first <= last < n:
                raise ValueError(f"spans[{b}]: ({first}, {last}) is reversed or outside [0, {n})")
            sl = slice(FRAMES_PER_CODE * first, FRAMES_PER_CODE * (last + 1))
            if not bool(keep[b, sl].all()):
                raise ValueError(f"spans[{b}]: ({first}, {last}) overlaps another span")
            keep[b, sl] = False
    return keep


def check_inpaint_args(mel_shape, spans, keep, codes, resample, sampler, eta, t_start, n_steps):
    """every refusal of inpaint_mel that needs no device, before any launch -> keep, bool [B,T] on the host.
    Nothing kept is allowed with t_start=None (it is the plain loop); everything kept is refused: there is nothing to do."""
    if len(mel_shape) != 3 or mel_shape[-1] % FRAMES_PER_CODE != 0 or mel_shape[-1] == 0:
        raise ValueError(f"mel must be [B,128,T] with T a multiple of 4 (the codes' hop), not shape {tuple(mel_shape)}")
    B, _, T = mel_shape
    if (spans is None) == (keep is None):
        raise ValueError("give exactly one of spans= (code spans to regenerate) and keep= (a frame mask)")
    if sampler == "dpmsolver++":
        raise ValueError("inpainting is not available with dpmsolver++ (a multistep history does not survive the overwrite)")
    if sampler not in ("p", "ddim"):
        raise ValueError(f"sampler must be 'p' or 'ddim', not {sampler!r}")
    if not float(eta) >= 0.0:
        raise ValueError(f"eta must be >= 0, not {eta!r}")
    if isinstance(resample, bool) or not isinstance(resample, (int, np.integer)) or not 1 <= resample <= 32:
        raise ValueError(f"resample must be an integer in [1, 32], not {resample!r}")
    if t_start is not None and (isinstance(t_start, bool) or not isinstance(t_start, (int, np.integer)) or not 0 <= t_start < n_steps):
        raise ValueError(f"t_start must be an integer in [0, {n_steps}), not {t_start!r}")
    if codes is not None and tuple(torch.as_tensor(codes).shape) != (B, T // FRAMES_PER_CODE):
        raise ValueError(f"codes must be [{B}, {T // FRAMES_PER_CODE}] (one per 4 frames), not {tuple(torch.as_tensor(codes).shape)}")
    k = spans_to_keep(spans, B, T) if keep is None else check_keep(torch.as_tensor(keep).cpu(), B, T)
    if bool(k.all()):
        raise ValueError("every frame is kept: there is nothing to inpaint")
    return k


def splice_codes(mel, codes, span, new_codes):
    """Replace the inclusive code span (first, last) of ONE utterance by new_codes of any length (zero included): mel [128,T] or
    [1,128,T] (raw log-mel, T = 4 n), codes [n] or [1,n] -> (mel' [1,128,T'], codes' [1,n'], keep' bool [1,T']) with n' = n - (last -
    first + 1) + len(new_codes), T' = 4 n'.  The span's frames are cut out and 4 len(new_codes) placeholder frames (zeros: inpaint_mel
    never reads them) go in, keep' False exactly there.  Where new_codes come from - infer_gpt, forced_codes, a prompt decode - is the
    caller's business.  Feed the three to inpaint_mel(mel', ..., keep=keep', codes=codes')."""
    mel, codes = torch.as_tensor(mel), torch.as_tensor(codes)
    mel = mel[None] if mel.dim() == 2 else mel
    codes = codes[None] if codes.dim() == 1 else codes
    if mel.dim() != 3 or mel.shape[0] != 1 or codes.dim() != 2 or codes.shape[0] != 1 or mel.shape[-1] != FRAMES_PER_CODE * codes.shape[-1]:
        raise ValueError(f"splice_codes takes one utterance: mel [1,128,4n] and codes [1,n], not {tuple(mel.shape)} and {tuple(codes.shape)}")
    n = codes.shape[-1]
    if not (isinstance(span, (list, tuple)) and len(span) == 2):
        raise ValueError(f"span must be (first, last), not {span!r}")
    first, last = int(span[0]), int(span[1])
    if not 0 <= first <= last < n:
        raise ValueError(f"span ({first}, {last}) is reversed or outside [0, {n})")
    new = torch.as_tensor(new_codes).reshape(-1).to(codes.dtype).to(codes.device)
    m = int(new.numel())
    f0, f1 = FRAMES_PER_CODE * first, FRAMES_PER_CODE * (last + 1)
    hole = torch.zeros((1, mel.shape[1], FRAMES_PER_CODE * m), dtype=mel.dtype, device=mel.device)
    mel2 = torch.cat([mel[:, :, :f0], hole, mel[:, :, f1:]], dim=-1)
    codes2 = torch.cat([codes[:, :first], new[None], codes[:, last + 1:]], dim=-1)
    keep2 = torch.ones((1, mel2.shape[-1]), dtype=torch.bool)
    keep2[:, f0:f0 + FRAMES_PER_CODE * m] = False
    return mel2, codes2, keep2
