"""Speaking-rate control: the frame plan of stage B, on the host (pure functions on lists and arrays: no device, no library).

The reference's DiffusionTts.timestep_independent expands the code embedding [B,768,n] to ANY frame count with
F.interpolate(size=T, mode='nearest') (vqvae/diff_model.py:252); only do_spectrogram_diffusion fixes T = 4 n.  A frame plan says, per
row b with n_b codes, how many mel frames T_b it gets and which code every frame reads: a map m_b[0 .. T_b) into [0, n_b).  Three ways
to ask for one (at most one per call):

  speed        a rate, or one per row, in [0.25, 4]: T_b = max(4, 4 int(n_b / speed_b + 0.5)) in float64, and the UNIFORM map - torch's
               own nearest rule in float32 (uniform_map)
  durations    per row n_b integers >= 0, the frames of every code (at least one positive): the map is repeat_interleave; a sum that
               is no multiple of 4 is completed by extending the last code of positive duration (the plan reports it, `extended`)
  span_rates   per row a list of (first_code, last_code, rate), inclusive spans as align() hands them out, disjoint, inside [0, n_b),
               rate in [0.25, 4]: sugar that becomes durations - a code outside every span gets 4 frames, a span of L codes
               F = max(1, int(4 L / rate + 0.5)) frames spread as d_j = (j + 1) F // L - j F // L

durations and span_rates need the codes before the call (forced_codes).  Every T_b is a multiple of 4, as the vocoder needs it.
speed None - or 1.0 with nothing else - is no plan at all: the caller keeps the x4 launch and its bits.

The maps themselves are built on the device (csrc/frame_map.hip) from lens_n, frames and durations; their restatement here serves the
alignment times of a planned call (code_bounds) and nothing on the hot path.  Audio quality at other rates under a trained checkpoint
is UNMEASURED."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MIN_RATE, MAX_RATE = 0.25, 4.0
FRAMES_PER_CODE = 4          # the reference's fixed expansion (do_spectrogram_diffusion: output_seq_len = latents.shape[1] * 4)
SAMPLES_PER_FRAME = 256      # the vocoder's hop: 1024 samples per code at 4 frames per code


@dataclass
class FramePlan:
    """frames [B]: T_b; durations: None (the uniform map) or int32 [B, max(n)], zero beyond a row's codes, each row summing to T_b;
    extended [B]: the frames added to a row's last positive duration to reach a multiple of 4 (0 for a uniform plan)"""
    n: list
    frames: list
    durations: object = None
    extended: list = None

    @property
    def Tmax(self):
        return max(self.frames)

    def row_map(self, b):
        """row b's frame -> code map, int64 [T_b] (the device kernels' result, restated)"""
        if self.durations is None:
            return uniform_map(self.n[b], self.frames[b])
        return durations_map(self.durations[b, : self.n[b]])

    def code_bounds(self, b):
        """int64 [n_b + 1]: code j covers frames [bounds[j], bounds[j + 1]) - bounds[j] is the first t with m[t] >= j, T_b when there is
        none; a code without a frame gets an empty interval"""
        return code_bounds(self.row_map(b), self.n[b])


def uniform_map(n, T):
    """F.interpolate(arange(n), size=T, mode='nearest') as an index map, bit for bit: torch computes, in FLOAT32 with the division and
    the product each rounded once,  scale = float(n) / float(T);  m[t] = min(int(floorf(float(t) * scale)), n - 1).  That is not
    floor(t n / T) - e.g. (n, T, t) = (14, 92, 46): 46 * 14 / 92 = 7 exactly, the float32 scale falls below 14 / 92 and the product
    floors to 6.  At T = 4 n the scale is exactly 0.25 and the map is t // 4."""
    n, T = int(n), int(T)
    if n < 1 or T < 1:
        raise ValueError(f"uniform_map: n and T have to be >= 1, but are {n} and {T}")
    scale = np.float32(n) / np.float32(T)
    prod = np.arange(T, dtype=np.float32) * scale                 # float32 x float32 -> float32, rounded once
    return np.minimum(np.floor(prod).astype(np.int64), n - 1)


def durations_map(durations):
    """repeat_interleave(arange(n), durations): code j owns durations[j] consecutive frames"""
    d = np.asarray(durations, np.int64).reshape(-1)
    return np.repeat(np.arange(d.size, dtype=np.int64), d)


def code_bounds(m, n):
    """a monotone frame -> code map m [T] over n codes -> int64 [n + 1], bounds[j] = the first t with m[t] >= j (T when none)"""
    m = np.asarray(m, np.int64).reshape(-1)
    return np.searchsorted(m, np.arange(int(n) + 1), side="left").astype(np.int64)


def _rate(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what} has to be a number in [{MIN_RATE}, {MAX_RATE}], but is {v!r}")
    v = float(v)
    if not MIN_RATE <= v <= MAX_RATE:                              # (NaN fails both comparisons)
        raise ValueError(f"{what} has to be in [{MIN_RATE}, {MAX_RATE}], but is {v!r}")
    return v


def check_speed(speed, B):
    """speed -> None (no plan: speed None, or every rate exactly 1.0) or a list of B rates.  ValueError on anything outside
    [0.25, 4], on a row count other than B."""
    if speed is None:
        return None
    if isinstance(speed, (list, tuple, np.ndarray)) or (hasattr(speed, "dim") and speed.dim() > 0):
        rows = [v.item() if hasattr(v, "item") else v for v in (speed.tolist() if hasattr(speed, "tolist") else speed)]
        if len(rows) != B:
            raise ValueError(f"speed holds {len(rows)} rates for B = {B} rows: one number, or one per row")
        rates = [_rate(v, f"speed[{b}]") for b, v in enumerate(rows)]
    else:
        rates = [_rate(speed.item() if hasattr(speed, "item") else speed, "speed")] * B
    return None if all(r == 1.0 for r in rates) else rates


def speed_frames(n, rate):
    """T = max(4, 4 int(n / rate + 0.5)), in float64"""
    return max(4, 4 * int(np.float64(n) / np.float64(rate) + 0.5))


def check_durations(durations, n):
    """per-row durations against the rows' code counts n -> a list of int64 arrays.  ValueError on a row count or a length that does not
    match, a non-integer or negative entry, a row without a positive entry."""
    if durations is None or isinstance(durations, (int, float)) or len(durations) != len(n):
        raise ValueError(f"durations has to hold one row of frame counts per utterance (B = {len(n)})")
    rows = []
    for b, (d, nb) in enumerate(zip(durations, n)):
        a = np.asarray(d.cpu().numpy() if hasattr(d, "cpu") else d)
        if a.ndim != 1 or a.size != nb:
            raise ValueError(f"durations[{b}] holds {a.size if a.ndim == 1 else tuple(a.shape)} entries for the row's {nb} codes: one per code")
        if a.dtype.kind not in "iu":
            if a.dtype.kind != "f" or not np.array_equal(a, np.floor(a)):
                raise ValueError(f"durations[{b}] has to hold integers (frames per code)")
        a = a.astype(np.int64)
        if a.min() < 0 or a.max() < 1:
            raise ValueError(f"durations[{b}] has to hold non-negative frame counts, at least one of them positive")
        if int(a.sum()) >= 2 ** 24:
            raise ValueError(f"durations[{b}] sums to {int(a.sum())} frames")
        rows.append(a)
    return rows


def span_durations(n, spans):
    """one row: (first_code, last_code, rate) spans over n codes -> int64 [n] durations.  ValueError on a span outside [0, n), on
    overlapping spans, on a rate outside [0.25, 4]."""
    d = np.full(int(n), FRAMES_PER_CODE, np.int64)
    taken = np.zeros(int(n), bool)
    for s in spans:
        if len(s) != 3:
            raise ValueError(f"span_rates: a span is (first_code, last_code, rate), not {s!r}")
        a, b, rate = s
        if int(a) != a or int(b) != b or not 0 <= int(a) <= int(b) < n:
            raise ValueError(f"span_rates: the span ({a}, {b}) is not inside the row's codes 0 .. {n - 1} (first <= last, inclusive)")
        a, b, rate = int(a), int(b), _rate(rate, "span_rates: a rate")
        if taken[a:b + 1].any():
            raise ValueError(f"span_rates: the span ({a}, {b}) overlaps another span of its row")
        taken[a:b + 1] = True
        L = b - a + 1
        F = max(1, int(np.float64(4 * L) / np.float64(rate) + 0.5))
        j = np.arange(L, dtype=np.int64)
        d[a:b + 1] = (j + 1) * F // L - j * F // L
    return d


def check_request(speed=None, durations=None, span_rates=None, forced_codes=None, B=None):
    """the three keywords of one request, before any launch -> None (no plan: today's path) or a dict for make_plan.  At most one of the
    three; durations and span_rates need forced_codes (the code counts have to be known before the call) and are checked in full here."""
    given = [k for k, v in (("speed", speed), ("durations", durations), ("span_rates", span_rates)) if v is not None]
    if len(given) > 1:
        raise ValueError(f"at most one of speed, durations and span_rates may be given, not {' and '.join(given)}")
    if not given:
        return None
    if speed is not None:
        rates = check_speed(speed, B)
        return None if rates is None else dict(speed=rates)
    if forced_codes is None:
        raise ValueError(f"{given[0]} needs forced_codes: every row's code count has to be known before the call "
                         f"(re-render the codes of an earlier call: return_candidates / return_alignment)")
    n = [len(c) for c in forced_codes]
    if B is not None and len(n) != B:
        raise ValueError(f"{given[0]}: {len(n)} forced code rows for B = {B}")
    if durations is not None:
        return dict(durations=check_durations(durations, n))
    if isinstance(span_rates, (int, float)) or len(span_rates) != len(n):
        raise ValueError(f"span_rates has to hold one list of (first_code, last_code, rate) per utterance (B = {len(n)})")
    return dict(durations=[span_durations(nb, s) for nb, s in zip(n, span_rates)])


def make_plan(n, request):
    """the rows' code counts and check_request's result -> FramePlan, or None for no plan"""
    if request is None:
        return None
    n = [int(v) for v in n]
    if "speed" in request:
        rates = request["speed"]
        if len(rates) != len(n):
            raise ValueError(f"speed holds {len(rates)} rates for {len(n)} rows")
        return FramePlan(n=n, frames=[speed_frames(nb, r) for nb, r in zip(n, rates)], extended=[0] * len(n))
    rows = request["durations"]
    if len(rows) != len(n) or any(len(d) != nb for d, nb in zip(rows, n)):
        raise ValueError(f"durations of {[len(d) for d in rows]} entries for rows of {n} codes")
    dur = np.zeros((len(n), max(n)), np.int32)
    frames, extended = [], []
    for b, d in enumerate(rows):
        d = np.array(d, np.int64)
        total = int(d.sum())
        ext = -total % 4
        d[np.nonzero(d)[0][-1]] += ext                            # the last code that speaks is held to the next multiple of 4
        dur[b, : d.size] = d
        frames.append(total + ext)
        extended.append(ext)
    return FramePlan(n=n, frames=frames, durations=dur, extended=extended)
