"""Per-row sampling settings of a decode session: the host side.

Rows of different requests share a decode session (the batch is where the throughput comes from), and each keeps its own sampling
settings: the device sampler runs one workgroup per row and reads the row's slot of its control block (csrc/gpt_kernels.h GptCtl).
`resolve_sampling` is the ONE function that turns the `sampling=` argument of SynthesizerTrn.infer / infer_gpt / infer_stream /
infer_many and of UnifiedVoice.inference_speech_* into what Runtime.gpt_prefill / gpt_generate take as `rows=`; it runs on the host
only and raises ValueError before any launch.

    key                   range                          missing
    temperature           > 0, finite                    0.8    (the reference's call, vqvae/model_24k.py:782-792)
    top_p                 (0, 1]                         0.8
    top_k                 int >= 0, 0 = off              the call's top_k=
    repetition_penalty    > 0, finite                    2.0
    typical_mass          [0, 1], 0 / 1 = off            0 (off)
    max_generate_length   1 .. the call's                the call's max_generate_length=
    do_sample             bool                           True; False = greedy: top-k 1, temperature 1, top-p 1 (gpt/model.py's mapping)
    the eight non-beam keys of decode_options            the call's decode_options=

Refused: unknown keys, the beam keys (a beam session is uniform), a wrong row count, `sampling` together with num_beams > 1, a cap above
the call's.  How any setting sounds under a trained checkpoint is unmeasured here."""
import math
import numbers

from .decode_options import BEAM_KEYS, KEYS as PROCESSOR_KEYS, validate_decode_options

SCALAR_KEYS = ("temperature", "top_p", "top_k", "repetition_penalty", "typical_mass", "max_generate_length", "do_sample")
SAMPLING_KEYS = SCALAR_KEYS + PROCESSOR_KEYS
REFERENCE = dict(temperature=0.8, top_p=0.8, repetition_penalty=2.0, typical_mass=0.0)      # config.TEMPERATURE / TOP_P / REPETITION_PENALTY


def _real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def _int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _row(where, s, top_k, G, processors, vocab, base):
    """one row's dict (or None) -> the complete record Runtime takes"""
    s = {} if s is None else s
    if not hasattr(s, "items"):
        raise ValueError(f"{where}: a row's settings have to be a dict (or None), not {type(s).__name__}")
    for k in s:
        if k in BEAM_KEYS:
            raise ValueError(f"{where}: `{k}` is a beam-search keyword - a beam session is uniform, per-row settings are refused under beams")
        if k not in SAMPLING_KEYS:
            raise ValueError(f"{where}: unknown key `{k}` (served: {', '.join(SAMPLING_KEYS)})")
    get = lambda k, d: d if s.get(k) is None else s[k]      # noqa: E731
    t, p, rp, tm = get("temperature", base["temperature"]), get("top_p", base["top_p"]), get("repetition_penalty", base["repetition_penalty"]), \
        get("typical_mass", base["typical_mass"])
    k, cap, do_sample = get("top_k", top_k), get("max_generate_length", G), get("do_sample", True)
    if not _real(t) or not 0 < t < math.inf:
        raise ValueError(f"{where}: `temperature` has to be a finite float > 0, but is {t!r}")
    if not _real(p) or not 0 < p <= 1:
        raise ValueError(f"{where}: `top_p` has to be a float in (0, 1], but is {p!r}")
    if not _int(k) or k < 0:
        raise ValueError(f"{where}: `top_k` has to be an integer >= 0 (0 = off), but is {k!r}")
    if not _real(rp) or not 0 < rp < math.inf:
        raise ValueError(f"{where}: `repetition_penalty` has to be a finite float > 0, but is {rp!r}")
    if not _real(tm) or not 0 <= tm <= 1:
        raise ValueError(f"{where}: `typical_mass` has to be a float in [0, 1], but is {tm!r}")
    if not _int(cap) or not 1 <= cap <= G:
        raise ValueError(f"{where}: `max_generate_length` has to be an integer in 1 .. the call's {G}, but is {cap!r}")
    if not isinstance(do_sample, bool):
        raise ValueError(f"{where}: `do_sample` has to be a bool, but is {do_sample!r}")
    own = {k2: v for k2, v in s.items() if k2 in PROCESSOR_KEYS}
    try:
        proc = validate_decode_options({**processors, **own}, vocab=vocab, do_sample=do_sample)
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    if not do_sample:       # greedy = the one largest logit behind the penalty and the processors: top-k 1 keeps exactly it
        k, t, p, tm = 1, 1.0, 1.0, 0.0
    return dict(top_k=int(k), top_p=float(p), temperature=float(t), repetition_penalty=float(rp), typical_mass=float(tm),
                max_generate_length=int(cap), processors=proc)


def resolve_sampling(sampling, B, *, top_k=50, max_generate_length, decode_options=None, vocab=8194, num_beams=None, base=None,
                     always_rows=False):
    """sampling -> None (today's uniform session: the scalar fields, the very launches and bits of a call without `sampling`) or a list
    of B complete row records dict(top_k, top_p, temperature, repetition_penalty, typical_mass, max_generate_length, processors) for
    Runtime's `rows=`.

    sampling: None; a dict (the same settings for every row); or a sequence of B entries, each None or a dict.  A key missing from a
    row takes the call's top_k / max_generate_length / decode_options, else the reference's constant (`base` replaces those constants:
    UnifiedVoice's mirror hands in its own call's values).  Rows that all resolve to what the call decodes under anyway resolve to
    None (always_rows: never - the caller merges them with another request's rows)."""
    if sampling is None and not always_rows:
        return None
    B, G = int(B), int(max_generate_length)
    if sampling is not None and num_beams is not None and num_beams > 1:
        raise ValueError("`sampling` cannot be combined with `num_beams` > 1 (a beam session is uniform)")
    consts = dict(REFERENCE, **(base or {}))
    processors = validate_decode_options(decode_options, vocab=vocab)
    stray = [k for k in processors if k in BEAM_KEYS]
    if stray and sampling is not None:
        raise ValueError("`sampling` cannot be combined with `num_beams` > 1 (a beam session is uniform)")
    if sampling is None or hasattr(sampling, "items"):
        rec = _row("sampling", sampling, top_k, G, processors, vocab, consts)
        rows = [dict(rec) for _ in range(B)]
    else:
        if isinstance(sampling, (str, bytes)) or not hasattr(sampling, "__len__"):
            raise ValueError(f"`sampling` has to be None, a dict or a sequence of {B} dicts, not {type(sampling).__name__}")
        if len(sampling) != B:
            raise ValueError(f"`sampling` holds {len(sampling)} rows for a batch of {B}")
        rows = [_row(f"sampling[{b}]", s, top_k, G, processors, vocab, consts) for b, s in enumerate(sampling)]
    if always_rows:
        return rows
    plain = _row("sampling", None, top_k, G, processors, vocab, consts)
    return None if all(r == plain for r in rows) else rows


def session_cap(rows, max_generate_length):
    """the max_generate_length a session of these rows runs under: its largest row cap (the library asks for exactly that)"""
    return int(max_generate_length) if rows is None else max(r["max_generate_length"] for r in rows)


def check_forced_caps(rows, forced):
    """forced codes next to per-row settings: a row whose cap is below the length of its forced row cannot be served"""
    if rows is None or forced is None:
        return
    for b, (r, f) in enumerate(zip(rows, forced)):
        if len(f) > r["max_generate_length"]:
            raise ValueError(f"sampling[{b}]: `max_generate_length` {r['max_generate_length']} is below the {len(f)} forced_codes of the row")


def repeat_rows(rows, n):
    """num_candidates / num_return_sequences = n: the settings repeat with the rows (repeat_interleave)"""
    return None if rows is None else [dict(r) for r in rows for _ in range(int(n))]
