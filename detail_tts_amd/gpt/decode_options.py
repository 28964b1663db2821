"""HF generate()'s remaining decode-time logits processors as the device sampler serves them: the host side.

The reference's inference_speech_tortoise / inference_speech_valle (gpt/model.py:514-579) hand **hf_generate_kwargs to HF's generate;
`validate_decode_options` is the ONE function that checks the keywords below - for the mirror's keyword arguments and for the
`decode_options` dict of SynthesizerTrn.infer / infer_gpt / infer_stream alike - before any library call, with the error classes of the
HF constructors (transformers generation/logits_process.py), and returns what Runtime hands to dtts_gpt_options.

    keyword                           HF class                                  off
    no_repeat_ngram_size = n          NoRepeatNGramLogitsProcessor              None, 0
    min_length                        MinLengthLogitsProcessor                  None, 0
    min_new_tokens                    MinNewTokensLengthLogitsProcessor         None, 0
    exponential_decay_length_penalty  ExponentialDecayLengthPenalty             None
    suppress_tokens                   SuppressTokensLogitsProcessor             None, []
    begin_suppress_tokens             SuppressTokensAtBeginLogitsProcessor      None, []
    min_p                             MinPLogitsWarper        (do_sample only)  None, 0
    epsilon_cutoff                    EpsilonLogitsWarper     (do_sample only)  None, 0
    num_beams = K                     _beam_search (do_sample=False)            None, 1      (2 .. 16: csrc/gpt_beam.hip)
    length_penalty, early_stopping    its two knobs (False / True / "never")    read under beams only
Under beams nothing is sampled, and HF runs the processors on LOG-PROBABILITIES: the repetition penalty multiplies the (negative) scores
of seen ids.  `split_beam_options` takes the three beam keys out of a validated dict; `beam_request` is what the public entries call (it also
refuses what beams exclude); Runtime refuses a processors dict that still carries a beam key.

Counting (HF's input_ids of a row = its fill-id-1 prefix columns, 8192, an acoustic prompt's codes, input_tokens, generated tokens):
min_length counts all of it; min_new_tokens, the decay's start and begin_suppress_tokens count from the end of HF's prompt, which holds
everything but the generated tokens.  `first_stop_step` is the fold of the two length processors the control block carries."""
import numbers

NGRAM_MAX = 16          # SAMP_NGRAM_MAX of csrc/gpt_kernels.h
KEYS = ("no_repeat_ngram_size", "min_length", "min_new_tokens", "exponential_decay_length_penalty", "suppress_tokens",
        "begin_suppress_tokens", "min_p", "epsilon_cutoff")
WARPER_KEYS = ("min_p", "epsilon_cutoff")


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _ids(name, v, vocab):
    ids = [v] if _is_int(v) else list(v)
    for i in ids:
        if not _is_int(i) or not 0 <= int(i) < vocab:
            raise ValueError(f"`{name}` has to be a list of token ids in [0, {vocab}), but is {v!r}")
    return sorted(set(int(i) for i in ids))


def validate_decode_options(options, vocab=8194, do_sample=True, strict=True):
    """options: None or a mapping of the keywords above -> dict of the ones that are switched ON, normalised (ints, a (start, factor)
    tuple, sorted id lists, floats); {} means today's decode.  Every bad value raises ValueError here, before any launch.  strict: a key
    outside KEYS is an error (the decode_options dict); the mirror passes strict=False and hands over only the keys it knows.  Under
    do_sample=False the two warpers are checked and then dropped, as HF builds them only when sampling."""
    if options is None:
        return {}
    if not hasattr(options, "items"):
        raise ValueError(f"decode_options has to be a dict of {', '.join(KEYS)}, not {type(options).__name__}")
    out = {}
    if any(k in options for k in BEAM_KEYS):          # the beam keywords travel in the same dict; K = 1 / None leaves nothing behind
        K, lp, es = validate_beam_options(options.get("num_beams"), options.get("length_penalty"), options.get("early_stopping"))
        if K:
            out.update(num_beams=K, length_penalty=lp, early_stopping={0: False, 1: True, 2: "never"}[es])
            do_sample = False
    for k, v in options.items():
        if k in BEAM_KEYS:
            continue
        if k not in KEYS:
            if strict:
                raise ValueError(f"decode_options: unknown keyword {k!r} (served: {', '.join(KEYS)})")
            continue
        if v is None:
            continue
        if k == "no_repeat_ngram_size":
            if not _is_int(v) or v < 0:
                raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {v}")
            if v > NGRAM_MAX:
                raise ValueError(f"no_repeat_ngram_size {v} is above the device sampler's cap of {NGRAM_MAX}")
            if v:
                out[k] = int(v)
        elif k in ("min_length", "min_new_tokens"):
            if not _is_int(v) or v < 0:
                raise ValueError(f"`{k}` has to be a non-negative integer, but is {v}")
            if v:
                out[k] = int(v)
        elif k == "exponential_decay_length_penalty":
            if not isinstance(v, (tuple, list)) or len(v) != 2 or not _is_int(v[0]) or v[0] < 0 or isinstance(v[1], bool) or \
                    not isinstance(v[1], numbers.Real):
                raise ValueError(f"`exponential_decay_length_penalty` has to be (start_index >= 0, decay_factor), but is {v!r}")
            if not 1.0 < float(v[1]) < float("inf"):
                raise ValueError(f"`exponential_decay_length_penalty`: the decay factor has to be a finite float > 1, but is {v[1]}")
            out[k] = (int(v[0]), float(v[1]))
        elif k in ("suppress_tokens", "begin_suppress_tokens"):
            ids = _ids(k, v, vocab)
            if ids:
                out[k] = ids
        elif k == "min_p":
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0 <= v <= 1.0:
                raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {v}")
            if v > 0 and do_sample:
                out[k] = float(v)
        elif k == "epsilon_cutoff":
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0 <= v < 1:          # (NaN fails the range)
                raise ValueError(f"`epsilon_cutoff` has to be a float > 0 and < 1, but is {v}")
            if v > 0 and do_sample:
                out[k] = float(v)
    return out


BEAMS_MAX = 16          # BEAM_MAXK of csrc/gpt_kernels.h: the K beams of an utterance are rows of ONE decode session
BEAM_KEYS = ("num_beams", "length_penalty", "early_stopping")


def validate_beam_options(num_beams=None, length_penalty=None, early_stopping=None, **other):
    """HF generate()'s beam keywords -> (K, length_penalty, early_stopping code 0 / 1 / 2); K = 0 means no beam search (num_beams None
    or 1: today's decode, the other two keywords are then only checked, as HF ignores them without beams).  `other`: what the call also
    carries and beams exclude - do_sample, typical_sampling, input_tokens, forced_codes, forced_uniforms, num_candidates,
    num_return_sequences, stream; each refusal is a ValueError that names its keyword, before any launch."""
    if num_beams is None:
        num_beams = 1
    if not _is_int(num_beams) or num_beams < 1:
        raise ValueError(f"`num_beams` has to be an integer >= 1, but is {num_beams!r}")
    if length_penalty is None:
        length_penalty = 1.0
    if isinstance(length_penalty, bool) or not isinstance(length_penalty, numbers.Real) or not float("-inf") < float(length_penalty) < float("inf"):
        raise ValueError(f"`length_penalty` has to be a finite float, but is {length_penalty!r}")
    if early_stopping is None:
        early_stopping = False
    if not (isinstance(early_stopping, bool) or early_stopping == "never"):
        raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {early_stopping!r}")
    es = 2 if early_stopping == "never" else int(bool(early_stopping))
    K = int(num_beams)
    nrs = other.get("num_return_sequences")
    if K == 1:
        return 0, float(length_penalty), es
    if K > BEAMS_MAX:
        raise ValueError(f"`num_beams` = {K} does not fit a decode session: the beams of an utterance are rows of one session of {BEAMS_MAX}")
    if other.get("do_sample"):
        raise ValueError("`do_sample`=True with `num_beams` > 1 (beam-sample) is not served: pass do_sample=False")
    for key in ("typical_sampling", "input_tokens", "forced_codes", "forced_uniforms", "stream"):
        if other.get(key) is not None and other.get(key) is not False:
            raise ValueError(f"`{key}` cannot be combined with `num_beams` > 1")
    if (other.get("num_candidates") or 1) > 1:
        raise ValueError("`num_candidates` > 1 cannot be combined with `num_beams` > 1 (the beams are the candidates)")
    if nrs is not None and (not _is_int(nrs) or not 1 <= nrs <= K):
        raise ValueError(f"`num_return_sequences` ({nrs}) has to be smaller or equal to `num_beams` ({K})")
    return K, float(length_penalty), es


def split_beam_options(validated):
    """validated decode options -> (processors without the beam keys, None or dict(num_beams, length_penalty, early_stopping))"""
    proc = {k: v for k, v in validated.items() if k not in BEAM_KEYS}
    beam = {k: validated[k] for k in BEAM_KEYS if k in validated}
    return proc, (beam if beam.get("num_beams", 0) > 1 else None)


def beam_request(decode_options, forced_codes=None, num_candidates=1, return_candidates=False, stream=False):
    """What infer / infer_gpt / infer_stream do with their decode_options: validate, split, and refuse - by the keyword's name, before any
    launch - what a beam search cannot be combined with.  -> (processors, None or dict(num_beams, length_penalty, early_stopping))"""
    proc, beam = split_beam_options(validate_decode_options(decode_options))
    if beam:
        validate_beam_options(**beam, forced_codes=forced_codes, num_candidates=num_candidates, stream=True if stream else None)
        if return_candidates:
            raise ValueError("`return_candidates` cannot be combined with `num_beams` > 1 (the beams are the candidates)")
    return proc, beam


def first_stop_step(input_len, forced_prefix, min_length=0, min_new_tokens=0):
    """The first decode step (0-based index of the generated token) at which the stop token may be drawn.  input_len: the row's
    input_ids length at step 0 = 1 + text positions + mel stream (fill ids, 8192 and an acoustic prompt's codes included; GptCtl.lp);
    forced_prefix: the input_tokens in front of the generated tokens, which HF counts as prompt.  At step j HF sees input_len + j ids,
    j - forced_prefix of them new: the stop is -inf while input_len + j < min_length or j - forced_prefix < min_new_tokens.
    This IS the library's fold (dtts_gpt_first_stop_step, host only: what dtts_gpt_prefill writes into the control block)."""
    from .. import _lib
    return int(_lib.load().dtts_gpt_first_stop_step(int(input_len), int(forced_prefix), int(min_length), int(min_new_tokens)))


def decay_multipliers(factor, n):
    """float32 [n]: the table the library uploads for exponential_decay_length_penalty = (start, factor) (dtts_gpt_decay_multipliers,
    host only): entry i = float(factor ** i - 1), the power in double as Python evaluates it, saturated at 1e30.  Any factor > 1 is
    served at any max_generate_length: far behind `start` HF's own multiplier leaves float32 (its scores turn NaN, or Python's pow
    raises OverflowError); here the stop token is then the only one left."""
    import numpy as np
    from .. import _lib
    out = np.zeros(int(n), np.float32)
    _lib.load().dtts_gpt_decay_multipliers(float(factor), int(n), out.ctypes.data)
    return out
