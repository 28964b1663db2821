"""Best-of-N code candidates: host-side bookkeeping (noise-stream ids, ranking).  No device work here: the scores come from
Runtime.gpt_score (dtts_gpt_score), the model's own log-probability of every candidate's codes.

Whether picking the likeliest of N candidates improves the audio is UNMEASURED (there is no trained checkpoint to listen to); what the
ranking does guarantee is that a candidate that drew the stop token is preferred to one that ran into max_generate_length."""
from __future__ import annotations

import numpy as np

MAX_CANDIDATES = 16
CANDIDATE_STREAM_STRIDE = 2 ** 20      # candidate c of utterance b draws its GPT noise from Philox stream sample_ids[b] + c * 2**20


def check_num_candidates(num_candidates, forced_codes=None):
    """host-side check of infer()'s num_candidates, before any launch -> int in 1 .. 16"""
    n = num_candidates
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= MAX_CANDIDATES:
        raise ValueError(f"num_candidates must be an integer in [1, {MAX_CANDIDATES}], not {num_candidates!r}")
    if int(n) > 1 and forced_codes is not None:
        raise ValueError("num_candidates > 1 samples its candidates: it cannot be combined with forced_codes")
    return int(n)


def check_choose(choose, B, num_candidates):
    """host-side check of infer()'s choose -> None or a list of B candidate indices in [0, num_candidates)"""
    if choose is None:
        return None
    c = [int(v) for v in choose]
    if len(c) != B or any(not 0 <= v < num_candidates for v in c):
        raise ValueError(f"choose must name one candidate in [0, {num_candidates}) for each of the {B} utterances, not {choose!r}")
    return c


def expand_sample_ids(sample_ids, num_candidates):
    """[B] utterance ids -> [B * N] ids in repeat_interleave order: candidate c of utterance b is sample_ids[b] + c * 2**20, so
    candidate 0 IS the single-candidate decode.  Two candidates on one noise stream would be the same draw sequence: ValueError."""
    ids = [int(i) + c * CANDIDATE_STREAM_STRIDE for i in sample_ids for c in range(int(num_candidates))]
    if len(set(ids)) != len(ids):
        raise ValueError(f"sample_ids {list(sample_ids)} expand to colliding candidate streams (stride {CANDIDATE_STREAM_STRIDE}): "
                         "two candidates would share a noise stream")
    if ids and (min(ids) < -2 ** 31 or max(ids) >= 2 ** 31):
        raise ValueError("expanded candidate stream ids leave the int32 range")
    return ids


def rank_candidates(logprobs, ncodes, stopped):
    """The candidates of ONE utterance -> (index of the best, scores float64 [N]).

    logprobs: N rows (arrays of >= ncodes[c] per-token log-probabilities; the stop token's included when it was drawn), ncodes [N] >= 1,
    stopped [N] bool (the candidate drew the stop token).  A candidate's score is the MEAN log-probability over its ncodes tokens (a
    sum would favour short sequences); every stopped candidate ranks above every candidate that ran into max_generate_length; ties go
    to the lowest index."""
    n = len(ncodes)
    if n < 1 or len(logprobs) != n or len(stopped) != n:
        raise ValueError("rank_candidates: one logprob row, one length and one stopped flag per candidate")
    scores = np.zeros(n, np.float64)
    for c in range(n):
        k = int(ncodes[c])
        if k < 1:
            raise ValueError("rank_candidates: a candidate has no tokens")
        scores[c] = float(np.mean(np.asarray(logprobs[c], np.float64)[:k]))
    best = 0
    for c in range(1, n):
        if (bool(stopped[c]), scores[c]) > (bool(stopped[best]), scores[best]):      # strict: ties keep the lower index
            best = c
    return best, scores
