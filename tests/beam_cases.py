"""The planted beam-search steps of tests/golden/beam_steps.npz: case table and input regeneration (no logits are stored).

A case is U utterances of K beams decoded for `steps` steps over a vocabulary of V ids (stop token V - 1, which is also the fill id of
unwritten positions), behind a prompt of P ids per utterance.  The logits of (step, row) depend on the case's seed alone - not on what
the beams hold - so HF's own functions (make_golden_beams.py), the numpy restatement (beam_model.py) and the device (op_beam_step) can
be fed the same rows.  Each row has 3K "hot" ids at spread levels over a flat background; `eos_rank[step]` plants the stop token at that
rank of every row (0 = the row's best id) at that step, or leaves it in the background (None).

    G      max new tokens: a continuation also stops when step + 1 == G ("max_length reached")
    lp     length_penalty        es   early_stopping: 0 False, 1 True, 2 "never"
    rp     repetition penalty    ngram   no_repeat_ngram_size     (both act on log-probabilities)
The seed actually used is the first at or above `seed` whose decision gaps are all >= MIN_GAP / MIN_REL_GAP; the generator searches it and stores it."""
import hashlib

import numpy as np

MIN_GAP = 1e-2          # between adjacent accumulated scores of the top 2K + 1 candidates
MIN_REL_GAP = 1e-3      # between adjacent scores of the finished-set merge and in the heuristic's comparison, relative to the larger one
                        # (those are divided by length ** length_penalty: their scale moves with the penalty, float32's resolution with it)


def _c(V, K, U, steps, G, eos_rank, lp=1.0, es=0, rp=1.0, ngram=0, P=3, seed=0, nrs=None):
    return dict(V=V, K=K, U=U, steps=steps, G=G, eos_rank=eos_rank, lp=lp, es=es, rp=rp, ngram=ngram, P=P, seed=seed, nrs=nrs or K)


N = None
CASES = {
    # stop tokens entering the second K only (rank K .. 2K-1 of the flat candidates comes from rank >= 1 inside a row)
    "v8194_k2_second_k": _c(8194, 2, 1, 6, 12, [N, N, 2, N, 3, N]),
    # ... and the first K; one finished hypothesis beats later ones or not depending on the length penalty
    "v8194_k3_first_k": _c(8194, 3, 2, 7, 12, [N, 1, N, 0, N, 1, N], seed=100),
    "v8194_k8": _c(8194, 8, 1, 5, 12, [N, N, 1, 0, 2], seed=200),
    "v40_k3_u3": _c(40, 3, 3, 8, 12, [N, 1, N, 0, 1, N, 0, N], seed=300),
    # every one of the first K candidates stops at once (the stop token dominates every row), then the search goes on from the second K
    "all_first_k_stop": _c(8194, 3, 1, 6, 12, [N, N, "all", N, 1, N], seed=400),
    # max_length: G = steps, the last step stops every continuation
    "max_length_k2": _c(8194, 2, 2, 5, 5, [N, N, 1, N, N], seed=500),
    "max_length_k8_v40": _c(40, 8, 1, 4, 4, [N, 2, N, N], seed=600),
    # length_penalty in {0, 0.5, 2, -1} (1 is everywhere else), with stops early and late so that the divisor decides the order
    "lp0": _c(8194, 3, 1, 8, 12, [N, 0, N, 1, N, 0, 1, N], lp=0.0, seed=700),
    "lp05": _c(8194, 3, 1, 8, 12, [N, 0, N, 1, N, 0, 1, N], lp=0.5, seed=800),
    "lp2": _c(8194, 3, 2, 8, 12, [N, 0, N, 1, N, 0, 1, N], lp=2.0, seed=900),
    "lp_neg1": _c(8194, 2, 1, 8, 12, [N, 0, N, 1, N, 0, 1, N], lp=-1.0, seed=1000),
    # early_stopping True (stops once K are finished) and "never" (both signs of the length penalty)
    "es_true": _c(8194, 2, 2, 8, 12, [N, 0, 0, N, 0, 1, N, 0], es=1, seed=1100),
    "es_true_k3_v40": _c(40, 3, 1, 8, 12, [N, 0, 0, 0, N, 1, N, 0], es=1, seed=1200),
    "es_never_lp1": _c(8194, 2, 1, 8, 12, [N, 0, 0, N, 0, 1, N, 0], es=2, lp=1.0, seed=1300),
    "es_never_lp_neg": _c(8194, 2, 2, 8, 12, [N, 0, 0, N, 0, 1, N, 0], es=2, lp=-1.0, seed=1400),
    "es_never_lp2_k3": _c(8194, 3, 1, 8, 9, [N, 0, 0, 0, N, 1, 0, 0], es=2, lp=2.0, seed=1450),
    # the two processors that depend on a row's own sequence, on log-probabilities
    "rep_penalty": _c(8194, 3, 2, 7, 12, [N, N, 1, N, 0, N, 1], rp=2.0, seed=1500),
    "rep_penalty_v40": _c(40, 2, 1, 8, 12, [N, N, 1, N, 0, N, 1, N], rp=1.3, seed=1600),
    "ngram2": _c(40, 3, 1, 8, 12, [N, N, N, 1, N, N, 0, N], ngram=2, seed=1700),
    "ngram3_rp": _c(8194, 2, 2, 8, 12, [N, N, N, 1, N, N, 0, N], ngram=3, rp=1.5, seed=1800),
}


def prompts(case):
    """[U, P] prompt ids of the utterances (never the stop token)"""
    rs = np.random.RandomState(7000 + case["seed"])
    return rs.randint(0, case["V"] - 1, (case["U"], case["P"])).astype(np.int64)


def case_logits(case, seed):
    """float32 [steps, U * K, V].  Few hot ids per row so that the ids of a sequence repeat (the penalty and the n-gram ban bite)."""
    V, K, U = case["V"], case["K"], case["U"]
    rs = np.random.RandomState(seed)
    nhot = 3 * K
    gap = max(0.45, 0.15 * K)          # level spacing of the hot ids: wider for more beams, whose 2K + 1 candidates would crowd otherwise
    pool = rs.choice(V - 1, size=min(V - 1, nhot + 2), replace=False)          # the hot ids come from one small pool
    out = np.empty((case["steps"], U * K, V), np.float32)
    for s in range(case["steps"]):
        for r in range(U * K):
            x = (rs.standard_normal(V) * 0.5 - 6.0 - gap * nhot).astype(np.float32)
            hot = rs.permutation(pool)[:nhot]
            x[hot] = (4.0 - gap * np.arange(nhot) + rs.uniform(-0.45 * gap, 0.45 * gap, nhot)).astype(np.float32)
            er = case["eos_rank"][s]
            if er == "all":
                x[V - 1] = 14.0
            elif er is not None:
                srt = np.sort(x[:V - 1])[::-1]
                x[V - 1] = srt[0] + 0.3 if er == 0 else 0.5 * (srt[er - 1] + srt[er])
            out[s, r] = x
    return out


def input_hash(logits, prompt):
    h = hashlib.sha1()
    h.update(np.ascontiguousarray(logits).tobytes())
    h.update(np.ascontiguousarray(prompt).tobytes())
    return h.hexdigest()


# ---- the end-to-end cases of tests/golden/gpt_generate_beams.npz: the reference's generate(num_beams=K, do_sample=False) under the synthetic
# weights.  The logits are near-uniform there, so a decode over the whole vocabulary has decision gaps of 1e-5 and less; the cases that
# suppress all ids but the stop token and a handful (as processor_cases' STOPPY does) have wide gaps AND finish hypotheses early.
# E2E_MIN_GAP = 20 x the largest |device - reference| accumulated score over the fixture's steps, measured on the MI355X by
# tests/test_gpu_beam.py's teacher-forced comparison (profiles/beam_measured_errors.txt); the generator keeps only inputs whose smallest
# decision gap (absolute for the 2K + 1 candidates, relative for the finished set) is at least that.
E2E_MIN_GAP = 3.6e-4


def _keep(ids):
    return sorted(set(range(8193)) - set(ids))


_IDS = [5229, 6940, 3850, 6200, 5562, 7829, 411, 1717, 2960, 4243, 7001, 8100, 93, 1208, 3333, 4750, 6061, 7420, 2222, 5005]
E2E_CASES = {
    # (B, K) = (1, 2): the whole vocabulary, no penalty
    "b1k2": dict(U=1, K=2, nrs=2, text_len=[10], prompt_m=0, seed=5, common=dict(repetition_penalty=1.0), beam=dict(length_penalty=1.0)),
    # (2, 3): seven ids left and a decay penalty that lifts the stop token: hypotheses finish early; different text lengths: the utterances' prefix lengths differ
    "b2k3": dict(U=2, K=3, nrs=2, text_len=[10, 7], prompt_m=0, seed=40,
                 common=dict(repetition_penalty=1.0, suppress_tokens=_keep(_IDS[:6]), exponential_decay_length_penalty=(3, 1.4)),
                 beam=dict(length_penalty=1.0, early_stopping=False)),
    # (3, 8): 24 rows, two groups; early_stopping=True
    "b3k8": dict(U=3, K=8, nrs=3, text_len=[9, 12, 6], prompt_m=0, seed=80,
                 common=dict(repetition_penalty=1.0, suppress_tokens=_keep(_IDS), exponential_decay_length_penalty=(2, 1.5)),
                 beam=dict(length_penalty=0.5, early_stopping=True)),
    # (3, 5): 15 rows in one session; the repetition penalty on log-probabilities (it reshuffles the beams at every step)
    "b3k5": dict(U=3, K=5, nrs=5, text_len=[8, 11, 5], prompt_m=0, seed=120,
                 common=dict(repetition_penalty=2.0, suppress_tokens=_keep(_IDS[:14]), exponential_decay_length_penalty=(4, 1.3)),
                 beam=dict(length_penalty=0.5, early_stopping=False)),
    # inference_speech_valle: behind an acoustic prompt of 6 codes
    "valle_b1k3": dict(U=1, K=3, nrs=3, text_len=[10], prompt_m=6, seed=160,
                       common=dict(repetition_penalty=1.0, suppress_tokens=_keep(_IDS[:8]), exponential_decay_length_penalty=(4, 1.3)),
                       beam=dict(length_penalty=2.0, early_stopping="never")),
}
