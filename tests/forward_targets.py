"""Helper of the loss-mode forward tests and of tests/golden/make_golden_forward.py (not a test module): the padded inputs and the targets
that dtts_gpt_forward_losses feeds and scores for given (text [B, Lt], codes [B, n]) after clip_inputs / set_mel_padding.  The device
builds them in C++ (Model::gpt_forward_losses); this is the same rule in numpy, for gathering expected log-probabilities."""
import numpy as np


def aligned_inputs_and_targets(text, codes, start_text_token=255, stop_text_token=0, start_mel_token=8192, stop_mel_token=8193):
    """-> (text_in [B, Lt+2] = [start, text, stop], text_tgt = [text, stop, stop], mel_in [B, n+2] = [start, codes, stop],
    mel_tgt = [codes, stop, stop])"""
    def one(a, start, stop):
        a = np.asarray(a, np.int64)
        B = a.shape[0]
        col = lambda v: np.full((B, 1), v, np.int64)
        return np.concatenate([col(start), a, col(stop)], 1), np.concatenate([a, col(stop), col(stop)], 1)
    ti, tt = one(text, start_text_token, stop_text_token)
    mi, mt = one(codes, start_mel_token, stop_mel_token)
    return ti, tt, mi, mt
