"""Host logic of best-of-N code candidates (detail_tts_amd/gpt/candidates.py) and infer()'s argument checks: no GPU, no library."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from detail_tts_amd.gpt.candidates import CANDIDATE_STREAM_STRIDE, expand_sample_ids, rank_candidates  # noqa: E402


def test_score_is_the_mean_not_the_sum():
    # candidate 0: 2 tokens of -3 (sum -6, mean -3); candidate 1: 10 tokens of -1 (sum -10, mean -1): the mean prefers 1, a sum would prefer 0
    lp = [np.full(12, -3.0, np.float32), np.full(12, -1.0, np.float32)]
    best, scores = rank_candidates(lp, [2, 10], [True, True])
    assert best == 1 and scores.dtype == np.float64
    np.testing.assert_allclose(scores, [-3.0, -1.0])
    # entries beyond ncodes are ignored (the device writes 0.0 there, which would lift a mean taken over the padded row)
    row = np.array([-4.0, -4.0, 0.0, 0.0], np.float32)
    _, scores = rank_candidates([row, row], [2, 4], [False, False])
    np.testing.assert_allclose(scores, [-4.0, -2.0])


def test_stopped_candidates_rank_first():
    lp = [np.full(4, -1.0), np.full(4, -9.0), np.full(4, -8.0)]
    best, _ = rank_candidates(lp, [4, 4, 4], [False, True, True])      # the likeliest candidate never stopped
    assert best == 2
    best, _ = rank_candidates(lp, [4, 4, 4], [False, False, False])    # nobody stopped: plain likelihood
    assert best == 0


def test_ties_go_to_the_lowest_index():
    lp = [np.full(3, -2.0), np.full(3, -2.0), np.full(3, -2.0)]
    assert rank_candidates(lp, [3, 3, 3], [True, True, True])[0] == 0
    assert rank_candidates(lp, [3, 3, 3], [False, True, True])[0] == 1
    with pytest.raises(ValueError):
        rank_candidates(lp, [3, 0, 3], [True, True, True])
    with pytest.raises(ValueError):
        rank_candidates(lp, [3, 3], [True, True])


def test_expanded_sample_ids_and_collisions():
    assert CANDIDATE_STREAM_STRIDE == 2 ** 20
    assert expand_sample_ids([31, 32], 3) == [31, 31 + 2 ** 20, 31 + 2 ** 21, 32, 32 + 2 ** 20, 32 + 2 ** 21]
    assert expand_sample_ids([7], 1) == [7]                            # candidate 0 is the single-candidate decode
    with pytest.raises(ValueError, match="noise stream"):
        expand_sample_ids([0, 2 ** 20], 2)                            # utterance 0's candidate 1 == utterance 1's candidate 0
    with pytest.raises(ValueError, match="noise stream"):
        expand_sample_ids([5, 5], 1)
    with pytest.raises(ValueError):
        expand_sample_ids([2 ** 31 - 5], 2)                           # leaves the int32 ids of the C ABI


class _NoDevice:
    """a model whose runtime must never be touched"""
    @property
    def rt(self):
        raise AssertionError("device work before the arguments were checked")


def test_infer_argument_checks_raise_before_any_device_call():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    text = torch.zeros((2, 4), dtype=torch.long)
    refer = torch.zeros((2, 128, 8))
    args = (text, [4, 4], refer, [8, 8])
    for bad in (0, 17, -1, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="num_candidates"):
            SynthesizerTrn.infer(_NoDevice(), *args, batch=True, num_candidates=bad)
    with pytest.raises(ValueError, match="forced_codes"):
        SynthesizerTrn.infer(_NoDevice(), *args, batch=True, num_candidates=2, forced_codes=[np.arange(3), np.arange(3)])
    with pytest.raises(ValueError, match="forced_codes"):
        SynthesizerTrn.infer(_NoDevice(), *args, batch=True, return_candidates=True, forced_codes=[np.arange(3), np.arange(3)])
    for bad in ([0], [0, 3], [0, -1], [0, 0, 0]):
        with pytest.raises(ValueError, match="choose"):
            SynthesizerTrn.infer(_NoDevice(), *args, batch=True, num_candidates=3, choose=bad)
    with pytest.raises(ValueError, match="choose"):
        SynthesizerTrn.infer(_NoDevice(), *args, batch=True, choose=[1, 0])          # N = 1 has candidate 0 only
    with pytest.raises(ValueError, match="noise stream"):
        SynthesizerTrn.infer(_NoDevice(), *args, batch=True, num_candidates=2, sample_ids=[0, 2 ** 20])
