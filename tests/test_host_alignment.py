"""Host side of the text-to-audio alignment (detail_tts_amd/gpt/alignment.py) on hand-made paths, and the NumPy fp32 monotone path of
tests/align_inputs.py - the reference tests/test_gpu_align_path.py holds the device kernel to - against a brute-force search."""
import numpy as np
import pytest

import align_inputs as AI
from detail_tts_amd.gpt import alignment as A


def test_spans_skips_stays_and_empty_tokens():
    #        codes: 0  1  2  3  4  5  6
    path = [0, 1, 1, 1, 4, 4, 5]
    spans = A.spans_from_path(path, 7, 7)
    assert spans == [(0, 0), (1, 3), None, None, (4, 5), (6, 6), None]
    # only the first n entries of a padded device row count
    assert A.spans_from_path(path + [-1, -1], 7, 7) == spans
    assert A.spans_from_path([2, 2], 2, 3) == [None, None, (0, 1)]


def test_spans_of_an_empty_path_and_bad_paths():
    assert A.spans_from_path([], 0, 4) == [None] * 4
    assert A.spans_from_path([-1, -1], 0, 2) == [None, None]
    with pytest.raises(ValueError):
        A.spans_from_path([0, 2, 1], 3, 4)          # goes back
    with pytest.raises(ValueError):
        A.spans_from_path([0, 4], 2, 4)             # leaves the text
    with pytest.raises(ValueError):
        A.spans_from_path([0], 2, 4)                # too short


def test_token_times_cover_whole_codes():
    t = A.token_times([(0, 0), None, (1, 3)], 1024, 24000)
    assert t[1] is None
    assert t[0] == (0.0, 1024 / 24000) and t[2] == (1024 / 24000, 4 * 1024 / 24000)


def test_group_words_merges_tokens_between_spaces():
    SP = 2
    ids = [SP, 10, 11, SP, SP, 12, SP, 13, 14]
    spans = [None, (0, 1), (2, 2), (3, 3), None, None, (4, 4), (5, 6), None]
    words = A.group_words(ids, spans, SP)
    assert [w["tokens"] for w in words] == [[1, 2], [5], [7, 8]]
    assert [w["span"] for w in words] == [(0, 2), None, (5, 6)]
    assert A.group_words([], [], SP) == []
    with pytest.raises(ValueError):
        A.group_words([1, 2], [None], SP)


def test_alignment_stats_report_skips_and_the_longest_stay():
    # 4 text tokens -> columns 1 .. 4 of 6; token 1 (column 2) and token 3 (column 4) are skipped
    path = [0, 1, 1, 1, 1, 3, 3, 5]
    st = A.alignment_stats(path, 8, 4, text_mass=[0.5] * 8 + [9.0])
    assert st["skipped"] == [1, 3] and st["coverage"] == 0.5 and st["longest_stay"] == 4
    assert st["mean_text_mass"] == pytest.approx(0.5)
    empty = A.alignment_stats([], 0, 3)
    assert empty == dict(coverage=0.0, skipped=[0, 1, 2], longest_stay=0, mean_text_mass=None)
    assert A.alignment_stats([0, 1], 2, 0)["coverage"] == 1.0


def test_describe_puts_it_together():
    d = A.describe([0, 1, 1, 3, -1], 4, [7, 2, 9], [1.0, 1.0, 0.5, 0.5], 1024, 24000, space_id=2)
    assert d["path"].tolist() == [0, 1, 1, 3] and d["token_spans"] == [(1, 2), None, (3, 3)]
    assert [w["tokens"] for w in d["words"]] == [[0], [2]]
    assert d["words"][1]["time"] == (3 * 1024 / 24000, 4 * 1024 / 24000)
    assert d["stats"]["skipped"] == [1] and d["stats"]["mean_text_mass"] == pytest.approx(0.75)


@pytest.mark.parametrize("n,m", [(n, m) for n in range(1, 6) for m in range(1, 6)])
def test_numpy_path_against_brute_force(n, m):
    rs = np.random.RandomState(10 * n + m)
    for trial in range(6):
        # multiples of 1/4: every sum is exact in fp32 and in float64, ties are real ties
        s = (rs.randint(-8, 9, (n, m)) / 4.0).astype(np.float32) if trial % 2 else rs.randn(n, m).astype(np.float32)
        p = AI.monotone_path(s)
        best, paths = AI.brute_force_path_score(s)
        assert tuple(p.tolist()) in paths, (s, p, paths)
        assert (np.diff(p) >= 0).all()


def test_numpy_path_ties_go_to_the_lowest_index_and_ragged_arguments():
    assert AI.monotone_path(np.zeros((4, 5), np.float32)).tolist() == [0, 0, 0, 0]
    s = AI.path_scores("constant", 5, 7)
    assert AI.monotone_path(s).tolist() == [0] * 5
    s = np.array([[0, 1, 1], [0, 0, 0], [0, 0, 2]], np.float32)
    # row 0's maximum is tied between columns 1 and 2 -> 1; row 1 from there: column 1 or 2 (0 each) -> 1; row 2: column 2
    assert AI.monotone_path(s).tolist() == [1, 1, 2]
    big = np.full((6, 6), -9.0, np.float32)
    big[:3, :4] = AI.path_scores("random", 3, 4)
    assert AI.monotone_path(big, 3, 4).tolist() == AI.monotone_path(big[:3, :4]).tolist()
    assert AI.monotone_path(big, 0, 4).shape == (0,)


def test_peaked_weights_scale_q_and_k_only():
    C = 4
    st = {"gpt.gpt.h.0.attn.c_attn.weight": np.ones((C, 3 * C), np.float32), "gpt.gpt.h.0.attn.c_attn.bias": np.ones((3 * C,), np.float32),
          "other": np.ones(3, np.float32)}
    out = AI.peaked_gpt_weights(st, 4.0)
    assert (out["gpt.gpt.h.0.attn.c_attn.weight"][:, : 2 * C] == 4).all() and (out["gpt.gpt.h.0.attn.c_attn.weight"][:, 2 * C:] == 1).all()
    assert (out["gpt.gpt.h.0.attn.c_attn.bias"][: 2 * C] == 4).all() and (out["gpt.gpt.h.0.attn.c_attn.bias"][2 * C:] == 1).all()
    assert (st["gpt.gpt.h.0.attn.c_attn.weight"] == 1).all() and out["other"] is st["other"]


def test_probs_reference_rows_sum_to_one_and_mutations_move_it():
    c = AI.probs_case(65, "block")
    P = AI.probs_reference(c["q"][0], c["k"][0], 65, c["scale"])
    assert np.allclose(P.sum(axis=2), 1.0, atol=1e-12) and (np.triu(P[0], 1) == 0).all()
    tab = AI.probs_mutation_table([c])
    assert set(tab) == set(AI.PROBS_MUTATIONS) and min(tab.values()) > 0.1, tab
