"""CPU: the request bookkeeping of SynthesizerTrn.infer / infer_stream (detail_tts_amd/pipeline.py) - which requests share a decode
session, how far ahead the request iterator is read, how a shared session's rows are merged and split back, request normalisation.
No GPU, no library."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from detail_tts_amd.pipeline import Request, group_requests, merge_session, normalize_request, split_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [2, 6, 3, 9, 8, 1, 2]


def _reqs(rows):
    return [dict(text=np.zeros((B, 3), np.int32), i=i) for i, B in enumerate(rows)]


def _ids(groups):
    return [[r["i"] for r in g] for g in groups]


def test_grouping_pairs_consecutive_small_requests():
    assert _ids(group_requests(iter(_reqs(ROWS)), True)) == [[0, 1], [2], [3], [4, 5], [6]]      # 3 | 9: 9 > 8; 8 + 1 share
    assert _ids(group_requests(iter(_reqs(ROWS)), False)) == [[i] for i in range(7)]
    assert _ids(group_requests(_reqs(ROWS))) == [[i] for i in range(7)]                           # pairing is off by default
    assert list(group_requests(iter([]), True)) == [] and list(group_requests(iter([]), False)) == []


@pytest.mark.parametrize("pair", [True, False])
def test_grouping_reads_at_most_two_requests_ahead(pair):
    pulled = [0]

    def source():
        for r in _reqs(ROWS):
            pulled[0] += 1
            yield r

    done = 0
    for g in group_requests(source(), pair):
        done += len(g)                      # requests up to and including this group
        assert pulled[0] - done <= 2
    assert done == pulled[0] == len(ROWS)


def _request(B, seed, first_id, forced=False):
    rs = np.random.RandomState(seed)
    return Request(B=B, rl=[40 + seed + b for b in range(B)], seed=seed, sids=[first_id + b for b in range(B)],
                   texts=[rs.randint(3, 255, 4 + b).astype(np.int32) for b in range(B)], refer=None,
                   forced=[rs.randint(0, 8192, 5 + b) for b in range(B)] if forced else None)


def test_merge_concatenates_rows_in_order_with_per_row_seeds():
    a, b = _request(2, 11, 100), _request(3, 22, 200)
    rl, texts, sids, seeds, forced = merge_session([a, b])
    assert rl == a.rl + b.rl and sids == [100, 101, 200, 201, 202] and seeds == [11, 11, 22, 22, 22] and forced is None
    assert len(texts) == 5 and all(t is u for t, u in zip(texts, a.texts + b.texts))
    a, b = _request(2, 11, 100, forced=True), _request(3, 22, 200, forced=True)
    forced = merge_session([a, b])[4]
    assert len(forced) == 5 and all(c is d for c, d in zip(forced, a.forced + b.forced))


def test_merge_refuses_forced_codes_in_one_request_only():
    with pytest.raises(AssertionError, match="forced_codes"):
        merge_session([_request(2, 11, 100, forced=True), _request(3, 22, 200)])
    with pytest.raises(AssertionError, match="forced_codes"):
        merge_session([_request(2, 11, 100), _request(3, 22, 200, forced=True)])


def test_merge_of_one_request_passes_its_scalar_seed_through():
    a = _request(3, 77, 5, forced=True)
    rl, texts, sids, seeds, forced = merge_session([a])
    assert seeds == 77 and rl == a.rl and sids == a.sids and len(texts) == 3 and len(forced) == 3


def test_split_gives_each_request_its_code_counts():
    assert split_session(np.array([5, 3, 4, 4, 2], np.int32), [2, 3]) == [[4, 2], [3, 3, 1]]
    assert split_session([7], [1]) == [[6]]
    for bad in ([5, 1, 4, 4, 2], [5, 3, 4, 4, 1], [1]):
        with pytest.raises(ValueError, match="no mel codes"):
            split_session(np.array(bad, np.int32), [2, 3] if len(bad) == 5 else [1])


def test_normalisation():
    text = torch.tensor([[5, 6, 7, 0, 0], [8, 9, 0, 0, 0], [3, 4, 5, 6, 0]], dtype=torch.long)
    refer = np.zeros((3, 128, 9), np.float32)
    st = normalize_request(text, torch.tensor([4, 3, 5]), refer, torch.tensor([9, 7, 8]))
    assert st.B == 3 and st.rl == [9, 7, 8] and all(type(v) is int for v in st.rl) and st.sids == [0, 1, 2] and st.forced is None
    assert isinstance(st.seed, int) and 0 <= st.seed < 2 ** 62
    assert [t.tolist() for t in st.texts] == [[5, 6, 7, 0], [8, 9, 0], [3, 4, 5, 6, 0]] and all(t.dtype == np.int32 for t in st.texts)
    assert tuple(st.refer.shape) == (3, 128, 9) and st.refer.device.type == "cpu"          # no transfer: stage A's stream makes it
    assert normalize_request(text, [4, 3, 5], refer, [9, 7, 8]).seed != st.seed               # drawn, not a constant
    codes = [np.arange(3), np.arange(4), np.arange(5)]
    st = normalize_request(text, [4, 3, 5], refer, [9, 7, 8], seed=12, sample_ids=(7, 8, 9), forced_codes=codes)
    assert st.seed == 12 and st.sids == [7, 8, 9] and st.forced is codes
    st = normalize_request(text, [4, 3, 5], refer, [9, 7, 8], seed=12, forced_codes=codes, batch=False)      # the reference's first row only
    assert st.B == 1 and st.rl == [9] and st.sids == [0] and len(st.texts) == 1 and len(st.forced) == 1 and st.refer.shape[0] == 1


def test_removed_knobs_are_gone_from_the_source():
    for rel in ("detail_tts_amd/pipeline.py", "detail_tts_amd/vqvae/model_24k.py"):
        src = open(os.path.join(ROOT, rel)).read()
        for name in ("DTTS_EXPERIMENT", "DTTS_SERIAL_VOCODER", "DTTS_STAGE_A_PRIORITY", "DTTS_PAIR_STAGE_A"):
            assert name not in src, (rel, name)
