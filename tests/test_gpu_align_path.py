"""GPU: the monotone-path kernel (csrc/align_path.hip, through Runtime.op_monotone_path) EXACTLY equal to the NumPy fp32 recurrence of
tests/align_inputs.py.  Each cell is one fp32 add plus compares, so there is no tolerance: planted diagonals, staircases with jumps,
constant rows (every prefix maximum a tie: the lowest index wins) and random scores on a 1/8 grid, from 1 x 1 up to the model's limits
(1603 codes x 803 text columns), and ragged n / m in one batch, each row bit-equal to the row run alone."""
import functools

import numpy as np
import pytest

import align_inputs as AI

torch = pytest.importorskip("torch")


@functools.lru_cache(maxsize=None)
def runtime():
    from detail_tts_amd.runtime import Runtime
    return Runtime({}, parts=(), extra={"unused": np.zeros(16, np.float32)})          # the entry reads no weight


@functools.lru_cache(maxsize=None)
def case(kind, n, m):
    s = AI.path_scores(kind, n, m)
    return s, AI.monotone_path(s)


def run(score, n, m):
    return runtime().op_monotone_path(torch.from_numpy(np.ascontiguousarray(score, np.float32)).cuda(), n, m).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", AI.PATH_SIZES, ids=[f"{n}x{m}" for n, m in AI.PATH_SIZES])
@pytest.mark.parametrize("kind", AI.PATH_KINDS)
def test_path_equals_the_numpy_recurrence(kind, n, m):
    s, ref = case(kind, n, m)
    got = run(s[None], [n], [m])
    assert got.shape == (1, n) and got.dtype == np.int32
    assert np.array_equal(got[0], ref), (kind, n, m, np.flatnonzero(got[0] != ref)[:8])
    if kind == "constant":
        assert (got == 0).all()
    assert np.array_equal(run(s[None], [n], [m]), got), "two calls differ"


@pytest.mark.gpu
def test_ragged_batch_rows_equal_the_rows_alone():
    dims = [(65, 257), (1, 5), (0, 3), (300, 200), (64, 64), (5, 1)]
    n_max, m_max = max(d[0] for d in dims), max(d[1] for d in dims)
    batch = np.full((len(dims), n_max, m_max), np.nan, np.float32)      # nothing outside a row's n x m may be read into its path
    for b, (n, m) in enumerate(dims):
        batch[b, :n, :m] = AI.path_scores(AI.PATH_KINDS[b % 4], n, m, seed=b + 1)
    got = run(batch, [d[0] for d in dims], [d[1] for d in dims])
    assert got.shape == (len(dims), n_max)
    for b, (n, m) in enumerate(dims):
        assert (got[b, n:] == -1).all(), b
        assert np.array_equal(got[b, :n], AI.monotone_path(batch[b], n, m)), b
        if n:
            alone = run(np.ascontiguousarray(batch[b:b + 1, :n, :m]), [n], [m])
            assert np.array_equal(alone[0], got[b, :n]), b


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,says", [((2,), (0,), "at least one text column"), ((5,), (3,), "outside [0, max]"), ((2,), (9,), "outside [0, max]")])
def test_bad_sizes_are_refused_before_any_launch(n, m, says):
    from conv_tile_probe import launches_of
    from detail_tts_amd.runtime import DttsError
    rt = runtime()
    score = torch.zeros((1, 4, 8), device="cuda")

    def attempt():
        with pytest.raises(DttsError) as e:
            rt.op_monotone_path(score, n, m)
        return str(e.value)
    msg, ran = launches_of(rt, attempt, level=2)
    assert says in msg and ran == {}, (msg, ran)


@pytest.mark.gpu
def test_more_columns_than_the_model_has_positions_is_refused():
    from detail_tts_amd.runtime import DttsError
    rt = runtime()
    with pytest.raises(DttsError, match="gpt_max_text_pos"):
        rt.op_monotone_path(torch.zeros((1, 2, 804), device="cuda"), [2], [804])
    with pytest.raises(DttsError, match="gpt_max_mel_pos"):
        rt.op_monotone_path(torch.zeros((1, 1604, 2), device="cuda"), [2], [2])
