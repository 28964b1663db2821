"""CPU: the speaking-rate frame plan (detail_tts_amd/duration.py) - the uniform map against torch's own F.interpolate, durations and
span_rates against their restatement (tests/duration_ref.py), every refusal, and which call stage B makes without a plan.
No GPU, no library."""
import numpy as np
import pytest

import duration_ref as R

torch = pytest.importorskip("torch")

from detail_tts_amd import duration as D  # noqa: E402

GRID = sorted(set(R.HARD_PAIRS) | {(n, 4 * n) for n in (1, 6, 12, 14, 26)} |
              {(n, T) for n in (1, 6, 7, 13, 26) for T in (4, 8, 12, 28, 52, 104, 148, 416)})


def torch_map(n, T):
    return torch.nn.functional.interpolate(torch.arange(n, dtype=torch.float32).view(1, 1, n), size=T, mode="nearest").view(-1).long().numpy()


def test_uniform_map_is_torchs_rule():
    for n, T in GRID:
        want = torch_map(n, T)
        assert np.array_equal(R.uniform_map(n, T), want), (n, T)
        assert np.array_equal(D.uniform_map(n, T), want), (n, T)
    for n in (1, 6, 12, 14, 26):                                   # at T = 4 n the rule is t // 4
        assert np.array_equal(D.uniform_map(n, 4 * n), np.arange(4 * n) // 4)


def test_integer_floor_is_not_torchs_rule():
    """what makes the test above mean something: at these pairs floor(t n / T) is a different map, at exactly the listed frames"""
    for (n, T), frames in R.HARD_FRAMES.items():
        want, wrong = torch_map(n, T), R.floor_map(n, T)
        assert tuple(np.nonzero(want != wrong)[0].tolist()) == frames, (n, T)
        assert all(wrong[t] == want[t] + 1 for t in frames)


def test_speed_plan():
    for n, s, T in ((14, 1.0, 56), (14, 0.6, 92), (26, 2.4, 44), (12, 0.25, 192), (12, 4.0, 12), (1, 4.0, 4), (6, 1.7, 16), (7, 1.7, 16)):
        assert D.speed_frames(n, s) == R.speed_frames(n, s) == T
    plan = D.make_plan([14, 26, 6], D.check_request(speed=[0.6, 2.4, 1.0], B=3))
    assert plan.frames == [92, 44, 24] and plan.durations is None and plan.extended == [0, 0, 0] and plan.Tmax == 92
    for b, (n, T) in enumerate(((14, 92), (26, 44), (6, 24))):
        assert np.array_equal(plan.row_map(b), R.uniform_map(n, T))
    plan = D.make_plan([14, 26], D.check_request(speed=0.6, B=2))
    assert plan.frames == [92, 172]
    assert all(T % 4 == 0 for s in np.linspace(0.25, 4.0, 41) for n in (1, 6, 26) for T in [D.speed_frames(n, s)])


def test_no_plan_is_no_plan():
    assert D.check_request() is None and D.make_plan([5, 6], None) is None
    assert D.check_request(speed=None, B=2) is None
    assert D.check_request(speed=1.0, B=2) is None and D.check_request(speed=1, B=2) is None
    assert D.check_request(speed=[1.0, 1.0], B=2) is None and D.check_request(speed=torch.tensor(1.0), B=2) is None
    assert D.check_request(speed=[1.0, 0.5], B=2) == dict(speed=[1.0, 0.5])


def test_durations_against_repeat():
    codes = [np.zeros(n, np.int64) for n in (6, 8, 7)]
    rows = [[0, 3, 0, 0, 5, 0], [4] * 8, [0, 0, 0, 9, 0, 0, 0]]     # leading, inner and trailing zeros | already 4 n | one code owns all
    plan = D.make_plan([6, 8, 7], D.check_request(durations=rows, forced_codes=codes, B=3))
    assert plan.frames == [8, 32, 12] and plan.extended == [0, 0, 3] and plan.durations.shape == (3, 8) and plan.durations.dtype == np.int32
    for b, d in enumerate(rows):
        padded, ext = R.pad_durations(d)
        assert ext == plan.extended[b] and plan.durations[b].tolist() == padded.tolist() + [0] * (8 - len(d))
        assert np.array_equal(plan.row_map(b), np.repeat(np.arange(len(d)), padded)) and len(plan.row_map(b)) == plan.frames[b]
    assert plan.durations[2].tolist() == [0, 0, 0, 12, 0, 0, 0, 0]                         # the LAST POSITIVE one is extended
    plan = D.make_plan([3], D.check_request(durations=[torch.tensor([1, 0, 0])], forced_codes=[[1, 2, 3]], B=1))
    assert plan.frames == [4] and plan.durations.tolist() == [[4, 0, 0]] and plan.extended == [3]
    # the bounds of the frame-based times: an empty interval for a code without a frame
    m = plan.row_map(0)
    assert plan.code_bounds(0).tolist() == [0, 4, 4, 4] == [R.code_interval(m, 0)[0]] + [R.code_interval(m, j)[1] for j in range(3)]


def test_span_rates_distribution_sums_exactly():
    rs = np.random.RandomState(0)
    for _ in range(200):
        n = int(rs.randint(6, 27))
        a = int(rs.randint(0, n))
        b = int(rs.randint(a, n))
        rate = float(rs.uniform(0.25, 4.0))
        d = D.span_durations(n, [(a, b, rate)])
        L = b - a + 1
        F = max(1, int(4 * L / rate + 0.5))
        assert d.tolist() == R.span_durations(n, [(a, b, rate)]).tolist()
        assert int(d[a:b + 1].sum()) == F and (d[:a] == 4).all() and (d[b + 1:] == 4).all()
        assert d[a:b + 1].max() - d[a:b + 1].min() <= 1 and d.min() >= 0
    d = D.span_durations(12, [(0, 2, 0.5), (5, 5, 4.0), (8, 11, 4.0)])
    assert d.tolist() == [8, 8, 8, 4, 4, 1, 4, 4, 1, 1, 1, 1]
    assert D.span_durations(6, [(0, 5, 4.0)]).tolist() == [1] * 6 and D.span_durations(6, []).tolist() == [4] * 6
    plan = D.make_plan([12], D.check_request(span_rates=[[(0, 2, 0.5), (5, 5, 4.0), (8, 11, 4.0)]], forced_codes=[np.zeros(12)], B=1))
    assert plan.frames == [48] and plan.extended == [3] and plan.durations[0].tolist() == [8, 8, 8, 4, 4, 1, 4, 4, 1, 1, 1, 4]
    assert D.span_durations(8, [(2, 5, 3.0)])[2:6].tolist() == [1, 1, 1, 2]                  # F = 5 over 4 codes: (j + 1) F // L - j F // L


def test_refusals():
    codes = [np.zeros(6), np.zeros(8)]
    bad = [
        dict(speed=0.2, B=2), dict(speed=4.5, B=2), dict(speed=float("nan"), B=2), dict(speed="fast", B=2), dict(speed=True, B=2),
        dict(speed=[1.0], B=2), dict(speed=[1.0, 9.0], B=2),
        dict(speed=1.0, durations=[[4] * 6, [4] * 8], forced_codes=codes, B=2),                # at most one of the three
        dict(speed=0.5, span_rates=[[], []], forced_codes=codes, B=2),
        dict(durations=[[4] * 6, [4] * 8], span_rates=[[], []], forced_codes=codes, B=2),
        dict(durations=[[4] * 6, [4] * 8], B=2),                                                # durations need forced_codes
        dict(span_rates=[[], []], B=2),
        dict(durations=[[4] * 6], forced_codes=codes, B=2),                                     # a row count
        dict(durations=[[4] * 6, [4] * 7], forced_codes=codes, B=2),                            # a length mismatch with the row's codes
        dict(durations=[[4] * 6, [4] * 7 + [-1]], forced_codes=codes, B=2),
        dict(durations=[[4] * 6, [0] * 8], forced_codes=codes, B=2),                            # none positive
        dict(durations=[[4] * 6, [1.5] * 8], forced_codes=codes, B=2),
        dict(durations=[[4] * 6, [4] * 8], forced_codes=codes, B=3),
        dict(span_rates=[[(0, 6, 1.0)], []], forced_codes=codes, B=2),                          # outside [0, n)
        dict(span_rates=[[(-1, 2, 1.0)], []], forced_codes=codes, B=2),
        dict(span_rates=[[(3, 2, 1.0)], []], forced_codes=codes, B=2),
        dict(span_rates=[[(0, 2, 1.0), (2, 4, 2.0)], []], forced_codes=codes, B=2),             # not disjoint
        dict(span_rates=[[(0, 2, 0.1)], []], forced_codes=codes, B=2),                          # the rate
        dict(span_rates=[[(0, 2, 5.0)], []], forced_codes=codes, B=2),
        dict(span_rates=[[(0, 2)], []], forced_codes=codes, B=2),
        dict(span_rates=[[]], forced_codes=codes, B=2),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            D.check_request(**kw)
    with pytest.raises(ValueError, match="forced_codes"):
        D.check_request(durations=[[4] * 6, [4] * 8], B=2)
    with pytest.raises(ValueError):
        D.make_plan([6, 8, 3], dict(speed=[0.5, 0.5]))
    with pytest.raises(ValueError):
        D.make_plan([6, 9], dict(durations=[np.full(6, 4), np.full(8, 4)]))
    for n, T in ((0, 4), (4, 0)):
        with pytest.raises(ValueError):
            D.uniform_map(n, T)


def test_request_normalisation_refuses_before_any_launch_and_carries_the_rate():
    from detail_tts_amd.pipeline import normalize_request
    text = torch.tensor([[5, 6, 7, 0], [8, 9, 0, 0]])
    refer = np.zeros((2, 128, 9), np.float32)
    codes = [np.arange(6), np.arange(8)]
    args = (text, [4, 3], refer, [9, 7])
    assert normalize_request(*args).rate is None and normalize_request(*args, speed=1.0).rate is None
    assert normalize_request(*args, speed=0.5).rate == dict(speed=[0.5, 0.5])
    assert normalize_request(*args, speed=[0.5, 2.0], batch=False).rate == dict(speed=[0.5])
    st = normalize_request(*args, forced_codes=codes, span_rates=[[(1, 2, 2.0)], []])
    assert [d.tolist() for d in st.rate["durations"]] == [[4, 2, 2, 4, 4, 4], [4] * 8]
    st = normalize_request(*args, forced_codes=codes, durations=[[1] * 6, [2] * 8], batch=False)
    assert len(st.rate["durations"]) == 1 and st.plan is None
    for kw in (dict(speed=9.0), dict(durations=[[4] * 6, [4] * 8]), dict(forced_codes=codes, durations=[[4] * 6, [4] * 7]),
               dict(speed=0.5, forced_codes=codes, span_rates=[[], []])):
        with pytest.raises(ValueError):
            normalize_request(*args, **kw)


class _StubRuntime:
    """records stage B's calls; returns tokens in the place of tensors"""

    def __init__(self):
        self.calls = []

    def diff_conditioning(self, refer, rl):
        return "cond"

    def diff_timestep_independent(self, *a, **kw):
        self.calls.append(("emb", a, kw))
        return "emb"

    def sampler_schedule(self, ts, sampler):
        return 0

    def diff_sample_ex(self, code_emb, seed, sids, **kw):
        self.calls.append(("sample", (code_emb, seed, sids), kw))
        return "mel"


class _StubModel:
    def __init__(self):
        self.rt = _StubRuntime()

    def _trunk_precision(self, prec):
        import contextlib
        return contextlib.nullcontext()


@pytest.mark.parametrize("speed", [None, 1.0, [1.0, 1.0]])
def test_without_a_plan_stage_b_takes_the_existing_call(speed):
    """speed None and speed 1.0: the embedding call of before - positional (lat, cond, n), no frames keyword - and 4 frames per code"""
    from detail_tts_amd.pipeline import normalize_request, stage_b
    st = normalize_request(torch.tensor([[5, 6, 0], [8, 0, 0]]), [3, 2], np.zeros((2, 128, 9), np.float32), [9, 7], seed=3, speed=speed)
    st.lat, st.n = "lat", [6, 9]
    m = _StubModel()
    mel, lens_t = stage_b(m, st, 0, 0.0, None, sched_ts=None)
    assert m.rt.calls[0] == ("emb", ("lat", "cond", [6, 9]), {}) and st.plan is None
    assert mel == "mel" and lens_t == [24, 36] and m.rt.calls[1][2]["lens"] == [24, 36]


def test_with_a_plan_stage_b_hands_the_frames_on():
    from detail_tts_amd.pipeline import normalize_request, stage_b
    st = normalize_request(torch.tensor([[5, 6, 0], [8, 0, 0]]), [3, 2], np.zeros((2, 128, 9), np.float32), [9, 7], seed=3, speed=[0.6, 2.4])
    st.lat, st.n = "lat", [14, 26]
    m = _StubModel()
    mel, lens_t = stage_b(m, st, 0, 0.0, None, sched_ts=None)
    assert m.rt.calls[0] == ("emb", ("lat", "cond", [14, 26]), dict(frames=[92, 44], durations=None))
    assert lens_t == [92, 44] and m.rt.calls[1][2]["lens"] == [92, 44] and st.plan.frames == [92, 44]


def test_frame_based_times_beside_token_times():
    from detail_tts_amd.gpt.alignment import describe, token_times, token_times_frames
    n, ids = 6, np.array([7, 8, 2, 9, 0])
    path = np.array([1, 1, 2, 4, 4, 6])
    plain = describe(path, n, ids, None, 1024, 24000, space_id=2)
    assert plain["token_times"] == token_times(plain["token_spans"], 1024, 24000)               # without a plan: as before
    same = describe(path, n, ids, None, 1024, 24000, space_id=2, frame_bounds=np.arange(7) * 4)   # the x4 map gives the same times
    assert same["times"] == plain["times"] and same["token_times"] == plain["token_times"] and same["words"] == plain["words"]
    d = np.array([0, 3, 0, 0, 5, 0])
    m = R.durations_map(d)
    bounds = D.code_bounds(m, n)
    got = describe(path, n, ids, None, 1024, 24000, space_id=2, frame_bounds=bounds)
    assert got["spans"] == plain["spans"] and got["stats"] == plain["stats"]
    for key in ("times", "token_times"):
        assert got[key] == [R.span_time(m, s) for s in got["spans" if key == "times" else "token_spans"]]
    assert [w["time"] for w in got["words"]] == [R.span_time(m, w["span"]) for w in got["words"]]
    assert got["times"][2] == (3 * 256 / 24000, 3 * 256 / 24000)                                 # code 2 owns no frame: an empty interval
    assert token_times_frames([(0, 5), None], bounds, 256, 24000) == [(0.0, 8 * 256 / 24000), None]
