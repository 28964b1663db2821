"""NumPy restatement of the speaking-rate frame plan (detail_tts_amd/duration.py, csrc/frame_map.hip), written from the issue's text
and independent of the package: the plan (frame counts), both frame -> code maps - the float32 rule of F.interpolate(mode='nearest')
spelled out operation by operation - and the frame-based alignment times."""
import numpy as np

# (n, T) with T % 4 == 0 at which floor(t n / T) is NOT torch's map: t n / T is an integer there and the float32 scale falls below n / T
HARD_PAIRS = ((14, 92), (26, 44), (20, 108), (12, 148), (6, 148))
HARD_FRAMES = {(14, 92): (46,), (26, 44): (22,), (20, 108): (81,), (12, 148): (37, 74), (6, 148): (74,)}


def uniform_map(n, T):
    """scale = float(n) / float(T);  m[t] = min((int)floorf(float(t) * scale), n - 1) - every operation in float32, rounded once"""
    scale = np.float32(np.float32(n) / np.float32(T))
    out = np.empty(T, np.int64)
    for t in range(T):
        prod = np.float32(np.float32(t) * scale)
        assert prod.dtype == np.float32
        out[t] = min(int(np.floor(prod)), n - 1)
    return out


def floor_map(n, T):
    """the exact integer rule t n // T: what the device must NOT compute"""
    return np.arange(T, dtype=np.int64) * n // T


def speed_frames(n, speed):
    return max(4, 4 * int(np.float64(n) / np.float64(speed) + 0.5))


def pad_durations(d):
    """durations -> (durations with the last positive one extended to a multiple of 4 in the sum, the extension)"""
    d = np.array(d, np.int64)
    ext = (-int(d.sum())) % 4
    last = max(j for j in range(d.size) if d[j] > 0)
    d[last] += ext
    return d, ext


def durations_map(d):
    return np.repeat(np.arange(len(d), dtype=np.int64), np.asarray(d, np.int64))


def span_durations(n, spans):
    d = [4] * n
    for a, b, rate in spans:
        L = b - a + 1
        F = max(1, int(np.float64(4 * L) / np.float64(rate) + 0.5))
        for j in range(L):
            d[a + j] = (j + 1) * F // L - j * F // L
    return np.asarray(d, np.int64)


def padded_maps(maps, Tmax):
    """row maps -> int32 [B, Tmax], -1 beyond a row's frames: what dtts_op_frame_map writes"""
    out = np.full((len(maps), Tmax), -1, np.int32)
    for b, m in enumerate(maps):
        out[b, : len(m)] = m
    return out


def code_interval(m, j):
    """code j covers frames [first t with m[t] >= j, first t with m[t] >= j + 1); T where there is none"""
    T = len(m)
    first = lambda v: next((t for t in range(T) if m[t] >= v), T)  # noqa: E731
    return first(j), first(j + 1)


def span_time(m, span, sampling_rate=24000, samples_per_frame=256):
    """an inclusive code span (first, last) -> (start, end) seconds under the map m"""
    if span is None:
        return None
    k = samples_per_frame / sampling_rate
    return code_interval(m, span[0])[0] * k, code_interval(m, span[1])[1] * k
