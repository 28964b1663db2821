"""numpy restatement of csrc/wav_join.hip.  Edges: frame energies in float64 (the kernel sums in float32: the tests plant frames whose
RMS is far from the threshold on either side, so both decide alike).  Join: fade weights and products in float32 exactly as the kernel
forms them - ONE division of two integers float32 holds exactly, one product - and pauses of exact +0.0."""
import numpy as np

F32 = np.float32


def frame_rms(row, n, frame=256):
    """float64 RMS of every frame of row[:n]; the last frame may be partial"""
    x = np.asarray(row[:n], np.float64)
    return np.array([np.sqrt(np.mean(x[a: a + frame] ** 2)) for a in range(0, n, frame)], np.float64)


def edges(wav, lens, *, frame=256, threshold, keep=0):
    """wav [B, stride], lens [B] -> int32 [B, 2] = (begin, end); a row with no loud frame: (0, 0).  Samples at or beyond lens[b] unread."""
    out = np.zeros((len(lens), 2), np.int32)
    for b, n in enumerate(lens):
        n = int(n)
        x = np.asarray(wav[b, :n], np.float64)
        loud = [f for f, a in enumerate(range(0, n, frame))
                if np.sum(x[a: a + frame] ** 2) >= float(threshold) ** 2 * len(x[a: a + frame])]
        if loud:
            out[b] = max(0, loud[0] * frame - keep), min(n, (loud[-1] + 1) * frame + keep)
    return out


def weights(count, fade):
    """float32 [count]: (2 i + 1) / (2 n) over the first n = min(fade, count // 2) samples, the mirror image over the last n, 1 between"""
    n = min(int(fade), count // 2)
    w = np.ones(count, F32)
    for i in range(n):
        w[i] = w[count - 1 - i] = F32(2 * i + 1) / F32(2 * n)
    return w


def join(wav, begins, counts, offsets, total, *, fade):
    """out[offsets[b] + i] = wav[b, begins[b] + i] w_b(i), i < counts[b]; every other sample +0.0.  Where the weight is 1 the
    sample's own bits are copied."""
    out = np.zeros(int(total), F32)
    for b, (s, c, o) in enumerate(zip(begins, counts, offsets)):
        s, c, o = int(s), int(c), int(o)
        x = np.asarray(wav[b, s: s + c], F32)
        n = min(int(fade), c // 2)
        y = x.copy()
        w = weights(c, fade)
        y[:n] = x[:n] * w[:n]
        if n:
            y[c - n:] = x[c - n:] * w[c - n:]
        out[o: o + c] = y
    return out


def join_plan(wavs, lens, kinds, pauses, *, fade, edge_list=None):
    """the whole long-form output of chunks given one by one: wavs[k] a 1-D waveform, lens[k] its sample count, kinds[k] how it ended,
    pauses {kind: samples}; edge_list[k] = (begin, end) or None (nothing trimmed) -> (float32 [N], offsets [K])"""
    parts, offsets, at = [], [], 0
    for k, (w, n, kind) in enumerate(zip(wavs, lens, kinds)):
        b, e = (0, int(n)) if edge_list is None else (int(edge_list[k][0]), int(edge_list[k][1]))
        pause = 0 if kind == "end" else int(pauses[kind])
        seg = join(np.asarray(w, F32)[None, :], [b], [e - b], [0], e - b + pause, fade=fade)
        parts.append(seg)
        offsets.append(at)
        at += len(seg)
    return (np.concatenate(parts) if parts else np.zeros(0, F32)), offsets
