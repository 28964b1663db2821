"""numpy float32 restatement of csrc/voice.hip's pool, in the kernel's order: j ascending, every product, sum and the quotient rounded
to float32 on its own; clips of weight 0 are skipped; a speaker with one live clip is copied."""
import numpy as np

F32 = np.float32


def pool(v, w=None):
    """v [S, n, D] float32, w [S, n] float32 or None (all 1) -> [S, D] float32"""
    v = np.asarray(v, F32)
    S, n, D = v.shape
    w = np.ones((S, n), F32) if w is None else np.asarray(w, F32)
    out = np.empty((S, D), F32)
    for s in range(S):
        live = [j for j in range(n) if w[s, j] != 0]
        if len(live) == 1:
            out[s] = v[s, live[0]]
            continue
        acc = (w[s, live[0]] * v[s, live[0]]).astype(F32)
        wsum = F32(w[s, live[0]])
        for j in live[1:]:
            acc = (acc + (w[s, j] * v[s, j]).astype(F32)).astype(F32)
            wsum = F32(wsum + w[s, j])
        out[s] = (acc / wsum).astype(F32)
    return out
