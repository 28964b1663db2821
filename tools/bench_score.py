"""dtts_gpt_score timing (reported, not gated): the fused kernel at 16 rows x 234 and 16 x 600 columns against the MATERIALISING route -
the existing mel_head conv launch (dtts_op_conv1d) into a [B, V, n] buffer + a log-softmax and gather over it (torch ops: the
comparison lives in this tool only, the product path has no such route) - with the peak extra device memory of both; and what
N = 4 candidates add to stage A at B = 2 against N = 1 (decode + scoring, 234 tokens, the same process).

    python tools/bench_score.py [out.txt]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from detail_tts_amd.gpt.candidates import expand_sample_ids
from detail_tts_amd.runtime import Runtime
from detail_tts_amd.weights import fold_weight_norm, synthetic_state_dict

V = 8194
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    rt = Runtime(fold_weight_norm(synthetic_state_dict(0, only_prefixes=["gpt."])), folded=True, parts=("gpt",))
    rs = np.random.RandomState(3)
    say("dtts_gpt_score vs the materialising route (mel_head conv into [B, V, n] + log_softmax + gather), fp32, one MI355X")
    for B, n in ((16, 234), (16, 600)):
        lat = torch.from_numpy(rs.randn(B, 768, n).astype(np.float32)).cuda()
        codes = [rs.randint(0, V, n).astype(np.int32) for _ in range(B)]
        idx = torch.from_numpy(np.stack(codes).astype(np.int64)).cuda()

        def fused():
            return rt.gpt_score(lat, codes)

        def materialised():
            logits = rt.op_conv1d("gpt.mel_head", lat, V, 1)
            return torch.log_softmax(logits, 1).gather(1, idx[:, None, :])[:, 0]

        err = float((fused() - materialised()).abs().max())
        t_f, t_m = timed(fused), timed(materialised)
        m_f, m_m = peak_extra(fused), peak_extra(materialised)
        gf = 2.0 * V * 768 * B * n / 1e9
        say(f"  {B} rows x {n} columns: fused {t_f:7.3f} ms ({gf / t_f:6.1f} TFLOP/s), peak extra memory {m_f:7.1f} MiB | "
            f"materialised {t_m:7.3f} ms, {m_m:7.1f} MiB | max |diff| {err:.2e}")
    say("  (fused: includes the host-side targets table; its partials live in a 4 MB workspace allocated at bind time, not counted)")
    # ---- what N = 4 adds to stage A at B = 2
    B, G = 2, 234
    refer = torch.from_numpy((rs.randn(B, 128, 936) * 2 - 5).astype(np.float32)).cuda()
    texts = [np.concatenate([rs.randint(3, 255, 60), [0]]) for _ in range(B)]

    def stage_a(N):
        ids = expand_sample_ids(list(range(B)), N)
        r = refer.repeat_interleave(N, 0).contiguous() if N > 1 else refer
        t = [x for x in texts for _ in range(N)]
        c, nc, lat = rt.gpt_generate(r, None, t, 1, ids, max_generate_length=G, suppress_eos=True)
        if N > 1:
            return rt.gpt_score(lat, [c[i, : nc[i]] for i in range(B * N)]).cpu()
        return lat

    t1, t4 = timed(lambda: stage_a(1), 3), timed(lambda: stage_a(4), 3)
    ids = expand_sample_ids(list(range(B)), 4)
    c, nc, lat = rt.gpt_generate(refer.repeat_interleave(4, 0).contiguous(), None, [x for x in texts for _ in range(4)], 1, ids,
                                 max_generate_length=G, suppress_eos=True)
    rows = [c[i, : nc[i]] for i in range(B * 4)]
    t_s = timed(lambda: rt.gpt_score(lat, rows).cpu())
    say(f"stage A at B = 2, {G} tokens: N = 1 {t1:.1f} ms; N = 4 (8 rows decoded + scored) {t4:.1f} ms = +{t4 - t1:.1f} ms, "
        f"of which the scoring call (8 x {G} columns, host copy included) {t_s:.3f} ms")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
