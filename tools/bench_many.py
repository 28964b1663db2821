#!/usr/bin/env python3
"""Time 32 single utterances through SynthesizerTrn.infer_many at 8 rows per call against the same 32 as serial batch-1 infer calls
(profiles/row_sampling_timing.txt).

    python tools/bench_many.py [N=32] [ROWS=8] [CODES=234] [STEPS=50]

Synthetic weights, suppress_eos (every utterance runs CODES codes), four voices, every fourth utterance with sampling settings of its
own.  Host clock around each form, ending in a device synchronise; one warm-up of each form first.  Prints one line per form and the
ratio.  The comparison is of time (a row is promised bit for bit only for the same grouping)."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
from detail_tts_amd.weights import select_inference_params, synthetic_state_dict

N, ROWS, CODES, STEPS = (int(v) for v in (sys.argv[1:5] + ["32", "8", "234", "50"][len(sys.argv) - 1:]))
m = SynthesizerTrn(select_inference_params(synthetic_state_dict(0)), folded=True)
rs = np.random.RandomState(0)
voices = [m.get_conditioning_latents(torch.from_numpy((rs.randn(1, 128, 200) * 2 - 5).astype(np.float32))) for _ in range(4)]
texts = [np.concatenate([rs.randint(3, 255, 40), [0]]) for _ in range(N)]
us = [dict(text=texts[i], speaker=voices[i % 4], **({"sampling": dict(temperature=0.6, top_p=0.9)} if i % 4 == 3 else {})) for i in range(N)]
kw = dict(max_generate_length=CODES, suppress_eos=True, diffusion_steps=STEPS)


def many():
    return sum(n for _, n in m.infer_many(iter(us), rows_per_call=ROWS, seed=3, **kw))


def serial():
    total = 0
    for i, u in enumerate(us):
        t = torch.from_numpy(u["text"])[None]
        _, lens = m.infer(t, [t.shape[1]], None, None, batch=True, speaker=u["speaker"], sampling=u.get("sampling"), seed=3, sample_ids=[i],
                          return_lengths=True, **kw)
        total += lens[0]
    return total


out = {}
for name, fn in (("infer_many", many), ("serial batch-1 infer", serial)):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    samples = fn()
    torch.cuda.synchronize()
    out[name] = time.perf_counter() - t0
    print(f"{name:22s} {N} utterances x {CODES} codes, {STEPS} diffusion steps: {out[name] * 1e3:9.1f} ms  = {out[name] * 1e3 / N:7.1f} ms per utterance, "
          f"{samples / 24000 / out[name]:6.1f} s of audio per second", flush=True)
print(f"infer_many at {ROWS} rows per call is {out['serial batch-1 infer'] / out['infer_many']:.2f} x the serial calls' rate", flush=True)
