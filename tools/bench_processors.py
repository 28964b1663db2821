#!/usr/bin/env python3
"""Time the GPT decode at batch 8 with 234 codes under HF's remaining logits processors (profiles/processors_timing.txt).

    python tools/bench_processors.py CHECKOUT LABEL ['{"no_repeat_ngram_size": 3}'] [rows]

CHECKOUT is the root of a built checkout of this project whose `detail_tts_amd` package is imported - this one, or for an A/B the
parent commit's (which takes no processors).  One process prints one line: median / min / max over 10 timed repetitions (3 warm-ups)
of the 233 decode steps behind the prefill, host clock around the session's decode calls ending in a device synchronise, and the
SHA-1 of the codes.  suppress_eos keeps every row at the full length, so the timings compare the same work; the stop-token options
then change no code, and the others rarely do under the synthetic weights - identical hashes do not mean an option was not applied
(tests/test_gpu_processors.py shows that each one bites).  For an A/B alternate the two checkouts, process by process, in one shell
loop, and compare the difference of the means with the process-to-process spread of either side.
A fourth argument `rows` decodes the same session under per-row settings (Runtime rows=: the eight rows at eight temperatures, the
processors - pass null for none - on every row): the per-row path at the same size (profiles/row_sampling_timing.txt)."""
import json
import sys
import time

tree, label = sys.argv[1], sys.argv[2]
proc = json.loads(sys.argv[3]) if len(sys.argv) > 3 else None
sys.path.insert(0, tree)
import numpy as np
import torch
import detail_tts_amd
from detail_tts_amd.pipeline import drain_session
from detail_tts_amd.runtime import Runtime
from detail_tts_amd.weights import select_inference_params, synthetic_state_dict

assert detail_tts_amd.__file__.startswith(tree), (detail_tts_amd.__file__, tree)
W = select_inference_params(synthetic_state_dict(0))
rt = Runtime(W, folded=True, parts=("gpt",))
rs = np.random.RandomState(0)
B, G = 8, 234
refer = torch.from_numpy((rs.randn(B, 128, 200) * 2 - 5).astype(np.float32)).cuda()
texts = [np.concatenate([rs.randint(3, 255, 40), [0]]).astype(np.int32) for _ in range(B)]
kw = dict(max_generate_length=G, top_k=50, top_p=0.8, temperature=0.8, repetition_penalty=2.0, suppress_eos=True)
if proc:
    if "exponential_decay_length_penalty" in proc:
        proc["exponential_decay_length_penalty"] = tuple(proc["exponential_decay_length_penalty"])
    kw["processors"] = proc
if len(sys.argv) > 4 and sys.argv[4] == "rows":
    kw["rows"] = [dict(top_k=50, top_p=0.8, temperature=0.6 + 0.05 * b, repetition_penalty=2.0, max_generate_length=G, processors=proc)
                  for b in range(8)]
ts, codes0 = [], None
for rep in range(13):
    rt.gpt_prefill(refer, [200] * B, texts, 5, list(range(B)), **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    codes, ncodes, _ = drain_session(rt, G, True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if rep >= 3:
        ts.append((t1 - t0) * 1e3)
    codes0 = codes if codes0 is None else codes0
    assert np.array_equal(codes, codes0)
ts = np.array(ts)
import hashlib
print(f"{label:28s} decode of {G - 1} steps x {B} rows: median {np.median(ts):8.3f} ms  min {ts.min():8.3f}  max {ts.max():8.3f}  "
      f"per token {np.median(ts) / (G - 1) * 1e3:7.2f} us  codes sha1 {hashlib.sha1(np.ascontiguousarray(codes0).tobytes()).hexdigest()[:12]}", flush=True)
