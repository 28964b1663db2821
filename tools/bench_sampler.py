#!/usr/bin/env python3
"""Step count / sampler options at the headline shape (batch 8, 10 s prompts, 234 codes, suppress_eos), all in ONE process and
interleaved round by round, so that the box's clock and power state is shared by every configuration:

    python tools/bench_sampler.py --rounds 3 --steps 3 --out profiles/sampler_options.json

Per configuration (sampler, diffusion steps): ms per batch and audio-s/s blocking (one infer() per batch) and pipelined
(infer_stream), and stage_ms of one un-pipelined pass with per-stage hipEvents.  Board power and shader clock over the timed
region as bench.py --full reports them (bench.PowerSampler)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import L_TEXT, N_CODES, T_REF, PowerSampler  # noqa: E402

CONFIGS = [("p", 50), ("ddim", 50), ("ddim", 25), ("ddim", 20), ("p", 25), ("dpmsolver++", 50), ("dpmsolver++", 20), ("dpmsolver++", 10)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3, help="batches per timed run")
    ap.add_argument("--warmup", type=int, default=1, help="batches per configuration before the first round")
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds over all configurations")
    ap.add_argument("--out", help="write the JSON record here")
    args = ap.parse_args()
    import torch
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    model = SynthesizerTrn(select_inference_params(synthetic_state_dict(0)), folded=True, device="cuda:0")
    model.rt.set_option("gpt_graph", 0)                          # as bench.py's default
    B = args.batch
    rs = np.random.RandomState(1)
    refer = torch.from_numpy((rs.randn(B, 128, T_REF) * 2 - 5).astype(np.float32)).cuda()
    text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, L_TEXT)), np.zeros((B, 1), np.int64)], 1).astype(np.int32))
    tl, rl = torch.full((B,), L_TEXT + 1), torch.full((B,), T_REF)
    sids = list(range(B))
    audio_s = B * N_CODES * 1024 / 24000.0

    def blocking(sampler, n, first, count):
        for i in range(count):
            model.infer(text, tl, refer, rl, batch=True, seed=1234 + first + i, sample_ids=sids, max_generate_length=N_CODES + 1,
                        suppress_eos=True, sampler=sampler, diffusion_steps=n)

    def pipelined(sampler, n, first, count):
        reqs = (dict(text=text, text_length=tl, refer=refer, refer_lengths=rl, seed=1234 + first + i, sample_ids=sids) for i in range(count))
        for _ in model.infer_stream(reqs, max_generate_length=N_CODES + 1, suppress_eos=True, sampler=sampler, diffusion_steps=n):
            pass

    for s, n in CONFIGS:                                         # warm-up: schedules built, workspaces grown, kernels loaded
        pipelined(s, n, 0, args.warmup)
    torch.cuda.synchronize()
    res = {f"{s}{n}": {"sampler": s, "diffusion_steps": n, "blocking_ms": [], "pipelined_ms": []} for s, n in CONFIGS}
    power = PowerSampler(0).start()
    for r in range(args.rounds):
        for s, n in CONFIGS:
            for mode, fn in (("blocking_ms", blocking), ("pipelined_ms", pipelined)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(s, n, 100 + r * args.steps, args.steps)
                torch.cuda.synchronize()
                res[f"{s}{n}"][mode].append(round((time.perf_counter() - t0) * 1e3 / args.steps, 1))
    power = power.stop()
    for s, n in CONFIGS:                                         # per-stage hipEvents (one un-pipelined pass; adds syncs, untimed)
        model.stage_ms = {}
        model.infer(text, tl, refer, rl, batch=True, seed=99, sample_ids=sids, max_generate_length=N_CODES + 1, suppress_eos=True,
                    sampler=s, diffusion_steps=n)
        torch.cuda.synchronize()
        res[f"{s}{n}"]["stage_ms"] = {k: round(v, 2) for k, v in model.stage_ms.items()}
        model.stage_ms = None
    for v in res.values():
        for mode in ("blocking", "pipelined"):
            ms = float(np.median(v[f"{mode}_ms"]))
            v[f"{mode}_median_ms"] = round(ms, 1)
            v[f"{mode}_audio_s_per_s"] = round(audio_s / (ms / 1e3), 1)
    base = res["p50"]["stage_ms"].get("diff_sample")
    for v in res.values():
        d = v["stage_ms"].get("diff_sample")
        v["diff_sample_vs_p50"] = round(d / base, 3) if d and base else None
    out = {"command": " ".join([os.path.relpath(sys.argv[0], ROOT)] + sys.argv[1:]), "batch": B, "codes": N_CODES, "prompt_frames": T_REF,
           "audio_s_per_batch": round(audio_s, 3), "rounds": args.rounds, "steps_per_run": args.steps,
           "device": torch.cuda.get_device_name(0), "power": power, "configs": res}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
