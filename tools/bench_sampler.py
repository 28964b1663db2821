#!/usr/bin/env python3
"""Step count / sampler options at the headline shape (batch 8, 10 s prompts, 234 codes, suppress_eos), all in ONE process and
interleaved round by round, so that the box's clock and power state is shared by every configuration:

    python tools/bench_sampler.py --rounds 3 --steps 3 --out profiles/sampler_options.json

Per configuration (sampler, diffusion steps, trunk precision): ms per batch and audio-s/s blocking (one infer() per batch) and
pipelined (infer_stream), the diffusion time alone once per round (hipEvents around stage B of one blocking call, interleaved like
the rest), and stage_ms of one un-pipelined pass with per-stage hipEvents.  Precision "fp16" = infer(trunk_precision="fp16"), the
reference's use_fp16 mode (layers[1:] of the trunk as single fp16 products).  Board power and shader clock over the timed region as
bench.py --full reports them (bench.PowerSampler), and per configuration over its own blocking runs (mean_W, sclk,
energy_J_per_step = mean_W x seconds per batch)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import L_TEXT, N_CODES, T_REF, PowerSampler  # noqa: E402

CONFIGS = [("p", 50, "fp32"), ("p", 50, "fp16"), ("ddim", 50, "fp32"), ("ddim", 25, "fp32"), ("ddim", 20, "fp32"), ("p", 25, "fp32"),
           ("dpmsolver++", 50, "fp32"), ("dpmsolver++", 20, "fp32"), ("dpmsolver++", 20, "fp16"), ("dpmsolver++", 10, "fp32")]


def key(s, n, prec):
    return f"{s}{n}" + ("" if prec == "fp32" else "_" + prec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3, help="batches per timed run")
    ap.add_argument("--warmup", type=int, default=1, help="batches per configuration before the first round")
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds over all configurations")
    ap.add_argument("--only", help="comma-separated configuration keys (p50, p50_fp16, ...): run these alone")
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

    configs = [c for c in CONFIGS if not args.only or key(*c) in args.only.split(",")]

    def blocking(sampler, n, prec, first, count):
        for i in range(count):
            model.infer(text, tl, refer, rl, batch=True, seed=1234 + first + i, sample_ids=sids, max_generate_length=N_CODES + 1,
                        suppress_eos=True, sampler=sampler, diffusion_steps=n, trunk_precision=prec)

    def pipelined(sampler, n, prec, first, count):
        reqs = (dict(text=text, text_length=tl, refer=refer, refer_lengths=rl, seed=1234 + first + i, sample_ids=sids) for i in range(count))
        for _ in model.infer_stream(reqs, max_generate_length=N_CODES + 1, suppress_eos=True, sampler=sampler, diffusion_steps=n,
                                    trunk_precision=prec):
            pass

    def staged(s, n, prec, seed):                                # one un-pipelined pass with per-stage hipEvents (adds syncs)
        model.stage_ms = {}
        model.infer(text, tl, refer, rl, batch=True, seed=seed, sample_ids=sids, max_generate_length=N_CODES + 1, suppress_eos=True,
                    sampler=s, diffusion_steps=n, trunk_precision=prec)
        torch.cuda.synchronize()
        out, model.stage_ms = {k: round(v, 2) for k, v in model.stage_ms.items()}, None
        return out

    for c in configs:                                            # warm-up: schedules built, workspaces grown, kernels loaded
        pipelined(*c, 0, args.warmup)
    torch.cuda.synchronize()
    res = {key(s, n, prec): {"sampler": s, "diffusion_steps": n, "trunk_precision": prec, "blocking_ms": [], "pipelined_ms": [], "diff_sample_ms": []}
           for s, n, prec in configs}
    pw = {key(*c): [] for c in configs}
    power = PowerSampler(0).start()
    for r in range(args.rounds):
        for c in configs:
            for mode, fn in (("blocking_ms", blocking), ("pipelined_ms", pipelined)):
                torch.cuda.synchronize()
                own = PowerSampler(0).start() if mode == "blocking_ms" else None
                t0 = time.perf_counter()
                fn(*c, 100 + r * args.steps, args.steps)
                torch.cuda.synchronize()
                res[key(*c)][mode].append(round((time.perf_counter() - t0) * 1e3 / args.steps, 1))
                if own:
                    pw[key(*c)].append(own.stop())
            res[key(*c)]["diff_sample_ms"].append(staged(*c, 50 + r).get("diff_sample"))
    power = power.stop()
    for c in configs:
        res[key(*c)]["stage_ms"] = staged(*c, 99)
    for k, v in res.items():
        for mode in ("blocking", "pipelined"):
            ms = float(np.median(v[f"{mode}_ms"]))
            v[f"{mode}_median_ms"] = round(ms, 1)
            v[f"{mode}_audio_s_per_s"] = round(audio_s / (ms / 1e3), 1)
        v["diff_sample_median_ms"] = round(float(np.median(v["diff_sample_ms"])), 2)
        own = [q for q in pw[k] if q]
        if own:
            w = float(np.mean([q["mean_W"] for q in own]))
            v["power"] = {"mean_W": round(w, 1), "mean_sclk_MHz": round(float(np.mean([q["mean_sclk_MHz"] for q in own]))),
                          "energy_J_per_step": round(w * v["blocking_median_ms"] * 1e-3, 1), "over": "the blocking runs of this configuration"}
    base = res["p50"]["diff_sample_median_ms"] if "p50" in res else None
    for v in res.values():
        v["diff_sample_vs_p50"] = round(v["diff_sample_median_ms"] / base, 3) if base else None
    # (the record names its --out file by its place in the repository, or by its name alone when it lies elsewhere)
    argv = [os.path.relpath(a, ROOT) if a == args.out and os.path.abspath(a).startswith(ROOT + os.sep) else (os.path.basename(a) if a == args.out else a)
            for a in sys.argv[1:]]
    out = {"command": " ".join([os.path.relpath(sys.argv[0], ROOT)] + argv), "batch": B, "codes": N_CODES, "prompt_frames": T_REF,
           "audio_s_per_batch": round(audio_s, 3), "rounds": args.rounds, "steps_per_run": args.steps,
           "device": torch.cuda.get_device_name(0), "power": power, "configs": res}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
