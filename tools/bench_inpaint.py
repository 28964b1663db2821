#!/usr/bin/env python3
"""What mel inpainting costs, and whether the DEFAULT path moved against the parent commit.  Two measurements, one file
(profiles/inpaint_timing.txt); reports, gates nothing, and no speed claim is attached to the feature.

1. The loop, in this process: at batch 8 x 10 s (T = 936) the 50-step DDIM loop (dtts_diff_sample_ex, eta = 0) against the inpainting
   loop (dtts_diff_inpaint) of the same steps with the middle third regenerated, at U = 1 and U = 2.  Expected: U = 1 costs one
   elementwise pass per step on top of the plain loop; U = 2 runs 2 x 49 + 1 = 99 trunk pairs against 50.
2. The default infer() against the parent commit, as tools/bench_align.py measures it: the headline request (batch 8, 234 codes) in
   fresh child processes, one per tree, interleaved round by round (parent first, then this commit).

    mkdir -p bench_out/parent && git archive HEAD~1 | tar -x -C bench_out/parent && (cd bench_out/parent && python -m detail_tts_amd.build)
    python tools/bench_inpaint.py --parent bench_out/parent [--rounds 3] [--trials 4] [--out profiles/inpaint_timing.txt]

Without --parent the parent-versus-commit line says "not measured".  Needs an MI355X."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loop_timing(B, T, N, trials):
    sys.path.insert(0, ROOT)
    import torch
    from detail_tts_amd.runtime import Runtime
    from detail_tts_amd.vqvae.utils.diffusion import space_timesteps
    from detail_tts_amd.weights import fold_weight_norm, synthetic_state_dict
    rt = Runtime(fold_weight_norm(synthetic_state_dict(0, only_prefixes=["diffusion."])), folded=True, parts=("diffusion",))
    sched = rt.diff_schedule(sorted(space_timesteps(4000, [N])))
    torch.manual_seed(0)
    known = torch.rand(B, 128, T, device="cuda") * 1.6 - 0.8
    ce = torch.randn(B, 768, T, device="cuda") * 0.5
    keep = torch.ones((B, T), dtype=torch.bool)
    keep[:, T // 3: 2 * T // 3] = False
    sids = list(range(B))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(trials):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    kinds = [("plain", lambda: rt.diff_sample_ex(ce, 1, sids, sched=sched, sampler=1, denorm=False)),
             ("inpaint_U1", lambda: rt.diff_inpaint(known, keep, ce, 1, sids, sched=sched, sampler=1)),
             ("inpaint_U2", lambda: rt.diff_inpaint(known, keep, ce, 1, sids, sched=sched, sampler=1, resample=2))]
    out = {k: timed(fn) for k, fn in kinds}
    none = rt.diff_inpaint(known, torch.zeros_like(keep), ce, 1, sids, sched=sched, sampler=1)
    out["same_bits_with_nothing_kept"] = bool(torch.equal(none, kinds[0][1]()))
    return out


def child(root, trials, batch, codes):
    """runs in a fresh process with `root` in front of sys.path: the code of that tree alone.  Prints one JSON line."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_inpaint needs an MI355X (no GPU visible): not run")
    import detail_tts_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(detail_tts_amd.__file__))) == os.path.abspath(root), detail_tts_amd.__file__
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    model = SynthesizerTrn(select_inference_params(synthetic_state_dict(0)), folded=True)
    rs = np.random.RandomState(0)
    B = batch
    refer = torch.from_numpy((rs.randn(B, 128, 200) * 2 - 5).astype(np.float32))
    text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, 40)), np.zeros((B, 1), np.int64)], 1))
    kw = dict(batch=True, seed=1, sample_ids=list(range(B)), max_generate_length=codes + 1, suppress_eos=True)

    def trial():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.infer(text, [41] * B, refer, [200] * B, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    trial()                          # warm-up: code objects, workspaces, captured graphs
    out = {"plain": [trial() for _ in range(trials)]}
    pr = torch.cuda.get_device_properties(0)          # the runtime may report a generic marketing name: the architecture says which part
    out["device"] = f"{pr.name} ({getattr(pr, 'gcnArchName', '?').split(':')[0]}, {pr.multi_processor_count} CUs)"
    print("BENCH_INPAINT " + json.dumps(out))


def run_child(root, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", os.path.abspath(root), "--trials", str(a.trials), "--batch", str(a.batch),
           "--codes", str(a.codes)]
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=root, env=env, timeout=400)
    if r.returncode != 0:
        sys.exit(f"the child of {root} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_INPAINT ")][-1]
    return json.loads(line[len("BENCH_INPAINT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trials", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--codes", type=int, default=234)
    ap.add_argument("--frames", type=int, default=936)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_timing.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root")
    a = ap.parse_args()
    if a.child:
        return child(a.root, a.trials, a.batch, a.codes)
    commit, parent, per_round, device = [], [], [], "?"
    for _ in range(a.rounds):            # parent, commit, parent, commit, ...: every process is fresh
        rp = run_child(a.parent, a) if a.parent else None
        rc = run_child(ROOT, a)
        device = rc["device"]
        commit += rc["plain"]
        if rp:
            parent += rp["plain"]
            per_round.append(statistics.median(rc["plain"]) - statistics.median(rp["plain"]))
    lt = loop_timing(a.batch, a.frames, a.steps, a.trials)       # after the children: this process opens the GPU only now
    med = {k: statistics.median(lt[k]) for k in ("plain", "inpaint_U1", "inpaint_U2")}
    fmt = lambda v: " ".join(f"{x:.1f}" for x in v)  # noqa: E731
    N = a.steps
    lines = [f"# tools/bench_inpaint.py on {device}, synthetic weights",
             f"# 1. the diffusion loop alone: batch {a.batch}, T = {a.frames}, ({N}-step ddim, eta = 0), the middle third regenerated; {a.trials} timed calls",
             "#    after one warm-up each, ms per call between device events",
             "plain_loop_ms\t" + fmt(lt["plain"]),
             "inpaint_U1_ms\t" + fmt(lt["inpaint_U1"]),
             "inpaint_U2_ms\t" + fmt(lt["inpaint_U2"]),
             f"U = 1 against the plain loop: median {med['inpaint_U1']:.1f} ms against {med['plain']:.1f} ms, {med['inpaint_U1'] - med['plain']:+.1f} ms "
             f"({100 * (med['inpaint_U1'] - med['plain']) / med['plain']:+.2f} %), {(med['inpaint_U1'] - med['plain']) / N * 1e3:+.0f} us per step; "
             f"spread of the plain loop's trials {max(lt['plain']) - min(lt['plain']):.1f} ms",
             f"U = 2 against the plain loop: median {med['inpaint_U2']:.1f} ms, x{med['inpaint_U2'] / med['plain']:.3f} ({2 * (N - 1) + 1} trunk pairs against "
             f"{N}: x{(2 * (N - 1) + 1) / N:.3f})",
             f"nothing kept, U = 1 gives the plain loop's bits: {lt['same_bits_with_nothing_kept']}",
             f"# 2. infer() at batch {a.batch}, {a.codes} codes per utterance: {a.rounds} rounds, each one fresh process per tree (parent first, then this",
             f"#    commit), {a.trials} timed calls per process after one warm-up call; ms per call, host clock between device synchronisations",
             "commit_plain_ms\t" + fmt(commit)]
    med_p = statistics.median(commit)
    if parent:
        med_q = statistics.median(parent)
        lines += ["parent_plain_ms\t" + fmt(parent),
                  f"default path, this commit against its parent: median {med_p:.1f} ms against {med_q:.1f} ms, {med_p - med_q:+.1f} ms "
                  f"({100 * (med_p - med_q) / med_q:+.2f} %); per round " + " ".join(f"{v:+.1f}" for v in per_round) +
                  f" ms; spread of the parent's trials {max(parent) - min(parent):.1f} ms"]
    else:
        lines += ["default path, this commit against its parent: not measured (no --parent checkout given)"]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
