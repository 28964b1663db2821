#!/usr/bin/env python3
"""What infer(return_alignment=True) costs, and whether the DEFAULT path moved against the parent commit: the headline request (batch 8,
234 codes per utterance, synthetic weights) timed in fresh child processes, one per tree, interleaved round by round (other work
shares the host: compare neighbours, not blocks).  A child builds the model of ITS tree, warms up, then times `--trials` infer() calls
of each kind between device synchronisations; this commit's child alternates plain and with-alignment calls, the parent's child runs
the plain call only.  Writes profiles/align_timing.txt.

    git worktree add --detach bench_out/parent HEAD~1 && (cd bench_out/parent && python -m detail_tts_amd.build)
    python tools/bench_align.py --parent bench_out/parent [--rounds 3] [--trials 4] [--out profiles/align_timing.txt]

Without --parent the parent-versus-commit line says "not measured".  No speed claim is attached to the feature.  Needs an MI355X."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(root, trials, batch, codes, align):
    """runs in a fresh process with `root` in front of sys.path: the code of that tree alone.  Prints one JSON line."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_align needs an MI355X (no GPU visible): not run")
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

    def trial(extra):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.infer(text, [41] * B, refer, [200] * B, **kw, **extra)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    kinds = [("plain", {})] + ([("aligned", dict(return_alignment=True))] if align else [])
    for _, extra in kinds:           # warm-up: code objects, workspaces, captured graphs
        trial(extra)
    out = {k: [] for k, _ in kinds}
    for _ in range(trials):
        for k, extra in kinds:
            out[k].append(trial(extra))
    pr = torch.cuda.get_device_properties(0)          # the runtime may report a generic marketing name: the architecture says which part
    out["device"] = f"{pr.name} ({getattr(pr, 'gcnArchName', '?').split(':')[0]}, {pr.multi_processor_count} CUs)"
    print("BENCH_ALIGN " + json.dumps(out))


def run_child(root, a, align):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", os.path.abspath(root), "--trials", str(a.trials), "--batch", str(a.batch),
           "--codes", str(a.codes)] + (["--align"] if align else [])
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=root, env=env, timeout=400)
    if r.returncode != 0:
        sys.exit(f"the child of {root} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_ALIGN ")][-1]
    return json.loads(line[len("BENCH_ALIGN "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trials", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--codes", type=int, default=234)
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_timing.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root")
    ap.add_argument("--align", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.root, a.trials, a.batch, a.codes, a.align)
    plain, aligned, parent, per_round, device = [], [], [], [], "?"
    for _ in range(a.rounds):            # parent, commit, parent, commit, ...: every process is fresh
        rp = run_child(a.parent, a, False) if a.parent else None
        rc = run_child(ROOT, a, True)
        device = rc["device"]
        plain += rc["plain"]
        aligned += rc["aligned"]
        if rp:
            parent += rp["plain"]
            per_round.append(statistics.median(rc["plain"]) - statistics.median(rp["plain"]))
    med_p, med_a = statistics.median(plain), statistics.median(aligned)
    lines = [f"# tools/bench_align.py on {device}: infer() at batch {a.batch}, {a.codes} codes per utterance, synthetic weights",
             f"# {a.rounds} rounds, each one fresh process per tree (parent first, then this commit), {a.trials} timed calls of each kind per process",
             "# after one warm-up call; ms per call, host clock between device synchronisations",
             "commit_plain_ms\t" + " ".join(f"{v:.1f}" for v in plain),
             "commit_with_alignment_ms\t" + " ".join(f"{v:.1f}" for v in aligned)]
    if parent:
        med_q = statistics.median(parent)
        lines += ["parent_plain_ms\t" + " ".join(f"{v:.1f}" for v in parent),
                  f"default path (return_alignment=False), this commit against its parent: median {med_p:.1f} ms against {med_q:.1f} ms, "
                  f"{med_p - med_q:+.1f} ms ({100 * (med_p - med_q) / med_q:+.2f} %); per round " + " ".join(f"{v:+.1f}" for v in per_round) +
                  f" ms; spread of the parent's trials {max(parent) - min(parent):.1f} ms"]
    else:
        lines += ["default path (return_alignment=False), this commit against its parent: not measured (no --parent checkout given)"]
    lines += [f"with alignment: median {med_a:.1f} ms against {med_p:.1f} ms plain, +{med_a - med_p:.1f} ms ({100 * (med_a - med_p) / med_p:+.2f} %)"]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
