"""What the speaking-rate control costs (reported, not gated; no performance claim belongs to it).

  * the code embedding at B = 8, n = 234 codes through the x4 launch (dtts_diff_timestep_independent) and through a frame plan
    (dtts_diff_timestep_independent_ex: one map launch + the gather in the place of the x4 launch) - uniform at 4 n frames, uniform at
    speed 0.8, and by durations - and the two map kernels alone (dtts_op_frame_map); device events around 200 calls each;
  * the DEFAULT infer (no plan: B = 8, 234 tokens, 50 diffusion steps) of this tree against a checkout of the parent commit with its
    library built (--parent DIR): fresh child processes, alternating parent / this / parent / this ..., each a warm-up and REPS timed
    calls ending in a device synchronise.  The parent against itself (the spread of its children's medians) is the yardstick for the
    difference between the two trees.  Without --parent only this tree is timed.

Every child runs under `timeout` (a hung child ends the tool, nothing is retried).

    python tools/bench_duration.py [--parent DIR] [out.txt]
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("DTTS_BENCH_TREE", ROOT)             # the tree a child imports the package from
sys.path.insert(0, TREE)

B, N, G, STEPS, TR, REPS, ROUNDS, CALLS = 8, 234, 235, 50, 936, 5, 3, 200


def _model():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    return SynthesizerTrn(select_inference_params(synthetic_state_dict(0)), folded=True)


def child_kernels():
    import numpy as np
    import torch
    from detail_tts_amd.duration import speed_frames
    rt = _model().rt
    g = torch.Generator("cuda").manual_seed(1)
    lat = torch.randn(B, 768, N, device="cuda", generator=g)
    cond = torch.randn(B, 1536, device="cuda", generator=g) * 0.1
    ln = [N] * B
    rs = np.random.RandomState(0)
    durs = [rs.randint(2, 7, N) for _ in range(B)]
    for d in durs:
        d[-1] += (-int(d.sum())) % 4
    slow = [speed_frames(N, 0.8)] * B

    def timed(fn):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / CALLS * 1e3

    forms = (("x4 launch (no plan)", lambda: rt.diff_timestep_independent(lat, cond, ln)),
             ("plan, uniform, 4 n frames", lambda: rt.diff_timestep_independent(lat, cond, ln, frames=[4 * N] * B)),
             (f"plan, uniform, speed 0.8 ({slow[0]} frames)", lambda: rt.diff_timestep_independent(lat, cond, ln, frames=slow)),
             ("plan, durations", lambda: rt.diff_timestep_independent(lat, cond, ln, frames=[int(d.sum()) for d in durs], durations=durs)),
             ("map kernel alone, uniform", lambda: rt.op_frame_map(ln, [4 * N] * B)),
             ("map kernel alone, durations", lambda: rt.op_frame_map(ln, [int(d.sum()) for d in durs], durs)))
    rows = {name: [] for name, _ in forms}
    for _ in range(3):                                       # three alternating passes
        for name, fn in forms:
            rows[name].append(timed(fn))
    base = float(np.median(rows[forms[0][0]]))
    for name, _ in forms:
        r = rows[name]
        extra = "" if "alone" in name or name == forms[0][0] else f"; {np.median(r) - base:+7.1f} us against the x4 launch"
        print(f"RESULT code embedding B = {B}, n = {N}: {name:42s} {np.median(r):8.1f} us per call, allocation of the result included "
              f"(min {min(r):.1f}, max {max(r):.1f}){extra}", flush=True)


def child_infer():
    import numpy as np
    import torch
    model = _model()
    rs = np.random.RandomState(3)
    text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, 60)), np.zeros((B, 1), np.int64)], 1).astype(np.int32))
    refer = torch.from_numpy((rs.randn(B, 128, TR) * 2 - 5).astype(np.float32)).cuda()
    kw = dict(batch=True, seed=1, max_generate_length=G, suppress_eos=True, diffusion_steps=STEPS)
    ts = []
    for i in range(2 + REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        model.infer(text, [61] * B, refer, [TR] * B, **kw)
        torch.cuda.synchronize()
        if i >= 2:
            ts.append((time.perf_counter() - t) * 1e3)
    print("RESULT " + " ".join(f"{t:.2f}" for t in ts), flush=True)


def run_child(mode, tree=ROOT, limit=300):
    env = dict(os.environ, DTTS_BENCH_TREE=tree)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True,
                       env=env, cwd=tree)
    if r.returncode != 0:
        print(r.stdout + r.stderr)
        raise SystemExit(f"the child ({mode}, {tree}) ended with status {r.returncode}")
    return [l[len("RESULT "):] for l in r.stdout.splitlines() if l.startswith("RESULT ")]


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child-kernels":
        return child_kernels()
    if args and args[0] == "--child-infer":
        return child_infer()
    parent = None
    if args and args[0] == "--parent":
        parent, args = os.path.abspath(args[1]), args[2:]
    import numpy as np
    out = run_child("--child-kernels")
    meds = {"this": [], "parent": []}
    for _ in range(ROUNDS):
        for name, tree in (("parent", parent), ("this", ROOT)):
            if tree is not None:
                meds[name].append(float(np.median([float(v) for v in run_child("--child-infer", tree)[0].split()])))
    what = f"default infer (no plan), B = {B}, {G - 1} tokens, {STEPS} steps, median of {REPS} calls per process"
    for name in ("parent", "this"):
        if meds[name]:
            out.append(f"{what}, {name:6s} tree: " + " ".join(f"{m:.1f}" for m in meds[name]) +
                       f" ms in {ROUNDS} alternating processes; median {np.median(meds[name]):.1f}, spread (max - min) {max(meds[name]) - min(meds[name]):.1f} ms")
    if parent is not None:
        out.append(f"this tree against the parent: {np.median(meds['this']) - np.median(meds['parent']):+.1f} ms between the medians; "
                   f"the parent against itself spreads over {max(meds['parent']) - min(meds['parent']):.1f} ms")
    else:
        out.append("the parent tree was not given (--parent DIR): no comparison")
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args:
        with open(args[0], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
