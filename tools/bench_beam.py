"""Beam-search decode timing (reported, not gated; no speed-up is claimed).

  a. ms per token of a beam session at (B, K) = (2, 4) and (1, 16) against a SAMPLED session of the same row count (8 / 16 rows): the
     difference of two runs of different lengths divided by the tokens between them, so the prefill drops out.
  b. the cache reorder's share of a beam token around steps 16, 234 and 600: the same difference with the handle option
     gpt_beam_skip_reorder on (the KV cache stays put; the results are then wrong, the other work is the same).
  c. the default decode, batch 8 x 234 codes, on this build (the figure the README quotes for the sampler's processors).
  d. (--ab PARENT_TREE) the same default decode on this tree and on a built checkout of the parent commit, INTERLEAVED: one fresh child
     process per run, parent / this / parent / this ..., four of each; a child reports the median of nine (234 - 1)-token differences.

Everything runs in ONE child process under `timeout` (a hung child ends the tool, nothing is retried); the variants of a comparison
alternate after a warm-up of each, medians of REPS repetitions with their spread.  Synthetic weights; suppress_eos keeps every session at
its full length.

    python tools/bench_beam.py [out.txt]
    python tools/bench_beam.py --ab PARENT_TREE [out.txt]        # d. alone; appended to out.txt
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5


def child():
    import numpy as np
    import torch
    from detail_tts_amd.runtime import Runtime
    from detail_tts_amd.weights import fold_weight_norm, synthetic_state_dict
    rt = Runtime(fold_weight_norm(synthetic_state_dict(0, only_prefixes=["gpt."])), folded=True, parts=("gpt",))
    rs = np.random.RandomState(3)

    def inputs(B):
        refer = torch.from_numpy((rs.randn(B, 128, 200) * 2 - 5).astype(np.float32)).cuda()
        return refer, [np.concatenate([rs.randint(3, 255, 30), [0]]).astype(np.int32) for _ in range(B)]

    def once(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()                                    # (both entries end in a device synchronise: the results come back to the host)
        return (time.perf_counter() - t) * 1e3

    def per_token(fns, g0, g1):
        """fns: name -> f(G).  -> name -> (median, min, max) ms per token between lengths g0 and g1, the variants alternating"""
        for f in fns.values():
            once(lambda: f(g0)), once(lambda: f(g1))
        acc = {k: [] for k in fns}
        for _ in range(REPS):
            for k, f in fns.items():
                acc[k].append((once(lambda: f(g1)) - once(lambda: f(g0))) / (g1 - g0))
        return {k: (float(np.median(v)), min(v), max(v)) for k, v in acc.items()}

    def beam(refer, texts, K, skip=False):
        def f(G):
            rt.set_option("gpt_beam_skip_reorder", 1 if skip else 0)
            try:
                return rt.gpt_generate_beams(refer, None, texts, K, max_generate_length=G, suppress_eos=True)
            finally:
                rt.set_option("gpt_beam_skip_reorder", 0)
        return f

    def sampled(refer, texts):
        return lambda G: rt.gpt_generate(refer, None, texts, 1, list(range(refer.shape[0])), max_generate_length=G, suppress_eos=True)

    for B, K in ((2, 4), (1, 16)):
        refer, texts = inputs(B)
        rrefer, rtexts = refer.repeat_interleave(K, 0).contiguous(), [t for t in texts for _ in range(K)]
        r = per_token({"beam": beam(refer, texts, K), "sampled": sampled(rrefer, rtexts)}, 32, 160)
        print(f"RESULT a. (B, K) = ({B}, {K}), {B * K} rows, tokens 32 .. 160: beam {r['beam'][0]:.4f} ms/token (min {r['beam'][1]:.4f}, max "
              f"{r['beam'][2]:.4f}) | sampled session of {B * K} rows {r['sampled'][0]:.4f} ms/token (min {r['sampled'][1]:.4f}, max "
              f"{r['sampled'][2]:.4f})", flush=True)
        for s0 in (16, 234, 600):
            r = per_token({"reorder": beam(refer, texts, K), "skipped": beam(refer, texts, K, skip=True)}, s0, s0 + 32)
            d = r["reorder"][0] - r["skipped"][0]
            print(f"RESULT b. (B, K) = ({B}, {K}) around step {s0}: {r['reorder'][0]:.4f} ms/token with the cache reorder, {r['skipped'][0]:.4f} "
                  f"without: {d:.4f} ms = {100 * d / r['reorder'][0]:.1f} % of the token (spread of either: {r['reorder'][2] - r['reorder'][1]:.4f} / "
                  f"{r['skipped'][2] - r['skipped'][1]:.4f})", flush=True)
    refer, texts = inputs(8)
    f = sampled(refer, texts)
    once(lambda: f(234)), once(lambda: f(234))
    t = sorted(once(lambda: f(234)) - once(lambda: f(1)) for _ in range(REPS))
    print(f"RESULT c. default decode, batch 8, 233 decode steps behind the prefill: {t[len(t) // 2]:.2f} ms (min {t[0]:.2f}, max {t[-1]:.2f}; "
          f"{REPS} repetitions, this build only)", flush=True)


def ab_child(root):
    """the default decode of the tree at `root` (its own package and library), batch 8, 233 decode steps behind the prefill"""
    sys.path.insert(0, root)
    os.chdir(root)
    import numpy as np
    import torch
    import detail_tts_amd
    from detail_tts_amd.runtime import Runtime
    from detail_tts_amd.weights import fold_weight_norm, synthetic_state_dict
    assert os.path.dirname(os.path.dirname(os.path.abspath(detail_tts_amd.__file__))) == root, detail_tts_amd.__file__
    rt = Runtime(fold_weight_norm(synthetic_state_dict(0, only_prefixes=["gpt."])), folded=True, parts=("gpt",))
    rs = np.random.RandomState(3)
    refer = torch.from_numpy((rs.randn(8, 128, 936) * 2 - 5).astype(np.float32)).cuda()
    texts = [np.concatenate([rs.randint(3, 255, 60), [0]]).astype(np.int32) for _ in range(8)]

    def once(G):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rt.gpt_generate(refer, None, texts, 1, list(range(8)), max_generate_length=G, suppress_eos=True)
        return (time.perf_counter() - t) * 1e3

    for _ in range(3):
        once(234), once(1)
    d = sorted(once(234) - once(1) for _ in range(9))
    print(f"RESULT {d[4]:.3f} {d[0]:.3f} {d[-1]:.3f}", flush=True)


def ab(parent, out_path):
    trees = {"parent": os.path.abspath(parent), "this": ROOT}
    meds = {k: [] for k in trees}
    for _ in range(4):
        for k, root in trees.items():
            r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--ab-child", root], capture_output=True, text=True)
            if r.returncode != 0:            # nothing is retried
                print(f"child ({k}) ended with status {r.returncode}\n{r.stderr[-2000:]}")
                sys.exit(1)
            meds[k].append(float([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][0].split()[1]))
    text = "RESULT d. default decode, batch 8, 233 decode steps, parent and this commit interleaved (one process per run, its median of 9):\n"
    for k, v in meds.items():
        text += f"   {k:6s} " + " ".join(f"{x:.2f}" for x in v) + f" ms   mean {sum(v) / len(v):.2f}, min {min(v):.2f}, max {max(v):.2f}\n"
    print(text)
    if out_path:
        open(out_path, "a").write(text)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--ab-child":
        ab_child(sys.argv[2])
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--ab":
        ab(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
        return
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
    head = ("tools/bench_beam.py: beam-search decode on one MI355X, synthetic weights, suppress_eos (full-length sessions).  Differences of "
            "two run lengths, variants alternating,\nmedians of %d repetitions.  Reported, not gated.\n" % REPS)
    text = head + "\n".join(lines) + ("\n" if lines else "") + ("" if r.returncode == 0 else f"child ended with status {r.returncode}\n{r.stderr[-2000:]}\n")
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
