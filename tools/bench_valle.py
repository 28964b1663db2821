"""Acoustic-prompt decode timing (reported, not gated): a session whose PREFILL covers an m = 235 code prompt (about 10 s of audio;
dtts_gpt_options.prompt_codes, UnifiedVoice.inference_speech_valle) against the same 235 tokens fed through the decode loop as forced
steps (forced_codes with the rest sampled: inference_speech_tortoise's input_tokens route, the only one there was before), both followed
by the same 64 sampled tokens, at B = 1 and B = 8.  The two routes differ in the reference's fill id at mel position 0, which costs one
more prefix column; they do the same amount of work otherwise.

Every batch size runs in a child process of its own under `timeout` (a hung child ends the tool, nothing is retried); inside a child
the two routes alternate, after a warm-up of each, and the median of the repetitions is reported with their spread.

    python tools/bench_valle.py [out.txt]
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M, G, REPS = 235, 64, 9


def child(B):
    import numpy as np
    import torch
    from detail_tts_amd.runtime import Runtime
    from detail_tts_amd.weights import fold_weight_norm, synthetic_state_dict
    rt = Runtime(fold_weight_norm(synthetic_state_dict(0, only_prefixes=["gpt."])), folded=True, parts=("gpt",))
    rs = np.random.RandomState(3)
    refer = torch.from_numpy((rs.randn(B, 128, 936) * 2 - 5).astype(np.float32)).cuda()
    texts = [np.concatenate([rs.randint(3, 255, 60), [0]]).astype(np.int32) for _ in range(B)]
    prompt = [rs.randint(0, 8192, M) for _ in range(B)]
    args = (refer, None, texts, 1, list(range(B)))

    def prefill_route():
        return rt.gpt_generate(*args, max_generate_length=G, suppress_eos=True, prompt_codes=prompt)

    def step_route():
        return rt.gpt_generate(*args, max_generate_length=M + G, suppress_eos=True, forced_codes=prompt, forced_fill=-1)

    def once(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()                                    # (gpt_generate ends in a device synchronise: the codes come back to the host)
        return (time.perf_counter() - t) * 1e3

    for fn in (prefill_route, step_route):
        once(fn), once(fn)
    tp, ts = [], []
    for _ in range(REPS):
        tp.append(once(prefill_route))
        ts.append(once(step_route))
    tp, ts = np.sort(tp), np.sort(ts)
    print(f"RESULT B = {B}: prompt of {M} codes + {G} sampled tokens | in the prefill {np.median(tp):8.2f} ms (min {tp[0]:.2f}, max {tp[-1]:.2f}) | "
          f"as forced decode steps {np.median(ts):8.2f} ms (min {ts[0]:.2f}, max {ts[-1]:.2f}) | difference {np.median(ts) - np.median(tp):8.2f} ms "
          f"({REPS} alternating repetitions)", flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]))
    lines = ["acoustic prompt in the prefill (prompt_codes) vs the same tokens as forced decode steps (forced_codes), fp32, one MI355X, "
             "synthetic weights, wall clock around calls that end in a device synchronise"]
    for B in (1, 8):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", str(B)],
                           capture_output=True, text=True, cwd=ROOT)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            lines.append(f"B = {B}: no measurement (child exit {r.returncode})")
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            print(lines[-1], flush=True)
            break                                # nothing more is started on the device after a failed child
        lines.append(got[0][len("RESULT "):])
        print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
