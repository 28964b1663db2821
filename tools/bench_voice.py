"""What a reusable voice saves (reported, not gated): infer() with the prompt mel against infer() with speaker= (a Voice made once from
the same prompt; the same waveform bit for bit), alternating, at the headline batch (8 x 10 s prompts) and at batch 1, with stage_ms, so
that gpt_prefill (conditioning encoder + prefix + GPT-2 prefill + first token) and diff_cond (contextual embedder + timestep-independent
embedding) are seen separately; and get_conditioning_latents itself for n = 1, 4, 8 clips of 10 s per speaker.

Every batch size runs in a child process of its own under `timeout` (a hung child ends the tool, nothing is retried); inside a child the
two forms alternate, after a warm-up of each, and the median of the repetitions is reported with their spread.

    python tools/bench_voice.py [out.txt]
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TR, LT, G, STEPS, REPS = 936, 60, 233, 50, 7


def child(B):
    import numpy as np
    import torch
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    model = SynthesizerTrn(select_inference_params(synthetic_state_dict(0)), folded=True)
    rs = np.random.RandomState(3)
    refer = torch.from_numpy((rs.randn(B, 128, TR) * 2 - 5).astype(np.float32)).cuda()
    rl = torch.tensor([TR] * B)
    text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, LT)), np.zeros((B, 1), np.int64)], 1))
    tl = torch.tensor([LT + 1] * B)
    kw = dict(batch=True, seed=1, sample_ids=list(range(B)), max_generate_length=G, suppress_eos=True, diffusion_steps=STEPS)
    voice = model.get_conditioning_latents(refer, rl)

    def with_refer():
        return model.infer(text, tl, refer, rl, **kw)

    def with_speaker():
        return model.infer(text, tl, None, None, speaker=voice, **kw)

    def once(fn):
        model.stage_ms = {}
        torch.cuda.synchronize()
        t = time.perf_counter()
        wav = fn()
        torch.cuda.synchronize()
        ms, stages = (time.perf_counter() - t) * 1e3, dict(model.stage_ms)
        model.stage_ms = None
        return ms, stages, wav

    same = None
    for fn in (with_refer, with_speaker):
        once(fn)
        _, _, wav = once(fn)
        same = wav.clone() if same is None else bool(torch.equal(same, wav))
    rows = {"refer": [], "speaker": []}
    for _ in range(REPS):
        for name, fn in (("refer", with_refer), ("speaker", with_speaker)):
            ms, st, _ = once(fn)
            rows[name].append((ms, st.get("gpt_prefill", 0.0), st.get("diff_cond", 0.0)))
    med = {k: np.median(np.asarray(v), 0) for k, v in rows.items()}
    lo = {k: np.min(np.asarray(v), 0) for k, v in rows.items()}
    hi = {k: np.max(np.asarray(v), 0) for k, v in rows.items()}
    for k in ("refer", "speaker"):
        print(f"RESULT B = {B} infer({k:7s}): {med[k][0]:8.2f} ms per request (min {lo[k][0]:.2f}, max {hi[k][0]:.2f}) | gpt_prefill "
              f"{med[k][1]:6.2f} ms (min {lo[k][1]:.2f}, max {hi[k][1]:.2f}) | diff_cond {med[k][2]:6.2f} ms (min {lo[k][2]:.2f}, max {hi[k][2]:.2f})", flush=True)
    print(f"RESULT B = {B} saved by speaker=: {med['refer'][0] - med['speaker'][0]:6.2f} ms per request (gpt_prefill "
          f"{med['refer'][1] - med['speaker'][1]:.2f}, diff_cond {med['refer'][2] - med['speaker'][2]:.2f}); same waveform bits: {same}; "
          f"{REPS} alternating repetitions, {G} tokens, {STEPS} diffusion steps", flush=True)
    if B == 1:
        for n in (1, 4, 8):
            clips = torch.from_numpy((rs.randn(1, n, 128, TR) * 2 - 5).astype(np.float32)).cuda()
            ts = []
            for i in range(REPS + 2):
                torch.cuda.synchronize()
                t = time.perf_counter()
                model.get_conditioning_latents(clips)
                torch.cuda.synchronize()
                if i >= 2:
                    ts.append((time.perf_counter() - t) * 1e3)
            print(f"RESULT get_conditioning_latents, 1 speaker x {n} clips of {TR} frames: {np.median(ts):6.2f} ms (min {min(ts):.2f}, max {max(ts):.2f})",
                  flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
        return
    lines = []
    for B in (8, 1):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", str(B)], capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            raise SystemExit(f"child B = {B} ended with status {r.returncode}")
        lines += [l[len("RESULT "):] for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    out = "\n".join(lines) + "\n"
    print(out, end="")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
