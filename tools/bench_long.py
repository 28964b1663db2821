"""What infer_long costs and what its pipelining gains (reported, not gated): a text of 32 chunks in one voice under the synthetic
weights, every chunk decoded to a fixed length (suppress_eos), 8 chunks per group.

  * audio-seconds per second through infer_long(rows_per_call=8): the groups through infer_stream, joined on the device;
  * the same groups as a loop of blocking infer(batch=True) calls, joined by the same kernels (longform.run(pipelined=False));
  * the time to the first piece of infer_long(stream=True);
  * what the edges and the join cost per group (the call, then a wait for the join stream), beside that group's share of the total.

Audio seconds are the chunks' samples BEFORE trimming: under random weights the waveform is noise of one level and a trim level means
nothing (-60 dB here, so that the edges kernel and its read-back run).  The two forms alternate after a warm-up of each, in a child
process under `timeout` (a hung child ends the tool, nothing is retried); medians with their spread.

    python tools/bench_long.py [out.txt]
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNKS, ROWS, UNITS, G, STEPS, TR, REPS = 32, 8, 40, 234, 50, 936, 5
SENT, SPACE_ID = 250, 2


def child():
    import numpy as np
    import torch
    from detail_tts_amd import longform
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    model = SynthesizerTrn(select_inference_params(synthetic_state_dict(0)), folded=True)
    rs = np.random.RandomState(7)
    text = np.concatenate([np.concatenate([rs.randint(3, 200, UNITS), [SENT, SPACE_ID]]) for _ in range(CHUNKS)])
    refer = torch.from_numpy((rs.randn(1, 128, TR) * 2 - 5).astype(np.float32)).cuda()
    voice = model.get_conditioning_latents(refer, [TR])
    kw = dict(speaker=voice, sentence_ids=[SENT], space_id=SPACE_ID, rows_per_call=ROWS, seed=1, trim_db=-60.0, max_generate_length=G,
              suppress_eos=True, diffusion_steps=STEPS)
    skw = dict(noise_scale=0.667, max_generate_length=G, suppress_eos=True, diffusion_steps=STEPS)
    plan = longform.prepare(model, text, **{k: v for k, v in kw.items() if k not in ("max_generate_length", "suppress_eos", "diffusion_steps")})
    assert len(plan["chunks"]) == CHUNKS
    join_ms = []

    def timed_join(*a, **k):
        t = time.perf_counter()
        out = longform.join_group(model, *a, **k)
        model._join_stream.synchronize()
        join_ms.append((time.perf_counter() - t) * 1e3)
        return out

    def whole(pipelined):
        torch.cuda.synchronize()
        t = time.perf_counter()
        pieces = list(longform.run(model, plan, skw, pipelined=pipelined))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        audio = sum(c["samples"] for _, cs in pieces for c in cs) / 24000.0
        return dt, audio, torch.cat([p for p, _ in pieces], 2)

    def first_piece():
        torch.cuda.synchronize()
        t = time.perf_counter()
        gen = model.infer_long(text, stream=True, **kw)
        piece = next(gen)
        model._join_stream.synchronize()
        dt = time.perf_counter() - t
        for _ in gen:
            pass
        torch.cuda.synchronize()
        return dt, piece.shape[-1] / 24000.0

    same = None
    for p in (True, False):
        whole(p)
        same = whole(p)[2] if same is None else bool(torch.equal(same, whole(p)[2]))
    rows = {True: [], False: []}
    for _ in range(REPS):
        for p in (True, False):
            dt, audio, _ = whole(p)
            rows[p].append((dt, audio / dt))
    for p, name in ((True, "infer_long (groups through infer_stream)"), (False, "blocking infer(batch=True) loop + the same join")):
        r = np.asarray(rows[p])
        print(f"RESULT {name}: {np.median(r[:, 1]):7.2f} audio-s/s (min {r[:, 1].min():.2f}, max {r[:, 1].max():.2f}); "
              f"{np.median(r[:, 0]) * 1e3:8.1f} ms for {CHUNKS} chunks = {CHUNKS // ROWS} groups of {ROWS} x {(G - 1) * 1024 / 24000:.2f} s", flush=True)
    print(f"RESULT the two forms give the same bits: {same}; {REPS} alternating repetitions, {G} tokens, {STEPS} diffusion steps", flush=True)
    ts = [first_piece() for _ in range(REPS)]
    print(f"RESULT time to the first piece (stream=True): {np.median([t for t, _ in ts]) * 1e3:8.1f} ms (min {min(t for t, _ in ts) * 1e3:.1f}, "
          f"max {max(t for t, _ in ts) * 1e3:.1f}) for {ts[0][1]:.2f} s of joined audio", flush=True)
    model.join_group = timed_join
    try:
        totals = [whole(True)[0] for _ in range(REPS)]
    finally:
        del model.join_group
    print(f"RESULT edges + join per group (call + wait, {ROWS} rows of {(G - 1) * 1024} samples): {np.median(join_ms):6.3f} ms "
          f"(min {min(join_ms):.3f}, max {max(join_ms):.3f}) beside {np.median(totals) * 1e3 / (CHUNKS // ROWS):8.1f} ms per group in all", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
        return
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stdout + r.stderr)
        raise SystemExit(f"the child ended with status {r.returncode}")
    out = "\n".join(l[len("RESULT "):] for l in r.stdout.splitlines() if l.startswith("RESULT ")) + "\n"
    print(out, end="")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
