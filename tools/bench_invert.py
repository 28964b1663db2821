"""Timing of DDIM inversion and of a sampling loop cut in two, at batch 8 x T = 936 and at batch 1 (TT overrides), N = 20 steps (NN
overrides), in one process:
  - an N-step inversion (dtts_diff_invert) against an N-step ddim_sample_loop (dtts_diff_sample_ex, eta = 0): the same 2N trunk forwards,
    expected equal within the run-to-run spread (the inversion's code-path table is built with the small-launch splits pinned off);
  - a loop cut in two (n_steps = N / 2, then dtts_diff_sample_from) against the whole loop, and whether both give the same bits.
Seed-0 synthetic weights: the timing does not depend on the values.  Recorded in profiles/invert_timing.txt; reports, gates nothing."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from detail_tts_amd.runtime import Runtime
from detail_tts_amd.vqvae.utils.diffusion import space_timesteps
from detail_tts_amd.weights import synthetic_state_dict, fold_weight_norm

T = int(os.environ.get("TT", 936))
N = int(os.environ.get("NN", 20))
W = fold_weight_norm(synthetic_state_dict(0, only_prefixes=["diffusion."]))
rt = Runtime(W, folded=True, parts=("diffusion",))
sched = rt.diff_schedule(sorted(space_timesteps(4000, [N])))
torch.manual_seed(0)


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, out


print(f"{N}-step schedule, T = {T}, wall ms per call (1 warm-up + 3 timed)")
for B in (8, 1):
    x = torch.rand(B, 128, T, device="cuda") * 1.6 - 0.8
    ce = torch.randn(B, 768, T, device="cuda") * 0.5
    sids = list(range(B))
    s = N // 2
    loop = lambda **k: rt.diff_sample_ex(ce, 1, sids, sched=sched, sampler=1, x_init=x, denorm=False, **k)  # noqa: E731
    ms_inv, _ = timed(lambda: rt.diff_invert(x, ce, N, sched), 3)
    ms_loop, whole = timed(loop, 3)

    def split():
        return rt.diff_sample_from(loop(n_steps=N - 1 - s), ce, s, 1, sids, sched=sched, sampler=1, denorm=False)

    ms_split, cut = timed(split, 3)
    print(f"B = {B}: inversion {ms_inv:8.1f} ms | ddim_sample_loop {ms_loop:8.1f} ms | x{ms_inv / ms_loop:.3f} || loop cut at step {s} "
          f"{ms_split:8.1f} ms | x{ms_split / ms_loop:.3f} of the whole | same bits: {torch.equal(cut, whole)} "
          f"(max-abs {float((cut - whole).abs().max()):.2e})")
