"""Timing of the bits-per-dim loop (dtts_diff_calc_bpd) on the 200-step schedule at T = 936 (TT overrides): rows_per_pass = B - one
timestep per trunk pass, the reference's loop shape - against the library's default grouping (about 32 (utterance, timestep) rows per
pass), at B = 1 and B = 8, in one process.  Also checks that both groupings give the same bits.  Seed-0 synthetic weights: the timing
does not depend on the values.  Recorded in profiles/bpd_timing.txt; no threshold."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from detail_tts_amd.runtime import Runtime
from detail_tts_amd.vqvae.utils.diffusion import space_timesteps
from detail_tts_amd.weights import synthetic_state_dict, fold_weight_norm

T = int(os.environ.get("TT", 936))
W = fold_weight_norm(synthetic_state_dict(0, only_prefixes=["diffusion."]))
rt = Runtime(W, folded=True, parts=("diffusion",))
sched = rt.diff_schedule(sorted(space_timesteps(4000, [200])))
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


print(f"dtts_diff_calc_bpd, 200 timesteps, T = {T}, Philox noise (seed 1), wall ms per call (1 warm-up + 2 timed)")
for B in (1, 8):
    x = torch.rand(B, 128, T, device="cuda") * 1.6 - 0.8
    ce = torch.randn(B, 768, T, device="cuda") * 0.5
    ms_b, out_b = timed(lambda: rt.diff_calc_bpd(sched, x, ce, seed=1, rows_per_pass=B), 2)
    ms_d, out_d = timed(lambda: rt.diff_calc_bpd(sched, x, ce, seed=1), 2)
    same = all(torch.equal(out_b[k], out_d[k]) for k in out_b)
    print(f"B = {B}: rows_per_pass = B ({200} passes of {B}) {ms_b:9.1f} ms | default ({-(-200 * B // 32)} passes of <= 32) {ms_d:9.1f} ms | "
          f"x{ms_b / ms_d:.2f} | same bits: {same} | total_bpd[0] {float(out_d['total_bpd'][0]):.4f}")
