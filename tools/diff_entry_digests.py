#!/usr/bin/env python3
"""SHA-256 of what every diffusion sampling entry returns, on shapes that reach every branch of the code-path table rule: one line per
case, to be compared line for line between two builds of the library (DTTS_LIB_PATH selects the other build).  Not a test: it gates
nothing and reads no fixture; the weights are the synthetic ones of the tests' `weights` fixture.

    python tools/diff_entry_digests.py > new.txt
    DTTS_LIB_PATH=/path/to/parent/libdetail_hip.so python tools/diff_entry_digests.py > parent.txt
    DTTS_INTEG_MAX_GB=0 python tools/diff_entry_digests.py ...        # no table: the in-step integrator, diff_invert's step-at-a-time route

DTTS_INTEG_MAX_GB is latched per process, so every setting is a process of its own.  Record: profiles/sampling_loop_refactor_digests.txt.
Needs an MI355X."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 10
# (name, T, lens): Bi = 6 -> table launches of 6 + 4 steps | Nu = 2 < B (umap shares a row), Bi = 5 -> 7 + 3 | one full row
SHAPES = [("ragged3", 48, [48, 20, 33]), ("shared_len", 40, [40, 23, 23]), ("single", 48, None)]


def digest(*tensors):
    return " ".join(hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for t in tensors)


def cases(rt, torch, name, T, lens, only=None):
    from detail_tts_amd.vqvae.utils.diffusion import space_timesteps
    B = len(lens) if lens else 1
    g = torch.Generator().manual_seed(1000 + T + 7 * B)
    rnd = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    ce = (rnd(B, 768, T) * 0.5).cuda()
    x0 = rnd(B, 128, T).cuda()
    known = (rnd(B, 128, T) * 0.5).clamp(-1, 1).cuda()
    noise = {n: rnd(n, B, 128, T).cuda() for n in (1, 6, 7, 10, 11)}
    keep = torch.zeros((B, T), dtype=torch.bool)
    keep[:, : T // 3] = True
    keep[:, 2 * T // 3:] = True
    sched, dpm = rt.diff_schedule(sorted(space_timesteps(4000, [N]))), rt.diff_schedule_dpm(N)
    seed, sids = 11, [5, 9, 2][:B]
    kw = dict(lens=lens)

    def emit(case, fn):
        if only is None or case in only:
            out = fn()
            print(f"{name}/{case}\t{digest(*(out if isinstance(out, tuple) else (out,)))}", flush=True)

    emit("sample_default_3steps", lambda: rt.diff_sample(ce, seed, sids, n_steps=3, **kw))
    for sname, sampler, eta, sc in (("p", 0, 0.0, sched), ("ddim05", 1, 0.5, sched), ("dpm", 2, 0.0, dpm)):
        for n in (0, 7):
            a = dict(sched=sc, sampler=sampler, eta=eta, n_steps=n, **kw)
            emit(f"sample_ex_{sname}_n{n or N}_drawn", lambda: rt.diff_sample_ex(ce, seed, sids, **a))
            given = dict(x_init=x0, denorm=False) if sampler == 2 else dict(x_init=x0, step_noise=noise[n or N], denorm=False)
            emit(f"sample_ex_{sname}_n{n or N}_given", lambda: rt.diff_sample_ex(ce, seed, sids, **a, **given))
    for sname, sampler, eta in (("p", 0, 0.0), ("ddim05", 1, 0.5)):
        a = dict(sched=sched, sampler=sampler, eta=eta, **kw)
        for first in (5, 2):
            emit(f"sample_from_{sname}_first{first}", lambda: rt.diff_sample_from(x0, ce, first, seed, sids, **a))
        emit(f"sample_from_{sname}_first5_noise", lambda: rt.diff_sample_from(x0, ce, 5, seed, sids, step_noise=noise[6], denorm=False, **a))
        for U in (1, 2):
            emit(f"inpaint_{sname}_U{U}_top_drawn", lambda: rt.diff_inpaint(known, keep, ce, seed, sids, resample=U, **a))
            emit(f"inpaint_{sname}_U{U}_first5_traj",
                 lambda: rt.diff_inpaint(known, keep, ce, seed, sids, resample=U, first_step=5, x_init=x0, return_trajectory=True, **a))
        emit(f"inpaint_{sname}_U2_first5_noises",
             lambda: rt.diff_inpaint(known, keep, ce, seed, sids, resample=2, first_step=5, x_init=x0, step_noise=noise[11],
                                     known_noise=noise[11] * 0.5, renoise=noise[11] * 0.25, **a))
        emit(f"step_{sname}", lambda: rt.diff_step(x0, ce, 4, seed, sids, sched=sched, sampler=sampler, eta=eta, return_x0=True, **kw))
    emit("invert_depth4_traj", lambda: rt.diff_invert(known, ce, 4, sched, return_trajectory=True, **kw))
    emit("p_sample", lambda: rt.diff_p_sample(x0, ce, 10, seed, sids, return_x0=True, **kw))
    emit("step_noise_given", lambda: rt.diff_step(x0, ce, 4, seed, sids, sched=sched, noise=noise[1][0], **kw))
    emit("step_dpm_second_order", lambda: rt.diff_step_dpm(x0, known, ce, 5, dpm, return_x0=True, **kw))
    emit("reverse_step", lambda: rt.diff_reverse_step(known, ce, 3, sched, return_x0=True, **kw))
    emit("mean_variance", lambda: rt.diff_mean_variance(x0, ce, 4, sched, **kw))


def main():
    import torch
    if not torch.cuda.is_available():
        sys.exit("diff_entry_digests needs an MI355X (no GPU visible): not run")
    from detail_tts_amd.runtime import Runtime
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    rt = Runtime(select_inference_params(synthetic_state_dict(0)), folded=True, parts=("diffusion",))
    print(f"# tools/diff_entry_digests.py: DTTS_INTEG_MAX_GB={os.environ.get('DTTS_INTEG_MAX_GB', '(unset)')}; {N}-step schedules; "
          "case, SHA-256 of every returned tensor", flush=True)
    for name, T, lens in SHAPES:
        cases(rt, torch, name, T, lens)
    rt.set_option("conv_x3", 0)                  # the exact fp32 kernels: one loop of each kind
    name, T, lens = SHAPES[0]
    cases(rt, torch, name + "_conv_x3=0", T, lens,
          only={"sample_ex_ddim05_n7_drawn", "sample_from_p_first2", "inpaint_ddim05_U2_top_drawn", "invert_depth4_traj", "reverse_step"})


if __name__ == "__main__":
    main()
