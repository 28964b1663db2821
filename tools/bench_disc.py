#!/usr/bin/env python3
"""Times MultiPeriodDiscriminator.forward(y, y_hat) plus the three loss functions at B = 16, t = 10240 against the same discriminator
written with torch.nn.functional.conv1d / conv2d on the same GPU (the project's own restatement on the folded weights, fp32, no TF32),
and writes profiles/disc_ab.txt.

Method: both sides warmed up, then timed in interleaved pairs (A B A B ...) with HIP events around each call; medians and the
inter-quartile range are reported.  No ratio is a pass criterion.

    python tools/bench_disc.py [--pairs 30] [--batch 16]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_mpd(W, y, y_hat):
    """the reference's arithmetic on folded weights: real and generated as one batch of 2B"""
    from detail_tts_amd.weights import DISC_P_CONVS, DISC_PERIODS, DISC_S_CONVS
    x0 = torch.cat([y, y_hat], 0)
    B = y.shape[0]
    scores, fmaps = [], []
    x, fm = x0, []
    for i, (_co, _ci, _k, s, g, p) in enumerate(DISC_S_CONVS):
        x = F.leaky_relu(F.conv1d(x, W[f"discriminators.0.convs.{i}.weight"], W[f"discriminators.0.convs.{i}.bias"], s, p, 1, g), 0.1)
        fm.append(x)
    x = F.conv1d(x, W["discriminators.0.conv_post.weight"], W["discriminators.0.conv_post.bias"], 1, 1)
    fm.append(x)
    scores.append(torch.flatten(x, 1, -1)); fmaps.append(fm)
    for d, per in enumerate(DISC_PERIODS, 1):
        x, fm = x0, []
        t = x.shape[-1]
        if t % per:
            x = F.pad(x, (0, per - t % per), "reflect")
        x = x.view(x.shape[0], 1, -1, per)
        for i, (_co, _ci, _k, s) in enumerate(DISC_P_CONVS):
            x = F.leaky_relu(F.conv2d(x, W[f"discriminators.{d}.convs.{i}.weight"], W[f"discriminators.{d}.convs.{i}.bias"], (s, 1), (2, 0)), 0.1)
            fm.append(x)
        x = F.conv2d(x, W[f"discriminators.{d}.conv_post.weight"], W[f"discriminators.{d}.conv_post.bias"], 1, (1, 0))
        fm.append(x)
        scores.append(torch.flatten(x, 1, -1)); fmaps.append(fm)
    return ([s[:B] for s in scores], [s[B:] for s in scores], [[m[:B] for m in f] for f in fmaps], [[m[B:] for m in f] for f in fmaps])


def torch_losses(dr, dg, fr, fg):
    fm = 2 * sum(torch.mean(torch.abs(r - g)) for a, b in zip(fr, fg) for r, g in zip(a, b))
    ld = sum(torch.mean((1 - r) ** 2) + torch.mean(g ** 2) for r, g in zip(dr, dg))
    lg = sum(torch.mean((1 - g) ** 2) for g in dg)
    return fm, ld, lg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=30)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disc_ab.txt"))
    a = ap.parse_args()
    import disc_inputs as DI
    from detail_tts_amd.vqvae.model_24k import MultiPeriodDiscriminator
    from detail_tts_amd.vqvae.modules import losses as L
    from detail_tts_amd.weights import select_discriminator_params, synthetic_state_dict
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    P = select_discriminator_params(synthetic_state_dict(0, only_prefixes=("discriminators.",), discriminator=True))
    disc = MultiPeriodDiscriminator(P, device="cuda:0", folded=True)
    W = {k: torch.from_numpy(v).cuda() for k, v in P.items()}
    rs = np.random.RandomState(7)
    y, y_hat = (torch.from_numpy(DI._signal(rs, a.batch, DI.A_T)).cuda() for _ in range(2))

    def ours():
        dr, dg, fr, fg = disc(y, y_hat)
        return L.feature_loss(fr, fg, rt=disc), L.discriminator_loss(dr, dg, rt=disc)[0], L.generator_loss(dg, rt=disc)[0]

    def base():
        with torch.no_grad():
            fm, ld, lg = torch_losses(*torch_mpd(W, y, y_hat))
            ld.item()                                    # the reference's discriminator_loss reads its lists back; ours does too
            return fm, ld, lg

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1), out

    for _ in range(5):
        ours(); base()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(a.pairs):
        t, oa = timed(ours); ta.append(t)
        t, ob = timed(base); tb.append(t)
    q = lambda v: (np.percentile(v, 25), np.median(v), np.percentile(v, 75))
    qa, qb = q(ta), q(tb)
    rel = [abs(float(x) - float(z)) / abs(float(z)) for x, z in zip(oa, ob)]
    lines = [f"MultiPeriodDiscriminator.forward + feature / discriminator / generator loss, B = {a.batch}, t = {DI.A_T}, fp32, {a.pairs} interleaved pairs after 5 warm-up calls each",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"libdetail_hip : median {qa[1]:.3f} ms (quartiles {qa[0]:.3f} .. {qa[2]:.3f})",
             f"torch F.conv* : median {qb[1]:.3f} ms (quartiles {qb[0]:.3f} .. {qb[2]:.3f})",
             f"ratio of medians (torch / libdetail_hip): {qb[1] / qa[1]:.3f}",
             f"losses agree to {max(rel):.2e} (relative; loss_fm, loss_disc, loss_gen)"]
    print("\n".join(lines))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
