#!/usr/bin/env python3
"""tests/golden/gpt_forward.npz FROM THE REFERENCE ITSELF: UnifiedVoice.forward in loss mode (gpt/model.py:429-491), on the CPU.

Runs only in the build container (needs the reference checkout and transformers), under the shim of make_golden.py with the seed-0
synthetic weights; gpt.text_head, which those leave at its torch init, is loaded from synthetic_state_dict(0, optional=True).  The
reference's forward has no attention mask and takes both cross-entropies as plain means over every position, so a batch is a rectangle.

Case A (keys a_*), B = 2, from gpt_forced.npz (prompt 64 frames, 13 text ids, 12 codes): row 0 as it is; row 1 with cond_length 40 (the
prompt zeroed beyond), the text cut to 7 ids and zero-padded, codes (7 c + 13) mod 8192 of row 0's and wav_length 5 * 1024, so that
set_mel_padding rewrites its codes from column 6 on with 8193.  Case B (keys b_*), B = 1: 127 text ids and 127 codes drawn from
RandomState(b_seed) (randint(1, 255) / randint(0, 8192)), the same prompt: 129 positions per span, one past gpt_score's 128-column tile.

Stored per case X (data only): X_text int32 [B, Lt], X_codes int32 [B, n] (as passed to forward, BEFORE set_mel_padding), X_refer_lens,
X_text_lens, X_wav_lens int32 [B]; X_loss fp32 [2] = the reference's own (loss_text, loss_mel); X_text_logprob fp32 [B, Lt + 2] and
X_mel_logprob fp32 [B, n + 2] = float64 log_softmax of the reference's text / mel logits gathered at the targets ([text, 0, 0] /
[padded codes, 8193, 8193]); X_logit_pos int32 [3] (first, one interior, last position) and X_logits fp32 [B, 3, len(logit_rows)] =
mel_logits[b, logit_rows, pos].  Shared: logit_rows int32 = 0, 37, 74, ... (stride 37, coprime with 32) + 8190 .. 8193; b_seed.
The prompt is gpt_forced.npz's `refer` and is not stored again.

The script asserts that the file stays within 64 KiB and that the fixture can see a wrong gather: both losses recomputed with the
targets shifted by one position (every position scored against the NEXT position's target) differ from the true ones by more than
20 x GATE, in both cases.  Random-init logits are nearly flat and a mean over 129 positions averages most of a shift away (typically
0.02 - 0.03 is left), so b_seed was picked for it: the first of 1 .. 400 whose two shifted losses are both more than 0.044 off
(`--search` repeats that search and prints the seed; it writes nothing).

    python tests/golden/make_golden_forward.py [--search]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/forward_targets.py

import make_golden as MG  # noqa: E402

GATE = 2e-3                 # the per-position gate of tests/test_gpu_forward_losses.py (make_golden_score.py's, the same kernel)
SEED_B = 206
ROW_STRIDE = 37


def case_a(g):
    refer, text, codes = g["refer"], g["text"], g["codes"]
    n = codes.shape[1]
    r = np.repeat(refer, 2, 0).copy()
    r[1, :, 40:] = 0.0
    t = np.zeros((2, text.shape[1]), np.int64)
    t[0] = text[0]
    t[1, :7] = text[0][:7]
    c = np.stack([codes[0].astype(np.int64), (codes[0].astype(np.int64) * 7 + 13) % 8192])
    return dict(refer=r, refer_lens=[refer.shape[2], 40], text=t, text_lens=[text.shape[1], 7], codes=c, wav_lens=[n * 1024, 5 * 1024])


def case_b(g):
    rs = np.random.RandomState(SEED_B)
    t = rs.randint(1, 255, (1, 127)).astype(np.int64)
    c = rs.randint(0, 8192, (1, 127)).astype(np.int64)
    return dict(refer=g["refer"].copy(), refer_lens=[g["refer"].shape[2]], text=t, text_lens=[127], codes=c, wav_lens=[127 * 1024])


def run(m, torch, case, rows):
    from detail_tts_amd.gpt.model import forward_inputs
    from forward_targets import aligned_inputs_and_targets
    grabbed = {}
    hook = m.gpt.text_head.register_forward_hook(lambda mod, inp, out: grabbed.__setitem__("text", out.detach()))
    try:
        loss_text, loss_mel, mel_logits = m.gpt(torch.from_numpy(case["refer"]), torch.tensor(case["refer_lens"]), torch.from_numpy(case["text"]),
                                                torch.tensor(case["text_lens"]), torch.from_numpy(case["codes"]).clone(),
                                                torch.tensor(case["wav_lens"]))
    finally:
        hook.remove()
    B, Lt, n = case["text"].shape[0], case["text"].shape[1], case["codes"].shape[1]
    text_logits = grabbed["text"].permute(0, 2, 1)                         # [B, 257, Lt + 2]
    assert mel_logits.shape == (B, 8194, n + 2) and text_logits.shape == (B, 257, Lt + 2), (mel_logits.shape, text_logits.shape)
    # the targets as this project's host preprocessing builds them must be the reference's: its own losses come out of them
    tx, cd = forward_inputs(case["text"], case["text_lens"], case["codes"], case["wav_lens"])
    _, tt, _, mt = aligned_inputs_and_targets(tx, cd)
    lst = torch.log_softmax(text_logits.double(), 1).numpy()
    lsm = torch.log_softmax(mel_logits.double(), 1).numpy()

    def gather(ls, tg):
        return np.stack([ls[b, tg[b], np.arange(tg.shape[1])] for b in range(tg.shape[0])])

    tlp, mlp = gather(lst, tt), gather(lsm, mt)
    assert abs(-tlp.mean() - float(loss_text)) < 1e-5 and abs(-mlp.mean() - float(loss_mel)) < 1e-5, (tlp.mean(), loss_text, mlp.mean(), loss_mel)
    # a gather one position off must be visible in BOTH losses
    for name, ls, tg, true in (("text", lst, tt, -tlp.mean()), ("mel", lsm, mt, -mlp.mean())):
        off = -gather(ls, np.roll(tg, -1, axis=1)).mean()
        assert abs(off - true) > 20 * GATE, (name, off, true)
        print(f"  {name}: loss {true:.4f}, targets shifted by one {off:.4f}")
    pos = np.array([0, (n + 2) // 2, n + 1], np.int32)
    lg = mel_logits.numpy()[:, rows][:, :, pos].transpose(0, 2, 1)        # [B, 3, rows]
    return dict(text=case["text"].astype(np.int32), codes=case["codes"].astype(np.int32), refer_lens=np.array(case["refer_lens"], np.int32),
                text_lens=np.array(case["text_lens"], np.int32), wav_lens=np.array(case["wav_lens"], np.int32),
                loss=np.array([float(loss_text), float(loss_mel)], np.float32), text_logprob=tlp.astype(np.float32),
                mel_logprob=mlp.astype(np.float32), logit_pos=pos, logits=lg.astype(np.float32))


def shift_gaps(m, torch, case):
    """|loss with every target taken from the next position - loss| for (text, mel): what the assertion in run() bounds from below"""
    from detail_tts_amd.gpt.model import forward_inputs
    from forward_targets import aligned_inputs_and_targets
    grabbed = {}
    hook = m.gpt.text_head.register_forward_hook(lambda mod, inp, out: grabbed.__setitem__("text", out.detach()))
    try:
        _, _, mel_logits = m.gpt(torch.from_numpy(case["refer"]), torch.tensor(case["refer_lens"]), torch.from_numpy(case["text"]),
                                 torch.tensor(case["text_lens"]), torch.from_numpy(case["codes"]).clone(), torch.tensor(case["wav_lens"]))
    finally:
        hook.remove()
    tx, cd = forward_inputs(case["text"], case["text_lens"], case["codes"], case["wav_lens"])
    _, tt, _, mt = aligned_inputs_and_targets(tx, cd)
    out = []
    for logits, tg in ((grabbed["text"].permute(0, 2, 1), tt), (mel_logits, mt)):
        ls = torch.log_softmax(logits.double(), 1).numpy()
        mean = lambda t: -np.mean([ls[b, t[b], np.arange(t.shape[1])] for b in range(t.shape[0])])
        out.append(abs(mean(np.roll(tg, -1, axis=1)) - mean(tg)))
    return out


def search_seed(m, torch, g, margin=0.044, last=400):
    """how SEED_B was picked: the first seed in 1 .. last whose case B has both shift gaps above `margin`"""
    global SEED_B
    keep = SEED_B
    try:
        for seed in range(1, last + 1):
            SEED_B = seed
            gaps = shift_gaps(m, torch, case_b(g))
            if min(gaps) > margin:
                return seed, gaps
    finally:
        SEED_B = keep
    return None, None


def main():
    MG.install_shim()
    import torch
    torch.set_grad_enabled(False)
    from detail_tts_amd.weights import synthetic_state_dict
    m = MG.build_reference_model()
    head = synthetic_state_dict(MG.SEED_W, only_prefixes=["gpt.text_head."], optional=True)
    m.gpt.text_head.load_state_dict({k[len("gpt.text_head."):]: torch.from_numpy(v) for k, v in head.items()})
    g = dict(np.load(os.path.join(HERE, "gpt_forced.npz")))
    if "--search" in sys.argv[1:]:
        seed, gaps = search_seed(m, torch, g)
        print("first seed with both shift gaps above 0.044:", seed, gaps, "(SEED_B =", SEED_B, ")")
        return
    rows = np.concatenate([np.arange(0, 8190, ROW_STRIDE), np.arange(8190, 8194)]).astype(np.int32)
    out = dict(logit_rows=rows, b_seed=np.array(SEED_B, np.int64))
    for tag, case in (("a", case_a(g)), ("b", case_b(g))):
        print(f"case {tag.upper()}:")
        out.update({f"{tag}_{k}": v for k, v in run(m, torch, case, rows).items()})
    MG.save("gpt_forward", **out)
    size = os.path.getsize(os.path.join(HERE, "gpt_forward.npz"))
    assert size <= 64 * 1024, size
    print("losses A:", out["a_loss"], "B:", out["b_loss"])


if __name__ == "__main__":
    main()
