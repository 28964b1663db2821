#!/usr/bin/env python3
"""tests/golden/gpt_score.npz FROM THE REFERENCE ITSELF: the log-probabilities its own UnifiedVoice.forward assigns to given mel codes.

Runs only in the build container (needs the reference checkout and transformers, CPU only), under the shim of make_golden.py with the
seed-0 synthetic weights.  Inputs are gpt_forced.npz's (refer, text, codes) plus a second, shorter row cut from them (prompt 40 frames,
7 text ids, 5 codes).  The reference's forward has no attention mask, so a padded batch would let the pad positions of the shorter row
leak into its logits: each row goes through forward alone (what a ragged batch MEANS), and the rows are stored padded.

Stored (data only): logprob fp32 [2, n] = log_softmax(mel_logits[:, :, :n_b], dim 1) gathered at the row's codes (0 beyond n_b); of
row 0 at positions 0, 5 and n - 1 the float64 log-sum-exp over V (f64_lse [3]) and the last four logits, rows 8190 .. 8193 = the end
of the last full 32-row tile and the 2-row V tail (logits_tail [3, 4]); and the FULL logit vector at position 5 (logits_full [8194]).
Three full fp32 vectors (96 KiB of incompressible floats) do not fit the 64 KiB the file is held to; one does.

    python tests/golden/make_golden_score.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402

# the gate of tests/test_gpu_score.py (the 20 x rule; profiles/score_measured_errors.txt).  Random-init logits are nearly flat: the
# stored log-probabilities must spread over more than 100 gates, else a wrong gather could pass.
GATE = 2e-3


def main():
    MG.install_shim()
    import torch
    torch.set_grad_enabled(False)
    m = MG.build_reference_model()
    g = dict(np.load(os.path.join(HERE, "gpt_forced.npz")))
    refer, text, codes = g["refer"], g["text"], g["codes"]
    n = codes.shape[1]
    rows = [dict(refer=refer[0], text=text[0], codes=codes[0]),
            dict(refer=refer[0][:, :40], text=text[0][:7], codes=codes[0][:5])]
    logprob = np.zeros((2, n), np.float32)
    at = lse = None
    for b, r in enumerate(rows):
        nb = len(r["codes"])
        _, _, mel_logits = m.gpt(torch.from_numpy(r["refer"][None].copy()), torch.tensor([r["refer"].shape[1]]),
                                 torch.from_numpy(r["text"][None].astype(np.int64)), torch.tensor([len(r["text"])]),
                                 torch.from_numpy(r["codes"][None].astype(np.int64)).clone(), torch.tensor([nb * 1024]))
        assert mel_logits.shape == (1, 8194, nb + 2), mel_logits.shape
        ml = mel_logits[:, :, :nb]
        lp = torch.log_softmax(ml.double(), 1)[0].numpy()                  # [V, nb]
        logprob[b, :nb] = lp[r["codes"], np.arange(nb)].astype(np.float32)
        if b == 0:
            at = ml[0, :, [0, 5, nb - 1]].T.numpy().astype(np.float32)     # [3, V]
            lse = torch.logsumexp(ml[0, :, [0, 5, nb - 1]].double(), 0).numpy()
    vals = np.concatenate([logprob[0, :n], logprob[1, :5]])
    spread = float(vals.std())
    assert spread > 100 * GATE, (spread, GATE)
    MG.save("gpt_score", refer_lens=np.array([refer.shape[2], 40], np.int32), text_lens=np.array([text.shape[1], 7], np.int32),
            ncodes=np.array([n, 5], np.int32), logprob=logprob, logits_steps=np.array([0, 5, n - 1]), f64_lse=lse, logits_tail=at[:, -4:],
            logits_full=at[1],
            spread=np.array(spread, np.float32))
    path = os.path.join(HERE, "gpt_score.npz")
    assert os.path.getsize(path) < 64 * 1024, os.path.getsize(path)
    print("logprob spread (std):", spread, "values:", vals)


if __name__ == "__main__":
    main()
