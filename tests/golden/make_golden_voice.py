#!/usr/bin/env python3
"""Fixtures of the multi-clip / latents-in surface FROM THE REFERENCE ITSELF (build container only, CPU): UnifiedVoice.get_conditioning
(gpt/model.py:419-427), DiffusionTts.get_conditioning (vqvae/diff_model.py:221-229) and UnifiedVoice.compute_embeddings (:492-513) +
inference_model.generate.  Same shim, synthetic weights and Philox multinomial as make_golden.py / make_golden_valle.py.  Data only.

voice_latents.npz, per case (S speakers x n clips of T = 64 frames): the clips, their valid lengths, and the two get_conditioning
results in float32 and in float64.  Equal-length cases call the reference's get_conditioning on [S,n,128,T] as it stands.  Ragged cases
apply the same reference modules clip by clip to each clip CUT to its length and combine them as the reference combines them: the mean
of the n conditioning-encoder outputs; the mean over the n contextual-embedder outputs concatenated along time.  `*_dclip64` holds every
clip's own embedder mean in float64 - the plain mean of those is the WRONG pooling for clips of unequal length, and `*_plain_err`
records by how much it misses the right one.

voice_generate.npz: cond_latents = get_conditioning of n = 2 clips -> compute_embeddings(cond_latents, text) -> inference_model.generate
under the Philox multinomial; run in float32 and float64, which must return the same codes (else the next sample id).

    python tests/golden/make_golden_voice.py
"""
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import SEED_N, build_reference_model, install_shim, philox_rng, save   # noqa: E402

T = 64
G = 12
# name -> clip lengths [S][n]; None = every clip is T frames long (the reference's own 4-D call)
CASES = {
    "s2n3_eq": ((2, 3), None),
    "s2n3_rag": ((2, 3), [[37, 50, 64], [64, 37, 50]]),
    "s1n2_rag": ((1, 2), [[50, 37]]),
    "s1n1_rag": ((1, 1), [[37]]),
}


def conditioning(m, x, lens):
    """x [S,n,128,T] torch, lens [S][n] or None -> (gpt [S,768], diffusion [S,1536], per-clip embedder means [S,n,1536])"""
    import torch
    S, n = x.shape[:2]
    if lens is None:
        g = m.gpt.get_conditioning(x).squeeze(-1)
        d = m.diffusion.get_conditioning(x)
        dclip = torch.stack([m.diffusion.contextual_embedder(x[:, j]).mean(-1) for j in range(n)], 1)
        return g, d, dclip
    gs, ds, dcs = [], [], []
    for s in range(S):
        clips = [x[s:s + 1, j, :, : lens[s][j]] for j in range(n)]
        gs.append(torch.stack([m.gpt.conditioning_encoder(c) for c in clips], 1).mean(1).squeeze(-1))
        emb = [m.diffusion.contextual_embedder(c) for c in clips]
        ds.append(torch.cat(emb, -1).mean(-1))
        dcs.append(torch.stack([e.mean(-1) for e in emb], 1))
    return torch.cat(gs), torch.cat(ds), torch.cat(dcs)


@contextlib.contextmanager
def keep_float64():
    """the reference's GroupNorm32 and attention softmax cast to float32 with Tensor.float(); inside this block a float64 tensor stays
    what it is, so the double() model is float64 end to end"""
    import torch
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else orig(self, *a, **k)
    try:
        yield
    finally:
        torch.Tensor.float = orig


def generate(gpt, cond, text, sample_id, **kw):
    """compute_embeddings + inference_model.generate as inference_speech_tortoise calls it (gpt/model.py:539-545) -> generated codes"""
    import torch
    with philox_rng(sample_id=sample_id):
        inputs = gpt.compute_embeddings(cond, torch.from_numpy(text).long())
        trunc = inputs.shape[1]
        gen = gpt.inference_model.generate(inputs, bos_token_id=gpt.start_mel_token, pad_token_id=gpt.stop_mel_token,
                                           eos_token_id=gpt.stop_mel_token, max_length=trunc + G, num_return_sequences=1, **kw)
    return gen[:, trunc:].numpy()


def main():
    install_shim()
    import torch
    torch.set_grad_enabled(False)
    m32 = build_reference_model()
    m64 = build_reference_model().double()
    rs = np.random.RandomState(11)
    out = dict(T=np.array(T), cases=np.array(list(CASES)))
    for name, ((S, n), lens) in CASES.items():
        x = (rs.randn(S, n, 128, T) * 2 - 5).astype(np.float32)
        g32, d32, _ = conditioning(m32, torch.from_numpy(x), lens)
        with keep_float64():
            g64, d64, dc64 = conditioning(m64, torch.from_numpy(x).double(), lens)
        assert g64.dtype == d64.dtype == torch.float64
        plain = dc64.mean(1)
        out[f"{name}_refer"] = x
        out[f"{name}_lens"] = np.asarray(lens if lens is not None else [[T] * n] * S, np.int32)
        out[f"{name}_gpt"], out[f"{name}_diffusion"] = g32.numpy(), d32.numpy()
        out[f"f64_{name}_gpt"], out[f"f64_{name}_diffusion"], out[f"f64_{name}_dclip"] = g64.numpy(), d64.numpy(), dc64.numpy()
        out[f"f64_{name}_plain_err"] = np.array(float((plain - d64).abs().max()))
        print(name, "f32 vs f64: gpt %.3e diffusion %.3e; plain mean of the clip means misses by %.3e" % (
            float((g32.double() - g64).abs().max()), float((d32.double() - d64).abs().max()), float((plain - d64).abs().max())))
    save("voice_latents", **out)

    # ---- latents-in decode
    x = torch.from_numpy(out["s1n2_rag_refer"][:, :, :, :])            # the n = 2 speaker, both clips at full length: the reference's own mean
    text = np.concatenate([rs.randint(3, 255, (1, 5)), [[0]]], 1).astype(np.int32)
    kw = dict(do_sample=True, top_p=0.8, temperature=0.8, length_penalty=1.0, repetition_penalty=2.0)
    c32 = m32.gpt.get_conditioning(x).squeeze(-1)
    c64 = m64.gpt.get_conditioning(x.double()).squeeze(-1)
    sid = 7
    while True:
        a = generate(m32.gpt, c32, text, sid, **kw)
        b = generate(m64.gpt, c64, text, sid, **kw)
        agree = a.shape == b.shape and np.array_equal(a, b)
        print("generate sample_id", sid, "f64 agrees" if agree else "f64 DISAGREES -> next seed", a.tolist())
        if agree:
            break
        sid += 100
        assert sid < 1000
    save("voice_generate", refer=x.numpy(), text=text, cond=c32.numpy(), f64_cond=c64.numpy(), codes=a, sample_id=np.array(sid),
         seed=np.array(SEED_N), G=np.array(G), f64_agree=np.array(agree), **{k: np.array(v) for k, v in kw.items()})


if __name__ == "__main__":
    main()
