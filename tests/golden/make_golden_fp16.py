#!/usr/bin/env python3
"""Golden vectors of the diffusion trunk's half-precision mode FROM THE REFERENCE ITSELF (DiffusionTts.enable_fp16 = use_fp16).

Same recipe as make_golden_dpm.py (reference imported under its shim, seed-0 synthetic weights and the "signal" variant, Philox noise
at the reference's RNG sites).  With enable_fp16 the reference runs layers[1:] of the trunk under autocast (vqvae/diff_model.py:299-309;
everything outside self.layers stays fp32).  On the CPU autocast selects bfloat16, so the recorded difference to the reference's own
fp32 run, E_ref, is the error of an 8-bit-significand trunk: the device's fp16-operand mode has to stay below E_ref / 4 of the same
case (tests/test_gpu_fp16.py says where the 4 comes from).  Stored in trunk_fp16.npz (data only):

  fwd48_t{t}_{cond,uncond}_{y32,y16}     DiffusionTts.forward at the T = 48 shape of diff_cond.npz / diff_forward.npz (its x), at the
                                         fixture's timestep and at t = 1234: the fp32 and the enable_fp16 output
  fwd936_s{step}_{cond,uncond}_{y32,y16}_{s,t}   the same at T = 936 on fullsize_inputs.inputs(), sampling steps 47 and 0 of the 50-step
                                         schedule, subsampled as fullsize.npz ([::4, ::13] + the 8 tail columns)
  ..._emax, ..._erel                     E_ref of the case: max |y16 - y32| and rms(y16 - y32) / rms(y32), over the FULL outputs
  e2e_mel_s / e2e_mel_t / e2e_wav_s      one 50-step SynthesizerTrn.infer at the headline configuration (234 forced codes, "signal"
                                         weights, sample id 5) with enable_fp16: mel and waveform subsampled as dpm_e2e.npz
  e2e_mel_emax / e2e_mel_erel / e2e_wav_emax / e2e_wav_erel   its difference to the reference's fp32 infer of the same request (which
                                         is checked to reproduce e2e_fullsize_signal.npz bit for bit): over the subsampled mel blocks
                                         and the full waveform
The generator checks that autocast really engaged (the first conv of layers[1] returns bfloat16 with the switch on, float32 with it off), that
every E_ref is non-zero, and that its fp32 runs reproduce the existing fp32 fixtures.

    python tests/golden/make_golden_fp16.py [--no-e2e]      # ~10 min on 8 cores
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
from make_golden import build_reference_model, install_shim, save  # noqa: E402

CH_STRIDE, T_STRIDE, TAIL, WAV_STRIDE = 4, 13, 8, 8
T48_EXTRA_TIMESTEP = 1234
STEPS_936 = (47, 0)


def sub(a):
    a = np.asarray(a.detach().numpy() if hasattr(a, "detach") else a)[0]
    return a[::CH_STRIDE, ::T_STRIDE].copy(), a[:, -TAIL:].copy()


def err(y16, y32):
    a, b = np.asarray(y16, np.float64), np.asarray(y32, np.float64)
    return float(np.max(np.abs(a - b))), float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


class Fp16:
    """enable_fp16 on a reference DiffusionTts for the duration of a block, with the dtype the first conv of layers[1] hands on recorded"""

    def __init__(self, diffusion, on):
        self.d, self.on, self.seen = diffusion, on, []

    def __enter__(self):
        self.prev = self.d.enable_fp16
        self.d.enable_fp16 = self.on
        import torch
        # (a layer's own output is x + h = fp32 again; the autocast shows in what its convs hand on)
        conv = next(mod for mod in self.d.layers[1].modules() if isinstance(mod, torch.nn.Conv1d))
        self.hook = conv.register_forward_hook(lambda mod, inp, out: self.seen.append(out.dtype))
        return self

    def __exit__(self, *a):
        import torch
        self.d.enable_fp16 = self.prev
        self.hook.remove()
        want = torch.bfloat16 if self.on else torch.float32
        assert self.seen and all(t == want for t in self.seen), (self.on, self.seen[:3])


def forwards(m):
    import torch
    from fullsize_inputs import inputs
    d = m.diffusion
    out = {"ch_stride": np.array(CH_STRIDE), "t_stride": np.array(T_STRIDE), "tail": np.array(TAIL)}
    F = dict(np.load(os.path.join(HERE, "diff_forward.npz")))
    G = dict(np.load(os.path.join(HERE, "fullsize.npz")))

    def pair(x, ts, ce):
        r = {}
        for on in (False, True):
            with Fp16(d, on):
                r[on] = (d(x, ts, precomputed_aligned_embeddings=ce).float().numpy(),
                         d(x, ts, precomputed_aligned_embeddings=ce, conditioning_free=True).float().numpy())
        return r

    x, ce = torch.from_numpy(F["x"]), torch.from_numpy(F["code_emb"])
    t48 = (int(F["ts"][0]), T48_EXTRA_TIMESTEP)
    out["fwd48_timesteps"] = np.array(t48, np.int64)
    for t in t48:
        r = pair(x, torch.tensor([t]), ce)
        if t == int(F["ts"][0]):
            assert np.array_equal(r[False][0], F["out_cond"]) and np.array_equal(r[False][1], F["out_uncond"]), "fp32 run != diff_forward.npz"
        for h, nm in enumerate(("cond", "uncond")):
            k = f"fwd48_t{t}_{nm}"
            out[k + "_y32"], out[k + "_y16"] = r[False][h], r[True][h]
            out[k + "_emax"], out[k + "_erel"] = (np.array(v) for v in err(r[True][h], r[False][h]))
            print(k, "E_ref max %.3e rel rms %.3e" % err(r[True][h], r[False][h]), "|y| max %.3f" % np.abs(r[False][h]).max(), flush=True)
    I = inputs()
    x, ce = torch.from_numpy(I["x"]), torch.from_numpy(I["code_emb"])
    out["fwd936_steps"] = np.array(STEPS_936, np.int64)
    for step in STEPS_936:
        r = pair(x, torch.tensor([int(m.infer_diffuser.timestep_map[step])]), ce)
        for h, nm in enumerate(("cond", "uncond")):
            k = f"fwd936_s{step}_{nm}"
            s32, t32 = sub(r[False][h])
            assert np.array_equal(s32, G[f"fwd{step}_{nm}_s"]) and np.array_equal(t32, G[f"fwd{step}_{nm}_t"]), "fp32 run != fullsize.npz"
            out[k + "_y32_s"], out[k + "_y32_t"] = s32, t32
            out[k + "_y16_s"], out[k + "_y16_t"] = sub(r[True][h])
            out[k + "_emax"], out[k + "_erel"] = (np.array(v) for v in err(r[True][h], r[False][h]))
            print(k, "E_ref max %.3e rel rms %.3e" % err(r[True][h], r[False][h]), flush=True)
    return out


def e2e(m, fp16):
    """the reference's own SynthesizerTrn.infer (50 ancestral steps) at the headline configuration -> (mel blocks, full waveform)"""
    import torch
    from fullsize_inputs import N_CODES, T, e2e_inputs
    I = e2e_inputs()
    g = m.gpt
    got = {}
    o_fv = m.infer_flowvae

    def infer_flowvae(mel, yl, *a, **k):
        assert mel.shape == (1, 128, T), mel.shape
        got["mel_s"], got["mel_t"] = sub(mel)
        return o_fv(mel, yl, *a, **k)

    m.infer_flowvae = infer_flowvae
    codes_t = torch.from_numpy(I["codes"])
    orig = g.inference_speech_tortoise
    g.inference_speech_tortoise = lambda *a, **k: torch.cat([codes_t, torch.tensor([[g.stop_mel_token]])], 1)
    t0 = time.time()
    try:
        with Fp16(m.diffusion, fp16), MG.philox_rng(sample_id=5):
            wav = m.infer(torch.from_numpy(I["text"]), torch.tensor([I["text"].shape[1]]), torch.from_numpy(I["refer"]),
                          torch.tensor([I["refer"].shape[2]]))
    finally:
        g.inference_speech_tortoise = orig
        m.infer_flowvae = o_fv
    w = wav.float().numpy()[0, 0]
    assert w.shape == (1024 * N_CODES,)
    print(f"e2e enable_fp16={fp16}: {time.time() - t0:.0f} s", flush=True)
    return got["mel_s"], got["mel_t"], w.astype(np.float32)


def main():
    install_shim()
    import torch
    torch.set_grad_enabled(False)
    out = forwards(build_reference_model())
    if "--no-e2e" not in sys.argv:
        E = dict(np.load(os.path.join(HERE, "e2e_fullsize_signal.npz")))
        m = build_reference_model("signal")
        s32, t32, w32 = e2e(m, False)
        assert np.array_equal(s32, E["mel_s"]) and np.array_equal(t32, E["mel_t"]) and np.array_equal(w32, E["wav"]), "fp32 infer != e2e_fullsize_signal.npz"
        s16, t16, w16 = e2e(m, True)
        out["e2e_seed"], out["e2e_sample_id"], out["e2e_wav_stride"] = np.array(MG.SEED_N), np.array(5), np.array(WAV_STRIDE)
        out["e2e_mel_s"], out["e2e_mel_t"], out["e2e_wav_s"] = s16, t16, w16[::WAV_STRIDE].copy()
        m16, m32 = np.concatenate([s16.ravel(), t16.ravel()]), np.concatenate([s32.ravel(), t32.ravel()])
        out["e2e_mel_emax"], out["e2e_mel_erel"] = (np.array(v) for v in err(m16, m32))
        out["e2e_wav_emax"], out["e2e_wav_erel"] = (np.array(v) for v in err(w16, w32))
        print("e2e E_ref: mel max %.3e rel %.3e, wav max %.3e rel %.3e" % (*err(m16, m32), *err(w16, w32)), flush=True)
    for k, v in out.items():
        if k.endswith(("_emax", "_erel")):
            assert float(v) > 0, k
    save("trunk_fp16", **out)


if __name__ == "__main__":
    main()
