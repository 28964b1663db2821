#!/usr/bin/env python3
"""Fixtures of UnifiedVoice.inference_speech_valle (gpt/model.py:546-579) FROM THE REFERENCE ITSELF (build container only, CPU): the
acoustic-prompt decode.  Same shim, synthetic weights and Philox multinomial as make_golden.py / make_golden_r5.py.  Stores data only:
inputs, seeds, the reference's returned codes and - through a forward hook on final_norm - the last-column hidden state of every step
(the value the next token is drawn from: what the device session writes as its decode-time latents).

Every case is run twice, in float32 and in float64, and must return the same codes: a case whose two runs disagree sits on a rounding
edge of the sampler and is replaced by the next seed (sample id), never compared more loosely.  `f64_agree` records the flag per case.

The two end-to-end cases are the reference's own SynthesizerTrn.infer / infer_gpt with line 782 / 819 calling inference_speech_valle
(inference_speech_tortoise monkeypatched, as make_golden.py does for forced codes), the prompt being encode()'s codes of a 40-frame mel.

    python tests/golden/make_golden_valle.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import SEED_N, build_reference_model, install_shim, philox_rng, save   # noqa: E402

G = 8               # max_generate_length of every case
KW = dict(top_p=0.8, temperature=0.8, length_penalty=1.0, repetition_penalty=2.0, max_generate_length=G)
# m = 130: with the 5-id text (Lt + 2 = 8 text positions) the prefix holds Lp = 1 + 8 + 132 = 141 columns, more than the 128 queries of
# one prefill attention block and more than two of its 64-key tiles (csrc/attention.hip: QPB = 128, KT = 64), and Lp + G = 149 takes the
# KV capacity from 128 to 256 columns
M_LONG = 130


def run_case(gpt, refer, rl, text, prompt, sample_id, dtype, **kw):
    """-> (codes [rows, <= G], hidden [steps, rows, C]) of one inference_speech_valle call"""
    import torch
    hid = []
    hook = gpt.final_norm.register_forward_hook(lambda mod, inp, out: hid.append(out[:, -1].detach().double().numpy().copy()))
    try:
        with philox_rng(sample_id=sample_id) as st:
            if kw.get("input_tokens") is not None:
                st["gpt_step"] = kw["input_tokens"].shape[1]       # forced positions draw nothing (oracle/philox.py keys a draw by its step)
            codes = gpt.inference_speech_valle(torch.from_numpy(refer).to(dtype), rl, torch.from_numpy(text), torch.from_numpy(prompt), **kw)
    finally:
        hook.remove()
    return codes.numpy(), np.stack(hid)


def main():
    install_shim()
    import torch
    torch.set_grad_enabled(False)
    m = build_reference_model()
    g32 = m.gpt
    g64 = build_reference_model().gpt.double()          # (a second instance: weight-norm hooks do not deep-copy)
    rs = np.random.RandomState(5)
    T_ref = 40
    refer2 = (rs.randn(2, 128, T_ref) * 2 - 5).astype(np.float32)
    text2 = np.concatenate([rs.randint(3, 255, (2, 5)), [[0], [0]]], 1).astype(np.int32)       # 5 ids + api.py's trailing 0
    text2[1, 3:] = 0          # row 1: a 3-id text.  The reference has no text mask: its batch is a rectangle and the shorter row's zeros are embedded as ids
    refer, text = refer2[:1], text2[:1]
    rl1, rl2 = torch.tensor([T_ref]), torch.tensor([T_ref, T_ref])
    prompts = {mm: rs.randint(0, 8192, (2, mm)).astype(np.int64) for mm in (0, 1, 5, 17, M_LONG)}
    input_tokens = np.array([[11, 12]], np.int64)

    # name -> (refer, rl, text, prompt, kwargs, sampled?)
    cases = {
        "m0": (refer, rl1, text, prompts[0][:1], dict(do_sample=True, num_return_sequences=1, **KW)),
        "m1": (refer, rl1, text, prompts[1][:1], dict(do_sample=True, num_return_sequences=1, **KW)),
        "typical": (refer, rl1, text, prompts[17][:1], dict(do_sample=True, num_return_sequences=1, typical_sampling=True, typical_mass=0.9, **KW)),
        "batch2": (refer2, rl2, text2, prompts[5], dict(do_sample=True, num_return_sequences=1, **KW)),
        "greedy": (refer, rl1, text, prompts[5][:1], dict(do_sample=False, num_return_sequences=1, length_penalty=1.0, repetition_penalty=2.0,
                                                           max_generate_length=G)),
        "nrs2": (refer, rl1, text, prompts[5][:1], dict(do_sample=True, num_return_sequences=2, **KW)),
        "input_tokens": (refer, rl1, text, prompts[5][:1], dict(do_sample=True, num_return_sequences=1, input_tokens=torch.from_numpy(input_tokens), **KW)),
        "long": (refer, rl1, text, prompts[M_LONG][:1], dict(do_sample=True, num_return_sequences=1, **KW)),
    }
    out = dict(refer2=refer2, text2=text2, seed=np.array(SEED_N), input_tokens=input_tokens, G=np.array(G), m_long=np.array(M_LONG))
    for mm, p in prompts.items():
        out[f"prompt_m{mm}"] = p
    names = []
    for name, (rf, rl, tx, pr, kw) in cases.items():
        sid = 7
        while True:
            c32, h32 = run_case(g32, rf, rl, tx, pr, sid, torch.float32, **kw)
            c64, _ = run_case(g64, rf, rl, tx, pr, sid, torch.float64, **kw)
            agree = c32.shape == c64.shape and np.array_equal(c32, c64)
            print(name, "sample_id", sid, "f64 agrees" if agree else "f64 DISAGREES -> next seed", c32.tolist())
            if agree:
                break
            sid += 100
            assert sid < 1000, name
        names.append(name)
        out[f"{name}_codes"], out[f"{name}_hidden"], out[f"{name}_sample_id"], out[f"{name}_f64_agree"] = c32, h32.astype(np.float32), np.array(sid), np.array(agree)
        out[f"{name}_prompt_m"] = np.array(pr.shape[1])
    out["cases"] = np.array(names)

    # ---- end to end: the reference's infer / infer_gpt with inference_speech_valle in the place of line 782 / 819
    rs = np.random.RandomState(6)
    T_e, L0 = 64, 12
    refer_e = (rs.randn(1, 128, T_e) * 2 - 5).astype(np.float32)
    text_e = np.concatenate([rs.randint(3, 255, (1, L0)), [[0]]], 1).astype(np.int32)
    prompt_mel = (rs.randn(1, 128, 40) * 2 - 5).astype(np.float32)
    prompt_e, _ = m.encode(torch.from_numpy(prompt_mel), torch.tensor([40]))                   # [1, 10] codes of the 40-frame prompt mel
    prompt_e = prompt_e.reshape(1, -1).long()
    refer_t, text_t, rl_e = torch.from_numpy(refer_e), torch.from_numpy(text_e), torch.tensor([T_e])
    orig = g32.inference_speech_tortoise
    got = {}

    def valle(*a, **k):
        k["max_generate_length"] = G
        got["codes"] = g32.inference_speech_valle(*a, prompt_e, **k)
        return got["codes"]

    g32.inference_speech_tortoise = valle
    try:
        with philox_rng(sample_id=5):
            wav_infer = m.infer(text_t, torch.tensor([text_e.shape[1]]), refer_t, rl_e)
        codes_infer = got["codes"].numpy()
        with philox_rng(sample_id=6):
            wav_gpt = m.infer_gpt(text_t, torch.tensor([text_e.shape[1]]), refer_t, rl_e)
        codes_gpt = got["codes"].numpy()
    finally:
        g32.inference_speech_tortoise = orig
    print("e2e codes", codes_infer.tolist(), codes_gpt.tolist())
    out.update(e2e_refer=refer_e, e2e_text=text_e, e2e_prompt_mel=prompt_mel, e2e_prompt=prompt_e.numpy(), e2e_infer_codes=codes_infer,
               e2e_infer_wav=wav_infer, e2e_infer_sample_id=np.array(5), e2e_gpt_codes=codes_gpt, e2e_gpt_wav=wav_gpt,
               e2e_gpt_sample_id=np.array(6))
    save("gpt_valle", **out)


if __name__ == "__main__":
    main()
