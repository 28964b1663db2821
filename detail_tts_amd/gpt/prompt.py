"""Acoustic prompts of UnifiedVoice.inference_speech_valle (reference gpt/model.py:546-579): host-side id assembly and checks.  No
device work here; csrc/model_gpt.hip (prompt_prefix_ids) builds the same streams for the prefill, and these helpers are what the
Python layer refuses bad prompts with before any library call.

The reference keeps the FIRST value of build_aligned_inputs_and_targets(mel_codes, start, stop), [8192, c_1 .. c_m] (the stop token
belongs to the second, the unused targets), so its fake_inputs hold 1 + (Lt + 3) + (m + 1) ids while the cached embedding covers
Lt + 3 columns.  The mel stream its GPT2InferenceModel.forward embeds (input_ids[:, mel_len:], gpt/model.py:132-136) is, per row,

    position 0      id 1 (the fill id of the prefix columns, embedded with mel_embedding)
    position 1      8192 (start_mel_token)
    position k + 1  c_k, k = 1 .. m
    position m+2+j  the j-th generated token

and HF's repetition penalty sees all of input_ids: {1, 8192} and the prompt's codes are penalised from the first step.  No stop token
closes the prompt, so none is in the history and none could finish the row."""
from __future__ import annotations

import numpy as np

FILL_ID = 1
START_MEL, STOP_MEL = 8192, 8193
N_CODES = 8192                   # prompt codes live in [0, 8192)
MAX_MEL_POS = 1603               # rows of mel_pos_embedding (max_mel_tokens + 3)


def prompt_rows(prompt_codes, B):
    """prompt_codes ([B, m] array / tensor, or a list of B one-dimensional arrays of any lengths, 0 included) -> list of B int64 arrays.
    ValueError on a wrong row count or a code outside [0, 8192)."""
    if hasattr(prompt_codes, "detach"):
        prompt_codes = prompt_codes.detach().cpu().numpy()
    if isinstance(prompt_codes, np.ndarray):
        if prompt_codes.ndim != 2:
            raise ValueError(f"prompt_codes: a [B, m] array or a list of B one-dimensional arrays, not shape {prompt_codes.shape}")
        rows = [r for r in prompt_codes]
    else:
        rows = [np.asarray(r.detach().cpu().numpy() if hasattr(r, "detach") else r) for r in prompt_codes]
    rows = [np.asarray(r).reshape(-1).astype(np.int64) for r in rows]
    if len(rows) != B:
        raise ValueError(f"prompt_codes: {len(rows)} rows for a batch of {B}")
    for b, r in enumerate(rows):
        if r.size and (int(r.min()) < 0 or int(r.max()) >= N_CODES):
            raise ValueError(f"prompt_codes: row {b} holds a code outside [0, {N_CODES})")
    return rows


def prompt_layout(rows, text_lens, max_generate_length, max_mel_pos=MAX_MEL_POS):
    """rows: prompt_rows' output; text_lens: ids per row as api.py passes them (trailing 0 included: the session embeds Lt + 2 text
    positions, [255, text.., 0]).  -> dict(mel_ids, n_p, lp, seen, pos_off): per row the mel stream [1, 8192, codes..] of the
    prefill, its length n_p = m + 2, the prefix length lp = 1 + (Lt + 2) + n_p (= the KV columns filled before the first decode step),
    the sorted ids the repetition-penalty history starts with, and pos_off = n_p, the mel position of the first generated token's input
    embedding.  ValueError when m + 3 + max_generate_length exceeds the position table: the session touches m + 2 + G of its rows (the
    sampler prepares the input of a token that is never fed) and one more is kept spare; the reference itself dies with IndexError
    from m + G = 1603 on."""
    G = int(max_generate_length)
    out = dict(mel_ids=[], n_p=[], lp=[], seen=[], pos_off=[])
    for b, r in enumerate(rows):
        m = int(len(r))
        if m + 3 + G > max_mel_pos:
            raise ValueError(f"prompt_codes: row {b} has {m} codes; m + 3 + max_generate_length = {m + 3 + G} exceeds the "
                             f"{max_mel_pos} rows of mel_pos_embedding")
        ids = np.concatenate([[FILL_ID, START_MEL], r]).astype(np.int64)
        out["mel_ids"].append(ids)
        out["n_p"].append(m + 2)
        out["lp"].append(1 + int(text_lens[b]) + 2 + m + 2)
        out["seen"].append(sorted(set(int(v) for v in ids)))
        out["pos_off"].append(m + 2)
    return out


def pack_prompt(prompt_codes, B, text_lens, max_generate_length, max_mel_pos=MAX_MEL_POS):
    """what Runtime hands to dtts_gpt_options: (codes int32 [B, stride >= 1] zero-padded, lens int32 [B]) after every check above"""
    rows = prompt_rows(prompt_codes, B)
    prompt_layout(rows, text_lens, max_generate_length, max_mel_pos)
    lens = np.array([len(r) for r in rows], np.int32)
    codes = np.zeros((B, max(1, int(lens.max()) if B else 1)), np.int32)
    for b, r in enumerate(rows):
        codes[b, : len(r)] = r
    return codes, lens


def check_prompt_args(prompt_codes, forced_codes, num_candidates):
    """host-side check of infer() / infer_gpt()'s prompt_codes against the arguments it cannot be combined with, before any launch"""
    if prompt_codes is None:
        return
    if forced_codes is not None:
        raise ValueError("prompt_codes continues a SAMPLED code sequence: it cannot be combined with forced_codes")
    if int(num_candidates) > 1:
        raise ValueError("prompt_codes with num_candidates > 1 (best-of-N behind a prompt) is not implemented")
