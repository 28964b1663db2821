#!/usr/bin/env python3
"""Generate tests/golden/token_processor_edges.npz and tests/golden/gpt_generate_processors.npz (see make_golden.py for the setting).

(a) token_processor_edges: for every case of tests/processor_cases.py::CASES and every row, HF's OWN processor classes
(transformers generation/logits_process.py) run in the order GenerationMixin._get_logits_processor builds them - RepetitionPenalty,
NoRepeatNGram, MinLength, MinNewTokensLength, ExponentialDecayLengthPenalty, SuppressTokens, SuppressTokensAtBegin, Temperature, TopK,
TopP, MinP, Epsilon - on input_ids = [1] * fills + hist with input_ids_seq_length = the row's prompt_len and eos = V - 1.  Stored per
case: the parameters, the seed, V, the SHA-1 of the regenerated inputs, the kept mask (np.packbits per row) and HF's values at the kept
positions.  No logits rows.  No case puts a top-p cut inside a tie group (asserted).

(b) gpt_generate_processors: codes of the reference's UnifiedVoice.inference_speech_tortoise (one set: inference_speech_valle) under the
synthetic weights, B = 2, one option set per keyword and one with all of them, plus two sets for what HF counts as prompt: `input_tokens`
with min_new_tokens and begin_suppress_tokens (B = 1: the reference admits input_tokens for one prompt only) and an acoustic prompt with
min_length; HF's multinomial is replaced by the Philox inverse-CDF
draw exactly as in make_golden_r5.py.  Every keyword goes through the reference's generate(**hf_generate_kwargs) - none had to be
pinned at processor level only.  Beside each set's codes `<set>.codes` the fixture holds `<set>.base`, the same call without the
option.  Stores inputs and codes only.

    python tests/golden/make_golden_processors.py [a|b|ab]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)


def hf_filtered(x, row, params, opts, V):
    import torch
    from transformers.generation import logits_process as L
    ids = torch.tensor([[1] * row["fills"] + [int(i) for i in row["hist"]]], dtype=torch.long)
    eos = torch.tensor([V - 1])
    procs = []
    if params["rp"] != 1.0:
        procs.append(L.RepetitionPenaltyLogitsProcessor(penalty=float(params["rp"])))
    if opts.get("no_repeat_ngram_size"):
        procs.append(L.NoRepeatNGramLogitsProcessor(int(opts["no_repeat_ngram_size"])))
    if opts.get("min_length"):
        procs.append(L.MinLengthLogitsProcessor(int(opts["min_length"]), eos))
    if opts.get("min_new_tokens"):
        procs.append(L.MinNewTokensLengthLogitsProcessor(int(row["prompt_len"]), int(opts["min_new_tokens"]), eos))
    if opts.get("exponential_decay_length_penalty") is not None:
        procs.append(L.ExponentialDecayLengthPenalty(tuple(opts["exponential_decay_length_penalty"]), eos, int(row["prompt_len"])))
    if opts.get("suppress_tokens"):
        procs.append(L.SuppressTokensLogitsProcessor(list(opts["suppress_tokens"])))
    if opts.get("begin_suppress_tokens"):
        procs.append(L.SuppressTokensAtBeginLogitsProcessor(list(opts["begin_suppress_tokens"]), int(row["prompt_len"])))
    assert not params["mass"]
    if params["temp"] != 1.0:
        procs.append(L.TemperatureLogitsWarper(float(params["temp"])))
    if params["top_k"]:
        procs.append(L.TopKLogitsWarper(top_k=int(params["top_k"])))
    pre = L.LogitsProcessorList(procs)(ids, torch.from_numpy(x[None].copy())).numpy()[0]
    if params["top_p"] < 1.0:
        procs.append(L.TopPLogitsWarper(top_p=float(params["top_p"])))
    f = L.LogitsProcessorList(procs)(ids, torch.from_numpy(x[None].copy())).numpy()[0]
    for v in np.unique(pre[np.isfinite(pre)]):                 # the top-p cut never falls inside a tie group here
        g = pre == v
        assert np.isfinite(f[g]).sum() in (0, int(g.sum())), "top-p cut inside a tie group"
    if opts.get("min_p"):
        procs.append(L.MinPLogitsWarper(min_p=float(opts["min_p"])))
    if opts.get("epsilon_cutoff"):
        procs.append(L.EpsilonLogitsWarper(epsilon=float(opts["epsilon_cutoff"])))
    f = L.LogitsProcessorList(procs)(ids, torch.from_numpy(x[None].copy())).numpy()[0]
    assert f.dtype == np.float32 and not np.isnan(f).any()
    return f


def opts_vector(opts):
    ed = opts.get("exponential_decay_length_penalty") or (-1, 0.0)
    return np.array([opts.get("no_repeat_ngram_size", 0), opts.get("min_length", 0), opts.get("min_new_tokens", 0), ed[0], ed[1],
                     opts.get("min_p", 0.0), opts.get("epsilon_cutoff", 0.0)], np.float64)


def make_edges(out_dir):
    import torch
    import processor_cases as P
    torch.manual_seed(0)
    torch.set_num_threads(1)
    out = {"cases": np.array(sorted(P.CASES))}
    for name in sorted(P.CASES):
        c = P.CASES[name]
        p = c["params"]
        logits, rows = P.case_inputs(name)
        f = np.stack([hf_filtered(logits[r], rows[r], p, P.case_options(name, r, logits), c["V"]) for r in range(c["R"])])
        kept = np.isfinite(f)
        out[name + ".params"] = np.array([p["rp"], p["temp"], p["top_k"], p["top_p"], p["mass"]], np.float64)
        out[name + ".opts"] = opts_vector(c["opts"])
        out[name + ".seed"] = np.array(c["seed"])
        out[name + ".V"] = np.array(c["V"])
        out[name + ".sha1"] = np.array(P.input_hash(logits, rows))
        out[name + ".kept"] = np.packbits(kept, axis=1)
        out[name + ".nkept"] = kept.sum(1).astype(np.int64)
        out[name + ".values"] = np.concatenate([f[r][kept[r]] for r in range(c["R"])]).astype(np.float32)
        print(f"{name:32s} V {c['V']:5d} kept {kept.sum(1).tolist()}")
    path = os.path.join(out_dir, "token_processor_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


# (b) the option sets: name -> (common keywords of the call, the option).  The base run of a set is the call without the option.
SAMPLED = dict(do_sample=True, top_p=0.8, temperature=0.8, repetition_penalty=2.0)
GREEDY = dict(do_sample=False, repetition_penalty=1.0)
# A decode whose stop token is likely at every step, for the two length processors to bite: all ids but the stop token and six others
# are suppressed and the temperature is high.  (An early ExponentialDecayLengthPenalty would do it too, but HF adds |-inf| * m to the
# -inf the length processors wrote: NaN scores.  The device keeps -inf there; no fixture row enters that state.)
STOPPY = dict(do_sample=True, top_k=0, top_p=1.0, temperature=3.0, repetition_penalty=2.0,
              suppress_tokens=sorted(set(range(8193)) - {5229, 6940, 3850, 6200, 5562, 7829}))
G_SETS = {
    "no_repeat_ngram_size": (GREEDY, dict(no_repeat_ngram_size=2)),
    "min_length": (STOPPY, dict(min_length=None)),                    # filled in below: the prefix columns count
    "min_new_tokens": (STOPPY, dict(min_new_tokens=9)),
    "exponential_decay_length_penalty": (SAMPLED, dict(exponential_decay_length_penalty=(3, 2.0))),
    "suppress_tokens": (GREEDY, dict(suppress_tokens=None)),          # filled in below: ids the base run draws
    "begin_suppress_tokens": (GREEDY, dict(begin_suppress_tokens=None)),
    "min_p": (dict(SAMPLED, top_k=0, top_p=1.0, temperature=1.5), dict(min_p=0.3)),
    "epsilon_cutoff": (dict(SAMPLED, top_k=0, top_p=1.0, temperature=1.5), dict(epsilon_cutoff=2e-4)),
    "valle_no_repeat_ngram_size": (GREEDY, dict(no_repeat_ngram_size=2)),
}
G_LEN = 16


def make_generate():
    from make_golden import SEED_N, build_reference_model, install_shim, philox_rng, save
    install_shim()
    import torch
    torch.set_grad_enabled(False)
    g = build_reference_model().gpt
    rs = np.random.RandomState(5)
    B, T_ref, L0, sid = 2, 64, 10, 11
    refer = (rs.randn(B, 128, T_ref) * 2 - 5).astype(np.float32)
    text = np.concatenate([rs.randint(3, 255, (B, L0)), np.zeros((B, 1), np.int64)], 1).astype(np.int32)
    prompt = rs.randint(0, 8192, (B, 6)).astype(np.int64)
    refer_t, text_t, rl = torch.from_numpy(refer), torch.from_numpy(text), torch.tensor([T_ref] * B)
    input_len = 1 + (L0 + 1 + 2) + 1                                  # cond + text positions (start, ids + pad 0, stop) + 8192

    def run(name, input_tokens=None, **kw):
        n = B if input_tokens is None else 1          # (the reference's torch.cat admits input_tokens for ONE prompt only, gpt/model.py:533-537)
        with philox_rng(sample_id=sid) as st:
            if input_tokens is not None:
                st["gpt_step"] = input_tokens.shape[1]                # forced positions draw nothing (make_golden_r5.py)
                kw = dict(kw, input_tokens=torch.from_numpy(input_tokens))
            if name.startswith("valle"):
                c = g.inference_speech_valle(refer_t[:n], rl[:n], text_t[:n], torch.from_numpy(prompt[:n]), num_return_sequences=1,
                                             max_generate_length=G_LEN, **kw)
            else:
                c = g.inference_speech_tortoise(refer_t[:n], rl[:n], text_t[:n], num_return_sequences=1, max_generate_length=G_LEN, **kw)
        c = c.numpy()
        return np.concatenate([c, np.full((n, G_LEN - c.shape[1]), 8193, c.dtype)], 1)

    out = {"sets": np.array(sorted(G_SETS) + ["all"])}
    allopt = {}
    for name in sorted(G_SETS):
        common, opt = G_SETS[name]
        base = run(name, **common)
        opt = dict(opt)
        if name == "min_length":
            opt["min_length"] = input_len + 12
        if name == "suppress_tokens":
            opt["suppress_tokens"] = sorted({int(base[0, 2]), int(base[1, 3]), int(base[0, 7])})
        if name == "begin_suppress_tokens":
            opt["begin_suppress_tokens"] = sorted({int(base[0, 0]), int(base[1, 0])})
        codes = run(name, **common, **opt)
        assert not np.array_equal(codes, base), name
        out[name + ".codes"], out[name + ".base"] = codes, base
        print(name, common, opt, "\n  base ", base.tolist(), "\n  codes", codes.tolist())
        import json
        out[name + ".common"] = np.array(json.dumps(common))
        out[name + ".option"] = np.array(json.dumps(opt))
        if not name.startswith("valle"):
            allopt.update(opt)
    import json
    common = dict(SAMPLED, top_k=0, top_p=1.0, temperature=1.5)
    # (the decay starts behind the last step the length processors ban the stop token at: see STOPPY)
    allopt.update(no_repeat_ngram_size=3, min_length=input_len + 6, min_new_tokens=8, exponential_decay_length_penalty=(8, 3.0))
    base = run("all", **common)
    codes = run("all", **common, **allopt)
    assert not np.array_equal(codes, base)
    print("all", allopt, "\n  base ", base.tolist(), "\n  codes", codes.tolist())
    out["all.codes"], out["all.base"] = codes, base
    out["all.common"], out["all.option"] = np.array(json.dumps(common)), np.array(json.dumps(allopt))
    # What HF counts as prompt, through the reference: a forced prefix (input_tokens, one prompt: the first row) with min_new_tokens and
    # begin_suppress_tokens, which count from BEHIND it, and an acoustic prompt with min_length, which counts its codes.
    input_tokens = np.array([[5229, 6940, 3850]], np.int64)
    base = run("input_tokens", input_tokens=input_tokens, **STOPPY)
    k = input_tokens.shape[1]
    first = int(base[0, k]) if int(base[0, k]) != 8193 else 5229
    opt = dict(min_new_tokens=7, begin_suppress_tokens=[first])
    codes = run("input_tokens", input_tokens=input_tokens, **STOPPY, **opt)
    for name, common, opt, codes, base in (
            ("input_tokens_min_new_tokens", STOPPY, opt, codes, base),
            ("valle_min_length", STOPPY, dict(min_length=input_len + 1 + prompt.shape[1] + 9), None, None)):
        if codes is None:
            base, codes = run(name, **common), run(name, **common, **opt)
        assert not np.array_equal(codes, base), name
        print(name, opt, "\n  base ", base.tolist(), "\n  codes", codes.tolist())
        out[name + ".codes"], out[name + ".base"] = codes, base
        out[name + ".common"], out[name + ".option"] = np.array(json.dumps(common)), np.array(json.dumps(opt))
    out["sets"] = np.array(sorted(G_SETS) + ["all", "input_tokens_min_new_tokens", "valle_min_length"])
    save("gpt_generate_processors", refer=refer, text=text, prompt=prompt, sample_id=np.array(sid), seed=np.array(SEED_N),
         input_tokens=input_tokens, input_len=np.array(input_len), valle_input_len=np.array(input_len + 1 + prompt.shape[1]), max_generate_length=np.array(G_LEN), **out)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "ab"
    if "a" in what:
        make_edges(HERE)
    if "b" in what:
        make_generate()
