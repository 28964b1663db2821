#!/usr/bin/env python3
"""Generate tests/golden/beam_steps.npz and tests/golden/gpt_generate_beams.npz (see make_golden.py for the setting).

beam_steps: for every case of tests/beam_cases.py::CASES, HF's OWN _get_top_k_continuations, _get_running_beams_for_next_iteration,
_update_finished_beams, _check_early_stop_heuristic and _beam_search_has_unfinished_sequences (transformers generation/utils.py), chained
exactly as _beam_search chains them, on the planted logits of the case; log_softmax, RepetitionPenaltyLogitsProcessor,
NoRepeatNGramLogitsProcessor, MaxLengthCriteria and EosTokenCriteria are HF's / torch's too.  Stored per case and step: the 2K
candidates (score, beam, token, stop), the running beams, the finished set, the two flags - and per case the seed the search settled
on (the first whose candidate gaps are all >= beam_cases.MIN_GAP and whose finished-set and heuristic comparisons are all
>= beam_cases.MIN_REL_GAP apart, relative; asserted), the SHA-1 of the regenerated inputs and the smallest gap.
HF keeps stepping an utterance that is done while others of its batch run; `done[step, u]` (HF's loop-end test applied to utterance u
alone, latched) marks from where on its running beams are no longer anybody's business.  No logits are stored.

gpt_generate_beams: the reference's UnifiedVoice.inference_speech_tortoise / inference_speech_valle under the synthetic weights with
generate(num_beams=K, do_sample=False, ...), 16 generated steps, every utterance run alone (HF's results are per utterance; the device
groups them).  Under this transformers version the reference's beam search needs two attribute assignments, made HERE and nowhere in the
reference: `g.inference_model.config.vocab_size = 8194` (the config holds max_mel_tokens, and _beam_search reshapes by it) and a no-op
`_reorder_cache` (the reference decodes without a cache, kv_cache=False, so every step re-runs the whole prefix and a no-op reorder is
exact; its own _reorder_cache is handed None).  Stored per case: inputs, options, the returned sequences / lengths / sequences_scores,
the greedy `.base` of the same call (which the beams must differ from), per step the top 2K + 1 accumulated scores, the 2K candidates
and the running beams (sequences and running_beam_scores) and the finished-set scores - so every decision's margin is on record -
and `.min_gap`, the smallest of them (candidates: absolute; finished set and heuristic: relative to the score).  The generator
searches input seeds and keeps the first whose min_gap is >= beam_cases.E2E_MIN_GAP.

    python tests/golden/make_golden_beams.py [a|b|ab] [case,case: only these cases of b]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

REAL = -1.0e8          # scores below this carry a -1e9: not a decision anybody reads


def _gaps(v):
    v = np.sort(np.asarray(v, np.float64)[np.isfinite(v) & (np.asarray(v) > REAL)])
    return float(np.diff(v).min()) if v.size > 1 else np.inf


def _rel_gaps(v):
    """smallest gap between adjacent real scores relative to the larger magnitude: the finished set holds scores divided by
    length ** length_penalty, whose scale - and float32's resolution with it - moves with the penalty"""
    v = np.sort(np.asarray(v, np.float64)[np.isfinite(v) & (np.asarray(v) > REAL)])
    if v.size < 2:
        return np.inf
    return float((np.diff(v) / np.maximum(np.abs(v[1:]), np.abs(v[:-1]))).min())


def hf_chain(case, seed):
    import torch
    from transformers.generation import logits_process as L
    from transformers.generation import stopping_criteria as S
    from transformers.generation.utils import GenerationMixin
    import beam_cases as BC

    class M(GenerationMixin):
        pass
    m = M()
    V, K, U, G, P, steps = case["V"], case["K"], case["U"], case["G"], case["P"], case["steps"]
    eos, lp = V - 1, float(case["lp"])
    es = {0: False, 1: True, 2: "never"}[case["es"]]
    logits, prompt = BC.case_logits(case, seed), BC.prompts(case)
    max_length, keep = P + G, 2 * K
    input_ids = torch.from_numpy(prompt).repeat_interleave(K, dim=0)
    procs = L.LogitsProcessorList()
    if case["rp"] != 1.0:
        procs.append(L.RepetitionPenaltyLogitsProcessor(penalty=float(case["rp"])))
    if case["ngram"]:
        procs.append(L.NoRepeatNGramLogitsProcessor(int(case["ngram"])))
    crit = S.StoppingCriteriaList([S.MaxLengthCriteria(max_length=max_length), S.EosTokenCriteria(eos_token_id=eos)])
    mask = torch.cat((torch.ones(K, dtype=torch.bool), torch.zeros(keep - K, dtype=torch.bool)))
    running_sequences = torch.full((U, K, max_length), eos, dtype=torch.int64)
    running_sequences[:, :, :P] = input_ids.view(U, K, P)
    sequences = running_sequences.clone()
    running_beam_scores = torch.zeros((U, K), dtype=torch.float)
    running_beam_scores[:, 1:] = -1e9
    beam_scores = torch.full((U, K), -1e9, dtype=torch.float)
    is_sent_finished = torch.zeros((U, K), dtype=torch.bool)
    unsat = torch.ones((U, 1), dtype=torch.bool)
    running_beam_indices = torch.full((U, K, max_length - P), -1, dtype=torch.int32)
    beam_indices = running_beam_indices.clone()
    done = np.zeros(U, bool)
    rec = {k: [] for k in ("cand_score", "cand_beam", "cand_tok", "stop", "run_seq", "run_score", "parents", "fin_seq", "fin_score",
                           "fin_flag", "fin_len", "unsat", "done")}
    min_gap = min_rel = np.inf
    cur_len = P
    for step in range(steps):
        flat = running_sequences[:, :, :cur_len].flatten(0, 1)
        log_probs = torch.nn.functional.log_softmax(torch.from_numpy(logits[step].copy()), dim=-1)
        log_probs = procs(flat, log_probs)
        log_probs = log_probs.view(U, K, V) + running_beam_scores[:, :, None]
        log_probs = log_probs.reshape(U, K * V)
        live = ~done
        top1 = torch.topk(log_probs, min(keep + 1, K * V))[0].numpy()
        for u in range(U):
            if live[u]:
                min_gap = min(min_gap, _gaps(top1[u]))
        tk_lp, tk_seq, tk_bi = m._get_top_k_continuations(
            accumulated_log_probs=log_probs, running_sequences=running_sequences, running_beam_indices=running_beam_indices, cur_len=cur_len,
            decoder_prompt_len=P, do_sample=False, beams_to_keep=keep, num_beams=K, vocab_size=V, batch_size=U)
        hits = crit(tk_seq[:, :, :cur_len + 1].flatten(0, 1), None).view(U, keep)
        running_sequences, running_beam_scores, running_beam_indices = m._get_running_beams_for_next_iteration(
            topk_log_probs=tk_lp, topk_running_sequences=tk_seq, topk_running_beam_indices=tk_bi, next_token_hits_stopping_criteria=hits,
            num_beams=K)
        prev_fin = beam_scores.numpy().copy()
        sequences, beam_scores, beam_indices, is_sent_finished = m._update_finished_beams(
            sequences=sequences, topk_running_sequences=tk_seq, beam_scores=beam_scores, topk_log_probs=tk_lp, beam_indices=beam_indices,
            topk_running_beam_indices=tk_bi, is_early_stop_heuristic_unsatisfied=unsat, is_sent_finished=is_sent_finished,
            next_token_hits_stopping_criteria=hits, top_num_beam_mask=mask, num_beams=K, cur_len=cur_len, decoder_prompt_len=P,
            length_penalty=lp, early_stopping=es)
        cur_len += 1
        # the margins of the finished-set merge and of the heuristic's comparison, for the utterances still running
        hl = (max_length - P) if (es == "never" and lp > 0.0) else (cur_len - P)
        for u in range(U):
            if not live[u]:
                continue
            newly = (tk_lp[u, :K] / ((cur_len - P) ** lp)).numpy()[hits[u, :K].numpy()]
            min_rel = min(min_rel, _rel_gaps(np.concatenate([prev_fin[u], newly])))
            if bool(is_sent_finished[u].all()):
                best = float(running_beam_scores[u, 0]) / (hl ** lp)
                if best > REAL:
                    min_rel = min(min_rel, _rel_gaps([best, float(beam_scores[u].min())]))
        unsat = m._check_early_stop_heuristic(
            is_early_stop_heuristic_unsatisfied=unsat, running_beam_scores=running_beam_scores, beam_scores=beam_scores,
            is_sent_finished=is_sent_finished, cur_len=cur_len, max_length=max_length, decoder_prompt_len=P, early_stopping=es,
            length_penalty=lp)
        for u in range(U):
            go = m._beam_search_has_unfinished_sequences(unsat[u:u + 1], is_sent_finished[u:u + 1], hits[u:u + 1], es)
            done[u] = done[u] or not bool(go)
        off = (torch.arange(U) * K).view(-1, 1)
        rec["cand_score"].append(tk_lp.numpy().copy())
        rec["cand_beam"].append((tk_bi[:, :, step] - off).numpy().astype(np.int32))
        rec["cand_tok"].append(tk_seq[:, :, cur_len - 1].numpy().astype(np.int32))
        rec["stop"].append(hits.numpy().copy())
        rec["run_seq"].append(running_sequences[:, :, P:].numpy().astype(np.int32))
        rec["run_score"].append(running_beam_scores.numpy().copy())
        rec["parents"].append((running_beam_indices[:, :, step] - off).numpy().astype(np.int32))
        rec["fin_seq"].append(sequences[:, :, P:].numpy().astype(np.int32))
        rec["fin_score"].append(beam_scores.numpy().copy())
        rec["fin_flag"].append(is_sent_finished.numpy().copy())
        rec["fin_len"].append((beam_indices + 1).bool().sum(-1).numpy().astype(np.int32))
        rec["unsat"].append(unsat.numpy()[:, 0].copy())
        rec["done"].append(done.copy())
    out = {k: np.stack(v) for k, v in rec.items()}
    out["min_gap"] = np.array(min_gap)
    out["min_rel_gap"] = np.array(min_rel)
    out["sha1"] = np.array(BC.input_hash(logits, prompt))
    return out


def make_steps(out_dir):
    import torch
    import beam_cases as BC
    torch.set_num_threads(1)
    out = {"cases": np.array(sorted(BC.CASES))}
    for name in sorted(BC.CASES):
        case = BC.CASES[name]
        for seed in range(case["seed"], case["seed"] + 4000):
            r = hf_chain(case, seed)
            if r["min_gap"] >= BC.MIN_GAP and r["min_rel_gap"] >= BC.MIN_REL_GAP:
                break
        assert r["min_gap"] >= BC.MIN_GAP and r["min_rel_gap"] >= BC.MIN_REL_GAP, (name, float(r["min_gap"]), float(r["min_rel_gap"]))
        nfin = int((r["fin_score"][-1] > REAL).sum())
        stops = r["stop"].sum(-1).tolist()
        print(f"{name:24s} seed {seed:5d} min gap {float(r['min_gap']):.4f} rel {float(r['min_rel_gap']):.4f} finished {nfin} done {r['done'].astype(int).tolist()} "
              f"stops/step {stops}")
        out[name + ".seed"] = np.array(seed)
        for k, v in r.items():
            out[name + "." + k] = v
    path = os.path.join(out_dir, "beam_steps.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


G_LEN = 16


def make_generate(only=None):
    import json

    import torch
    from transformers.generation.utils import GenerationMixin
    import beam_cases as BC
    from make_golden import build_reference_model, install_shim, save
    install_shim()
    torch.set_grad_enabled(False)
    g = build_reference_model().gpt
    g.inference_model.config.vocab_size = 8194                      # the two assignments of the docstring
    g.inference_model._reorder_cache = lambda past, beam_idx: past
    rec = {}
    o_top, o_run, o_fin = (GenerationMixin._get_top_k_continuations, GenerationMixin._get_running_beams_for_next_iteration,
                           GenerationMixin._update_finished_beams)

    def top(self, accumulated_log_probs, **kw):
        rec["top"].append(torch.topk(accumulated_log_probs, kw["beams_to_keep"] + 1)[0].numpy().copy())
        out = o_top(self, accumulated_log_probs=accumulated_log_probs, **kw)
        rec["cand_score"].append(out[0].numpy().copy())
        rec["P"] = kw["decoder_prompt_len"]
        return out

    def run(self, **kw):
        out = o_run(self, **kw)
        rec["run_seq"].append(out[0][:, :, rec["P"]:].numpy().astype(np.int32))
        rec["run_score"].append(out[1].numpy().copy())
        return out

    def fin(self, **kw):
        prev = kw["beam_scores"].numpy().copy()
        out = o_fin(self, **kw)
        K = kw["num_beams"]
        n = kw["cur_len"] + 1 - kw["decoder_prompt_len"]
        hits = kw["next_token_hits_stopping_criteria"][0, :K].numpy()
        newly = (kw["topk_log_probs"][0, :K] / (n ** kw["length_penalty"])).numpy()[hits]
        rec["rel"] = min(rec["rel"], _rel_gaps(np.concatenate([prev[0], newly])))
        rec["fin_score"].append(out[1].numpy().copy())
        rec["fin_len"] = (out[2] + 1).bool().sum(-1).numpy().astype(np.int32)
        return out

    def call(case, u, seed, beams):
        rs = np.random.RandomState(seed)
        L0 = case["text_len"][u]
        refer = (rs.randn(1, 128, 64) * 2 - 5).astype(np.float32)
        text = np.concatenate([rs.randint(3, 255, (1, L0)), np.zeros((1, 1), np.int64)], 1).astype(np.int32)
        prompt = rs.randint(0, 8192, (1, case["prompt_m"])).astype(np.int64) if case["prompt_m"] else None
        kw = dict(do_sample=False, max_generate_length=G_LEN, **case["common"])
        if beams:
            kw.update(num_beams=case["K"], num_return_sequences=case["nrs"], **case["beam"])
        else:
            kw.update(num_return_sequences=1)
        rec.clear()
        rec.update(top=[], cand_score=[], run_seq=[], run_score=[], fin_score=[], rel=np.inf)
        a = (torch.from_numpy(refer), torch.tensor([64]), torch.from_numpy(text))
        c = (g.inference_speech_valle(*a, torch.from_numpy(prompt), **kw) if prompt is not None else g.inference_speech_tortoise(*a, **kw)).numpy()
        c = np.concatenate([c, np.full((c.shape[0], G_LEN - c.shape[1]), 8193, c.dtype)], 1).astype(np.int32)
        return dict(refer=refer[0], text=text[0], prompt=None if prompt is None else prompt[0], seqs=c)

    GenerationMixin._get_top_k_continuations, GenerationMixin._get_running_beams_for_next_iteration = top, run
    GenerationMixin._update_finished_beams = fin
    out = {"cases": np.array(sorted(BC.E2E_CASES)), "max_generate_length": np.array(G_LEN)}
    if only:          # regenerate the named cases, keep the others as the fixture has them
        old = np.load(os.path.join(HERE, "gpt_generate_beams.npz"))
        out.update({k: old[k] for k in old.files if k.split(".")[0] not in only and k not in out})
    try:
        for name in sorted(only or BC.E2E_CASES):
            case = BC.E2E_CASES[name]
            K, nrs = case["K"], case["nrs"]
            case_gap = np.inf
            for u in range(case["U"]):
                for seed in range(case["seed"] + 1000 * u, case["seed"] + 1000 * u + 300):
                    r = call(case, u, seed, True)
                    gaps = [_gaps(t[0]) for t in rec["top"]]
                    gap = min(min(gaps), rec["rel"])
                    if gap < BC.E2E_MIN_GAP:
                        continue
                    kept = {k: (list(v) if isinstance(v, list) else v) for k, v in rec.items()}
                    base = call(case, u, seed, False)["seqs"]
                    rec.clear()
                    rec.update(kept)
                    if not np.array_equal(base[0], r["seqs"][0]):          # (a case must differ from its greedy base)
                        break
                    gap = -1.0
                assert gap >= BC.E2E_MIN_GAP, (name, u, gap)
                steps = len(rec["top"])
                pad = lambda a, fill: np.concatenate([a, np.full((G_LEN - a.shape[0],) + a.shape[1:], fill, a.dtype)])      # noqa: E731
                k = f"{name}.u{u}."
                out[k + "refer"], out[k + "text"], out[k + "seed"] = r["refer"], r["text"], np.array(seed)
                if r["prompt"] is not None:
                    out[k + "prompt"] = r["prompt"]
                out[k + "seqs"], out[k + "lens"], out[k + "scores"] = r["seqs"], rec["fin_len"][0, :nrs], rec["fin_score"][-1][0, :nrs]
                out[k + "steps"] = np.array(steps)
                out[k + "top"] = pad(np.stack([t[0] for t in rec["top"]]), 0.0)
                out[k + "cand_score"] = pad(np.stack([t[0] for t in rec["cand_score"]]), 0.0)
                out[k + "run_seq"] = pad(np.stack([t[0] for t in rec["run_seq"]]), 8193)
                out[k + "run_score"] = pad(np.stack([t[0] for t in rec["run_score"]]), 0.0)
                out[k + "fin_score"] = pad(np.stack([t[0] for t in rec["fin_score"]]), 0.0)
                out[k + "min_gap"] = np.array(gap)
                early = int((rec["fin_len"][0, :nrs] < G_LEN).sum())
                out[k + "base"] = base
                case_gap = min(case_gap, gap)
                print(flush=True, end="")
                print(f"{name} u{u} seed {seed} steps {steps} gap {gap:.2e} lens {rec['fin_len'][0, :nrs].tolist()} early {early} "
                      f"scores {rec['fin_score'][-1][0, :nrs].tolist()}\n   best {r['seqs'][0].tolist()}\n   base {base[0].tolist()}")
            out[name + ".options"] = np.array(json.dumps(dict(K=K, nrs=nrs, common=case["common"], beam=case["beam"])))
            out[name + ".min_gap"] = np.array(case_gap)
    finally:
        GenerationMixin._get_top_k_continuations, GenerationMixin._get_running_beams_for_next_iteration = o_top, o_run
        GenerationMixin._update_finished_beams = o_fin
    save("gpt_generate_beams", **out)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "ab"
    if "a" in what:
        make_steps(HERE)
    if "b" in what:
        make_generate(sys.argv[2].split(",") if len(sys.argv) > 2 else None)
