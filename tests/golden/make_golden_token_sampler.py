#!/usr/bin/env python3
"""Generate tests/golden/token_sampler_edges.npz FROM THE REFERENCE's logits processors (see make_golden.py for the setting).

For every case of tests/test_host_token_sampler.py::CASES the reference's processors run in the order its generate() applies them:
HF RepetitionPenaltyLogitsProcessor, the reference's own TypicalLogitsWarper (gpt/modules/typical_sampling.py, where the case has a
mass), HF TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper.  The logits and histories are NOT stored: a case is a numpy
RandomState seed plus a documented transform (case_inputs), the fixture holds their SHA-1.  Stored per case: the parameters, the
seed, V, the hash, the kept mask (np.packbits per row), HF's filtered values at the kept positions, and - where the top-p cut falls
inside a group of equal values, whose order torch.sort leaves undefined - the group's value and only HOW MANY of it HF kept (the
group's members are then absent from the mask).  Data only.

    python tests/golden/make_golden_token_sampler.py [out_dir]        # default: this directory
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)


def main(out_dir):
    import torch
    from make_golden import install_shim
    install_shim()
    from transformers import (LogitsProcessorList, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                              TopPLogitsWarper)
    from gpt.modules.typical_sampling import TypicalLogitsWarper
    import test_host_token_sampler as H

    torch.manual_seed(0)
    torch.set_num_threads(1)
    out = {"cases": np.array(sorted(H.CASES))}
    for name in sorted(H.CASES):
        c = H.CASES[name]
        p = c["params"]
        logits, hist = H.case_inputs(name)
        procs = [RepetitionPenaltyLogitsProcessor(float(p["rp"]))]
        if p["mass"]:
            procs.append(TypicalLogitsWarper(mass=float(p["mass"])))
        procs.append(TemperatureLogitsWarper(float(p["temp"])))
        if p["top_k"]:
            procs.append(TopKLogitsWarper(int(p["top_k"])))
        pre = LogitsProcessorList(procs)(torch.from_numpy(hist), torch.from_numpy(logits.copy())).numpy()
        procs.append(TopPLogitsWarper(float(p["top_p"])))
        f = LogitsProcessorList(procs)(torch.from_numpy(hist), torch.from_numpy(logits.copy())).numpy()
        assert f.dtype == np.float32 and f.shape == logits.shape
        kept = np.isfinite(f)
        assert np.array_equal(f[kept], pre[kept])
        sval = np.full(c["R"], np.nan, np.float32)
        scnt = np.full(c["R"], -1, np.int64)
        for r in range(c["R"]):
            for v in np.unique(pre[r][np.isfinite(pre[r])]):
                g = pre[r] == v
                k = int(kept[r][g].sum())
                if 0 < k < int(g.sum()):                     # the cut fell inside this tie group: keep the count, drop the members
                    assert scnt[r] < 0, (name, r)
                    sval[r], scnt[r] = v, k
                    kept[r][g] = False
        out[name + ".params"] = np.array([p["rp"], p["temp"], p["top_k"], p["top_p"], p["mass"]], np.float64)
        out[name + ".seed"] = np.array(c["seed"])
        out[name + ".V"] = np.array(c["V"])
        out[name + ".sha1"] = np.array(H.input_hash(logits, hist))
        out[name + ".kept"] = np.packbits(kept, axis=1)
        out[name + ".nkept"] = kept.sum(1).astype(np.int64)
        out[name + ".values"] = np.concatenate([f[r][kept[r]] for r in range(c["R"])]).astype(np.float32)
        out[name + ".straddle_value"] = sval
        out[name + ".straddle_count"] = scnt
        print(f"{name:20s} V {c['V']:5d} kept {kept.sum(1).tolist()} straddle {scnt.tolist()}")
    path = os.path.join(out_dir, "token_sampler_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
