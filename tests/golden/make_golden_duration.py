#!/usr/bin/env python3
"""tests/golden/duration_emb.npz: THE REFERENCE'S OWN DiffusionTts.timestep_independent (vqvae/diff_model.py:231-260) at frame counts
other than 4 n - the hook the speaking-rate control rides on: F.interpolate(code_emb, size=expected_seq_len, mode='nearest') (:252).

Runs only in the build container (needs the reference checkout and transformers), on the CPU, in eval mode, under the shim of
make_golden.py with the seed-0 synthetic weights.  Data only: per case (n, T) in CASES one seeded latent [1, n, 768], the one
conditioning latent [1, 1536] (diff_cond.npz's, stored again so that the file stands alone) and the reference's result, every
CH_STRIDE-th channel of [1, 768, T] (24 channels per GroupNorm group: every group is sampled).  The three expanded cases are the
pairs at which floor(t n / T) is not torch's index map; (12, 12) is the UNEXPANDED embedding of the (12, 148) latent - np.repeat of
it is what a durations plan expects.

The script asserts, before it stores anything:
  (a) each expanded result is the (n, n) result of the same latent gathered by tests/duration_ref.uniform_map, bit for bit - the
      restated float32 rule IS what the reference ran - and is NOT the gather by floor(t n / T);
  (b) the (12, 148) result's columns are (12, 12)'s under that map.

    python tests/golden/make_golden_duration.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/duration_ref.py

import make_golden as MG  # noqa: E402
import duration_ref as R  # noqa: E402

CASES = ((14, 92), (26, 44), (12, 148), (12, 12))
CH_STRIDE = 4


def main():
    MG.install_shim()
    import torch
    torch.set_grad_enabled(False)
    m = MG.build_reference_model()
    assert not m.diffusion.training
    cond = torch.from_numpy(dict(np.load(os.path.join(HERE, "diff_cond.npz")))["cond_latent"])
    rs = np.random.RandomState(77)
    lat = {n: rs.randn(1, n, 768).astype(np.float32) for n in sorted({n for n, _ in CASES})}
    run = lambda n, T: m.diffusion.timestep_independent(torch.from_numpy(lat[n]), cond, T, False).numpy()  # noqa: E731
    out = {"cond_latent": cond.numpy(), "ch_stride": np.array(CH_STRIDE), "cases": np.array(CASES)}
    for n, T in CASES:
        emb, plain = run(n, T), run(n, n)
        assert emb.shape == (1, 768, T) and emb.dtype == np.float32 and np.isfinite(emb).all()
        if T != n:
            assert np.array_equal(emb, plain[:, :, R.uniform_map(n, T)]), (n, T)                 # (a)
            assert not np.array_equal(emb, plain[:, :, R.floor_map(n, T)]), (n, T)
        out[f"latent_{n}"] = lat[n]
        out[f"emb_{n}_{T}"] = emb[:, ::CH_STRIDE]
        print(f"({n}, {T}): max |emb| {np.abs(emb).max():.3f}")
    assert np.array_equal(out["emb_12_148"], out["emb_12_12"][:, :, R.uniform_map(12, 148)])   # (b)
    MG.save("duration_emb", **out)
    size = os.path.getsize(os.path.join(HERE, "duration_emb.npz"))
    print("duration_emb.npz:", size, "bytes")
    assert size <= 512 * 1024, size


if __name__ == "__main__":
    main()
