"""Shared by tests/golden/make_golden_inpaint.py, tests/test_host_inpaint.py and tests/test_gpu_inpaint.py: what the inpainting fixture
(tests/golden/inpaint.npz) stores, how its noise is rebuilt, and the gates of the GPU parity test - in one place, so that the fixture
script can assert that every planted mistake moves a stored value by more than 20 x the gate that guards it.

The setting is invert_inputs': seed-0 synthetic weights, the T = 48 code embedding of sampler_chains.npz, the 10-step
conditioning_free=True diffuser; x_T = sampler_chains' ddim0_x_init, known = its ddim0_final, the span is frames 16 .. 31 (codes 4 .. 7)."""
import numpy as np

from invert_inputs import CH_STRIDE, N_STEPS, sub  # noqa: F401

T = 48
SPAN_CODES = (4, 7)
SPAN = slice(16, 32)
CHAINS = (("ddim", 1), ("ddim", 2), ("p", 1), ("p", 2))           # (sampler, resample U)
STORED_AFTER = (7, 4, 0)                                          # x after the last repeat of these steps (0: the final x)
NOISE_SEED = 20240607


def name(sampler, U):
    return f"{sampler}{U}"


def keep_mask():
    k = np.ones((1, T), bool)
    k[:, SPAN] = False
    return k


def noises(sampler, U, first_step=N_STEPS - 1):
    """the three override arrays of a chain, (step_noise, known_noise, renoise), each [first_step * U + 1, 1, 128, T] fp32: integers in
    [-512, 512] over 256 from a PCG64 stream of their own - exact on every machine, so nothing of them is stored but a checksum"""
    rng = np.random.Generator(np.random.PCG64([NOISE_SEED, CHAINS.index((sampler, U))]))
    shape = (first_step * U + 1, 1, 128, T)
    return tuple((rng.integers(-512, 513, shape) / 256).astype(np.float32) for _ in range(3))


# ---- gates of tests/test_gpu_inpaint.py::test_chains_against_the_reference: ~20 x the max-abs error measured on an MI355X
# (profiles/inpaint_measured_errors.txt), per chain over the three stored tensors; never below the fixture's own fp32-against-float64
# gap (stored as f64_gap, asserted by the fixture script and by test_host_inpaint.py), and at most 1/20 of the smallest planted-mistake
# movement (make_golden_inpaint.py asserts it).  (ddim, 1) is the loosest: it carries a 1e-6 perturbation of x_T to 5.8e-5 (the others: 4e-6).
CHAIN_GATE = {"ddim1": 5e-4, "ddim2": 9e-5, "p1": 1.1e-4, "p2": 9e-5}            # measured 2.30e-5, 4.08e-6, 5.22e-6, 3.99e-6
