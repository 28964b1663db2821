"""Shared by tests/golden/make_golden_invert.py, tests/test_host_invert.py and tests/test_gpu_invert.py: what the DDIM inversion fixture
(tests/golden/ddim_reverse.npz) stores, how it is subsampled, and the gates of the GPU tests - in one place, so
that the fixture script can assert every planted mistake moves a stored value by more than 20 x the gate that guards it.

The setting: seed-0 synthetic weights, the T = 48 code embedding of sampler_chains.npz, the 10-step conditioning_free=True diffuser,
x_start = sampler_chains' ddim0_final."""
import numpy as np

N_STEPS = 10
STEPS = (0, 4, 9)                 # teacher-forced ddim_reverse_sample steps: the first, a middle one (both clamp branches), the last (ab_next = 0)
PMV_STEPS = (9, 0)                # p_mean_variance, on sampler_chains' p_x_before_9 / p_x_before_0
PMV_KEYS = ("mean", "variance", "log_variance", "pred_xstart")
ROUND_TRIP_DEPTH = 5
SPLIT_LEVEL = 5
CH_STRIDE = 4                     # compared outputs are stored at every 4th mel channel (all 48 frames); tensors that are fed back, whole
PMV_CH_STRIDE = 8

# Depths at which the free-running inversion chain is compared with the reference's.  The chain is sensitive to its input (1e-5 of noise
# on x_start moves depth 9 by 7e-3), so a depth is usable only while 20 x the measured device error still sits a factor 20 below the
# smallest planted-mistake margin at that depth: make_golden_invert.py asserts that, profiles/ddim_reverse_measured_errors.txt has the
# measurements (the device stays 1.2e-5 off the reference's chain down to depth 10).
CHAIN_DEPTHS = (1, 5, 9)

# ---- gates of tests/test_gpu_invert.py: ~20 x the max-abs error measured on an MI355X over both kernel sets
# (profiles/ddim_reverse_measured_errors.txt), never below the reference's own fp32-against-float64 gap (make_golden_invert.py prints
# it: 3.2e-6 at t = 0, <= 5.5e-7 above; stored as f64_gap), never above 1/20 of the smallest planted-mistake margin (asserted there).
STEP_SAMPLE_GATE = {0: 9e-5, 4: 5e-5, 9: 5e-5}                    # measured 4.3e-6, 2.3e-6, 2.2e-6
# pred_xstart carries the forward's error times sqrt(1 / alpha_bar - 1): 0.005 at t = 0 (one ulp of 1.0 measured), ~150 at t = 9
STEP_X0_GATE = {0: 1.2e-6, 4: 2.6e-4, 9: 7e-3}                    # measured 6.0e-8, 1.3e-5, 3.4e-4
PMV_GATE = {(9, "mean"): 2.5e-5, (9, "variance"): 1.2e-6, (9, "log_variance"): 6e-7, (9, "pred_xstart"): 1.4e-3,
            (0, "mean"): 1.2e-6, (0, "variance"): 1e-9, (0, "log_variance"): 4e-5, (0, "pred_xstart"): 1.2e-6}
#                                 measured 1.1e-6, 6.0e-8, 3.0e-8, 6.9e-5 at t = 9 and 6.0e-8, 4.7e-11, 1.9e-6, 6.0e-8 at t = 0
CHAIN_GATE = {1: 9e-5, 5: 2.4e-4, 9: 2.5e-4}                      # measured 4.3e-6, 1.18e-5, 1.21e-5
ROUND_TRIP_GATE = 1.6e-4          # normalised mel (measured 8.0e-6); resynthesize's de-normalised mel is compared at DENORM_SCALE x this
SPLIT_GATE = 2e-3                 # t_start = 5 from the reference's own x at level 5 against ddim0_final: test_gpu_sampler's ddim0 chain gate
RAGGED_ROW_GATE = 1.2e-2          # a row of a ragged batch against the row alone: test_ragged_batch8_ddim_eta_rows_equal_alone's
DENORM_SCALE = (2.7 - (-11.512925465)) / 2.0


def sub(a, stride=CH_STRIDE):
    """the stored view of a [1, 128, T] (or [128, T]) tensor: every `stride`-th channel, every frame"""
    a = np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
    a = a[0] if a.ndim == 3 else a
    return np.ascontiguousarray(a[::stride])


def pairing(n, depth):
    """depth of an inversion -> the t_start that consumes it (None: depth n is pure eps' and feeds a whole loop as `noise`)"""
    if not 1 <= depth <= n:
        raise ValueError(depth)
    return depth if depth <= n - 1 else None
