"""Seeded inputs of tests/golden/flowvae.npz (the recipe of tests/golden/make_golden_flowvae.py; the fixture stores float64 checksums
of every array made here and the reference's results for them) and the gates of tests/test_gpu_flowvae.py.  Stored in full the
inputs alone (a [2, 513, 48] spectrogram, a [2, 192, 48] noise) would not fit the fixture's 128 KiB.

The case: B = 2, T = 48, y_lengths = (48, 44), segments of 40 frames; the fractions handed to the reference's torch.rand give
ids_slice = (8, 0): the last valid start of a full row (48 - 40) and the first start of a ragged one."""
import numpy as np

B, T, SEG = 2, 48, 40
LENGTHS = (48, 44)
SPEC_CHANNELS = 513
INTER = 192
IDS_SLICE = (8, 0)
RAND_FRACTIONS = (0.95, 0.1)          # floor(0.95 * (48 - 40 + 1)) = 8, floor(0.1 * (44 - 40 + 1)) = 0
SEED_Y, SEED_SPEC, SEED_NOISE, SEED_FLOW = 61, 62, 63, 64

LATENT_STRIDE = (4, 3)                 # stored samples of the [2, 192, 48] tensors: [:, ::4, ::3] (t = 45, beyond row 1's length, included)
WAV_STRIDE = 8                         # ... and of o [2, 1, 10240]
LATENTS = ("z", "z_p", "m_p", "logs_p", "m_q", "logs_q")

# Gates of tests/test_gpu_flowvae.py: 20 x the errors measured on the MI355X (profiles/flowvae_measured_errors.txt; where several
# comparisons share a gate, 20 x the largest of them).  tests/golden/make_golden_flowvae.py asserts that every mistake the fixture must
# see moves a stored value by more than 20 x these.
#   max |device - reference| over the stored samples: z 1.7e-6, z_p 1.7e-6, m_p 8.3e-7, logs_p 7.7e-7, m_q 7.5e-7, logs_q 9.5e-7,
#   quantized 1.4e-6, o 1.4e-8; every element of enc_q's outputs and the flow's against float64: z 2.3e-6 (2.4e-6 piece by piece),
#   m_q 8.8e-7, logs_q 8.3e-7, z_p 2.4e-6; the generator alone on the reference's g against the stage call: 1.6e-8.
#   kl: the device's scalar equals the reference's fp32 (70.530983) bit for bit; the gate is 20 fp32 ulps of it (7.6e-6 each).
#   flow: case B 4.8e-7.  wn (16 layers alone, relative to max(1, |ref|), against float64): 3.7e-7 split-precision route, 4.9e-7 fp32 route.
#   kl_f64 (the kernel against float64, relative): 2.2e-8 / 4.2e-8 / 3.7e-8.  round_trip (flow(flow^-1(z_p)) - z_p): 7.2e-7.
#   g_row0 (the per-row ref_enc entry against the reference's g on the full-length row): 2.4e-7.  philox (z against m_q + eps exp(logs_q)
#   with eps from the Philox unit entry, relative): 7.0e-8.
GATES = {"z": 4.8e-5, "z_p": 4.8e-5, "m_p": 1.7e-5, "logs_p": 1.6e-5, "m_q": 1.8e-5, "logs_q": 1.9e-5, "quantized": 2.9e-5, "o": 3.2e-7,
         "kl": 1.5e-4, "flow": 9.5e-6, "wn": 1e-5, "kl_f64": 8.5e-7, "round_trip": 1.4e-5, "g_row0": 4.8e-6, "philox": 1.4e-6}
# ... and of the float64 (sum, sum of squares) over each WHOLE tensor of the stage call against the reference's, the check on the
# elements the fixture does not sample: 20 x the measured |difference| (same file, flowvae_<k>_sum / _sumsq)
#   measured: z 8.3e-5 / 4.6e-4, z_p 6.9e-5 / 4.0e-4, m_p 7.1e-5 / 3.4e-5, logs_p 2.9e-5 / 1.5e-5, m_q 1.3e-4 / 5.7e-5,
#   logs_q 5.6e-5 / 5.9e-5, quantized 7.6e-6 / 2.6e-5, o 2.0e-5 / 2.5e-7
MOMENT_GATES = {"z": (1.7e-3, 9.2e-3), "z_p": (1.4e-3, 8e-3), "m_p": (1.5e-3, 6.9e-4), "logs_p": (5.9e-4, 3.1e-4), "m_q": (2.7e-3, 1.2e-3),
                "logs_q": (1.2e-3, 1.2e-3), "quantized": (1.6e-4, 5.3e-4), "o": (4e-4, 5.1e-6)}


def checksum(a):
    a = np.asarray(a, np.float64).reshape(-1)
    return np.array([a.sum(), (a * np.arange(1, a.size + 1) % 7.0).sum()], np.float64)


def moments(a):
    """float64 (sum, sum of squares) of a tensor, stored next to its samples"""
    a = np.asarray(a, np.float64)
    return np.array([a.sum(), np.square(a).sum()], np.float64)


def case():
    """y: a log-mel in its usual range; spec: linear magnitudes (positive, a few large bins); noise: enc_q's eps"""
    y = (np.random.RandomState(SEED_Y).randn(B, 128, T) * 2 - 5).astype(np.float32)
    rs = np.random.RandomState(SEED_SPEC)
    spec = (np.abs(rs.randn(B, SPEC_CHANNELS, T)) * np.exp(rs.randn(B, SPEC_CHANNELS, 1) * 0.5) * 0.6).astype(np.float32)
    noise = np.random.RandomState(SEED_NOISE).randn(B, INTER, T).astype(np.float32)
    return dict(y=y, y_lengths=np.array(LENGTHS, np.int64), spec=spec, noise=noise)


def flow_case():
    """a latent with NON-ZERO tails for the flow alone (the reference masks x1 inside every coupling layer; enc_q's z cannot show that,
    its tails are zero already)"""
    return (np.random.RandomState(SEED_FLOW).randn(B, INTER, T) * 0.8).astype(np.float32)


def sample(a):
    a = np.asarray(a)
    if a.shape[1] == 1:
        return a[:, :, ::WAV_STRIDE]
    return a[:, ::LATENT_STRIDE[0], ::LATENT_STRIDE[1]]
