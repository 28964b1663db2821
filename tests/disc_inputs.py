"""Seeded inputs of tests/golden/disc_losses.npz (the recipe of tests/golden/make_golden_disc.py; the fixture stores float64 checksums of
every array made here and the reference's results for them) and the gates of tests/test_gpu_disc.py.

Case A: B = 2, t = 10240 (train.segment_size): 10240 % p = 0, 1, 0, 6, 10 for p = 2, 3, 5, 7, 11 - the unpadded and the padded branch.
Case B: B = 3, t = 97 (prime: every period pads; DiscriminatorS shrinks 97 -> 25 -> 7 -> 2 -> 1; p = 11 has H = 9 -> 3 -> 1).
Case C: loss_mel of the flow-VAE stage on flowvae_inputs.case() with the waveform of wav_c()."""
import numpy as np

SEED_A, SEED_B, SEED_WAV = 91, 92, 93
A_B, A_T = 2, 10240
B_B, B_T = 3, 97
PERIODS = (2, 3, 5, 7, 11)
N_MAPS = 37                            # 7 of DiscriminatorS (6 convs + conv_post), 6 of each DiscriminatorP
A_SAMPLES, B_FULL, B_SAMPLES = 64, 256, 128

# Gates of tests/test_gpu_disc.py: 20 x the errors measured on the MI355X (profiles/disc_measured_errors.txt; where several comparisons
# share a gate, 20 x the largest of them).  tests/golden/make_golden_disc.py asserts that every mistake the fixture must see moves a
# stored value by more than 20 x these (profiles/disc_fixture_margins.txt).
#   score / map: max |device - reference| over a tensor's stored samples, relative to the largest stored magnitude of that tensor
#   (relerr), worst over all tensors: case A scores 2.9e-6, case A maps 3.0e-6, case B stored elements 3.1e-6.
#   full: every element of every case-B tensor against float64 (disc_ref), same normalisation: 3.2e-6.
#   mom_sum / mom_sumsq: the float64 sum over each WHOLE case-A tensor relative to its sum of magnitudes, and its sum of squares
#   relative to itself: 3.0e-7 / 6.9e-7 (spec_to_mel's sum: 4.0e-8).
#   loss: the scalars and lists of the three loss functions on the device's own maps against the reference's fp32, relative to
#   max(1, |ref|): at most 2.3e-7 (case B losses_r; loss_fm and loss_gen equal the reference's fp32 bit for bit in both cases).
#   map_mean: the 37 per-map mean |r - g| against float64 of the reference's maps, relative: 4.8e-7.
#   grouped: op_conv1d_grouped against float64, relative to max(1, |ref|): 4.2e-7 / 1.5e-7 / 9.6e-8 / 4.5e-7.
#   reduce: the reductions alone against float64, relative: 7.0e-8 / 7.8e-8 / 6.5e-8.
#   spec_to_mel: samples against the reference, absolute (log-mel values of magnitude up to 11): 9.5e-7.
#   loss_mel: the stage's scalar equals the reference's fp32 (138.123398) bit for bit; the gate is 20 fp32 ulps of it (1.1e-7 each,
#   relative).  stage_gan: the stage's loss_fm / loss_disc / loss_gen (on the device's own o) against the reference's, relative: 1.4e-7.
GATES = {"score": 5.7e-5, "map": 6.2e-5, "full": 6.4e-5, "mom_sum": 5.9e-6, "mom_sumsq": 1.4e-5, "loss": 4.7e-6, "map_mean": 9.5e-6,
         "grouped": 9.1e-6, "reduce": 1.6e-6, "spec_to_mel": 1.9e-5, "loss_mel": 2.2e-6, "stage_gan": 2.8e-6}


def _signal(rs, B, t):
    """band-limited: a few sinusoids below 4 kHz (at 24 kHz) plus noise, clipped to [-1, 1]"""
    n = np.arange(t)[None, :]
    x = np.zeros((B, t))
    for _ in range(4):
        f = rs.uniform(80.0, 4000.0, size=(B, 1)) / 24000.0
        x += rs.uniform(0.2, 0.45, size=(B, 1)) * np.sin(2 * np.pi * f * n + rs.uniform(0, 2 * np.pi, size=(B, 1)))
    x += 0.15 * rs.randn(B, t)
    return np.clip(x, -1.0, 1.0).astype(np.float32)[:, None, :]


def case_a():
    rs = np.random.RandomState(SEED_A)
    return dict(y=_signal(rs, A_B, A_T), y_hat=_signal(rs, A_B, A_T))


def case_b():
    rs = np.random.RandomState(SEED_B)
    return dict(y=_signal(rs, B_B, B_T), y_hat=_signal(rs, B_B, B_T))


def wav_c(B=2, frames=48, hop=256):
    return _signal(np.random.RandomState(SEED_WAV), B, frames * hop)


def checksum(a):
    a = np.asarray(a, np.float64).reshape(-1)
    return np.array([a.sum(), (a * np.arange(1, a.size + 1) % 7.0).sum()], np.float64)


def moments(a):
    """float64 (sum, sum of squares, sum of magnitudes) of a tensor"""
    a = np.asarray(a, np.float64)
    return np.array([a.sum(), np.square(a).sum(), np.abs(a).sum()], np.float64)


def sample_a(a):
    """about A_SAMPLES strided elements of a case-A tensor, in its reference shape's row-major order"""
    a = np.asarray(a).reshape(-1)
    return a[::max(1, -(-a.size // A_SAMPLES))]


def sample_b(a):
    """a case-B tensor in full when it has at most B_FULL elements, else about B_SAMPLES strided ones"""
    a = np.asarray(a).reshape(-1)
    return a if a.size <= B_FULL else a[::-(-a.size // B_SAMPLES)]


def slot(kind, side, i):
    """row of a tensor in the fixture's tables: per side (r, then g) the 6 scores, then the 37 maps"""
    return (0 if side == "r" else 6 + N_MAPS) + (i if kind == "score" else 6 + i)


def stored(g, tag, kind, side, i):
    """-> (the stored samples, the float64 moments) of one tensor of case `tag`: the fixture keeps the samples of all 86 tensors of a
    case in one array (`<tag>_samples`, rows delimited by `<tag>_sample_off`) and their moments in one table (`f64_<tag>_mom`)"""
    k, off = slot(kind, side, i), g[f"{tag}_sample_off"]
    return g[f"{tag}_samples"][off[k]:off[k + 1]], g[f"f64_{tag}_mom"][k]


def relerr(a, ref):
    """max |a - ref| relative to the largest magnitude in ref: how the scores' and maps' gates are taken (the maps' magnitudes span
    0.02 .. 1 rms, and so do their rounding errors)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


def flat_maps(fmaps):
    """6 lists of maps -> the 37 maps in order"""
    return [m for d in fmaps for m in d]
