"""Seeded inputs of tests/golden/diff_losses.npz (the recipe of tests/golden/make_golden_diff_losses.py; the fixture stores float64
checksums of every array made here, the reference's results for them, and the timesteps).  Stored in full, the inputs and the
reference's model output would not fit the fixture's 128 KiB together, so everything the generator itself draws is drawn here."""
import numpy as np

B_A, T_A = 3, 36
T_A_STEPS = (0, 1, 199)
SEED_A, SEED_B, SEED_C, SEED_B_NOISE = 51, 52, 53, 54

# Gates of the end-to-end losses against the reference's stored values (tests/test_gpu_diff_losses.py): 20 x what the MI355X measured
# (profiles/diff_losses_measured_errors.txt) - mse 1.2e-7, vb 1.2e-7, loss 4.8e-7, forward_diff 1.2e-7 (one fp32 ulp of the value each);
# forward_vq measured 0, so its gate is 20 x one fp32 ulp of the value (5.02: 4.8e-7).  tests/golden/make_golden_diff_losses.py asserts
# that every mistake the fixture must see moves a stored value by more than 20 x these.
GATES = {"mse": 2.5e-6, "vb": 2.5e-6, "loss": 1e-5, "forward_diff": 2.5e-6, "forward_vq": 1e-5}


def checksum(a):
    a = np.asarray(a, np.float64).reshape(-1)
    return np.array([a.sum(), (a * np.arange(1, a.size + 1) % 7.0).sum()], np.float64)


def case_a(diff_cond):
    """Case A, training_losses at B = 3, T = 36, t = (0, 1, 199): x_start in the normalised mel's range with a handful of entries of the
    t = 0 row pushed beyond +-0.999 (all three branches of the discretised NLL), the given noise, and aligned_conditioning /
    conditioning_latent made of tests/golden/diff_cond.npz (9 of its 12 latent frames; row b rolled by b frames and scaled)."""
    rs = np.random.RandomState(SEED_A)
    x = np.clip(rs.randn(B_A, 128, T_A) * 0.4 - 0.2, -0.95, 0.95).astype(np.float32)
    hi = rs.choice(128 * T_A, 24, replace=False)
    flat = x[0].reshape(-1)
    flat[hi[:12]] = np.float32(1.0) - rs.rand(12).astype(np.float32) * np.float32(5e-4)         # > 0.999
    flat[hi[12:]] = np.float32(-1.0) + rs.rand(12).astype(np.float32) * np.float32(5e-4)        # < -0.999
    noise = rs.randn(B_A, 128, T_A).astype(np.float32)
    lat = np.asarray(diff_cond["latent"], np.float32)[0, : T_A // 4]                               # [9, 768]
    aligned = np.stack([np.roll(lat, b, 0) * np.float32(1.0 + 0.1 * b) for b in range(B_A)]).astype(np.float32)
    cond = np.repeat(np.asarray(diff_cond["cond_latent"], np.float32), B_A, 0)
    return dict(x_start=x, noise=noise, aligned=aligned, cond=cond, t=np.array(T_A_STEPS, np.int64))


def case_b(gpt_forced):
    """Case B, forward_diff on two rows: y = the 64-frame prompt of tests/golden/gpt_forced.npz (row 1 reversed in time), its 13 text ids
    at full width in both rows (row 1 reversed, the trailing 0 kept), raw_mel of 36 frames, full-length raw_wav_length."""
    rs = np.random.RandomState(SEED_B)
    refer = np.asarray(gpt_forced["refer"], np.float32)
    y = np.concatenate([refer, refer[:, :, ::-1]], 0).copy()
    text = np.asarray(gpt_forced["text"], np.int64)
    text = np.concatenate([text, np.concatenate([text[:, -2::-1], text[:, -1:]], 1)], 0)
    raw_mel = (rs.randn(2, 128, 36) * 2 - 5).astype(np.float32)
    return dict(y=y, y_lengths=np.array([64, 64]), raw_mel=raw_mel, raw_spec_length=np.array([36, 36]), text=text,
                text_length=np.array([text.shape[1]] * 2), raw_wav_length=np.array([36 * 256] * 2))


def case_b_noise():
    """the noise the reference's training_losses was handed when it asked torch.randn_like for it (the generator patches that call)"""
    return np.random.RandomState(SEED_B_NOISE).randn(2, 128, 36).astype(np.float32)


def case_c():
    """Case C, forward_vq on two rows of 36 frames with y_lengths = (36, 28)"""
    rs = np.random.RandomState(SEED_C)
    return dict(y=(rs.randn(2, 128, 36) * 2 - 5).astype(np.float32), y_lengths=np.array([36, 28]))
