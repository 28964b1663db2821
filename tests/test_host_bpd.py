"""Host side of the diffusion decoder's bits-per-dim loop (no GPU): the float64 restatement tests/bpd_ref.py against the reference's
own numbers in tests/golden/diff_bpd.npz, the seeded inputs against the stored checksums, the refusals that must fire before anything is
launched, and the C ABI."""
import os
import types

import numpy as np
import pytest

import bpd_inputs as BI
import bpd_ref as BR
import diff_loss_inputs as DI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# |float64 restatement on the stored fp32 model output - the reference's own fp32 result| relative to max(1, |value|), measured on the
# CPU by tests/golden/make_golden_bpd.py: vb 1.5e-7, xstart_mse 2.2e-8, mse 5.3e-8; x 20 (xstart_mse: 20 x one fp32 ulp of its 1.18)
REF_GATE = {"vb": 3e-6, "xstart_mse": 2.4e-6, "mse": 1.1e-6}
SYMBOLS = ("dtts_diff_bpd_terms", "dtts_diff_prior_bpd", "dtts_diff_calc_bpd")


def make_diffuser(loop, conditioning_free=False):
    from detail_tts_amd.vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    return SpacedDiffusion(BI.use_timesteps(loop, space_timesteps), betas=get_named_beta_schedule("linear", 4000),
                           conditioning_free=conditioning_free)


class NoLaunchRt:
    """a runtime on which every call except get_option is a test failure: what must be rejected is rejected before the device is used"""

    def __init__(self, trunk_fp16=0):
        self._fp16 = trunk_fp16

    def get_option(self, key):
        assert key == "trunk_fp16"
        return self._fp16

    def __getattr__(self, name):
        raise AssertionError(f"the runtime was reached ({name}) before the arguments were checked")


def test_seeded_inputs_are_the_ones_the_fixture_was_made_of(golden):
    g = golden("diff_bpd")
    inp = BI.loop_inputs(golden("diff_cond"))
    assert inp["x_start"].shape == (BI.B, 128, BI.T)
    for k, v in inp.items():
        assert np.array_equal(DI.checksum(v), g["f64_sum_" + k]), k
    assert (inp["x_start"][0] < -0.999).any() and (inp["x_start"][0] > 0.999).any()         # row 0: all three NLL branches
    for loop in BI.LOOPS:
        d = make_diffuser(loop)
        S = d.num_timesteps
        assert list(d.timestep_map) == g[loop + "_timestep_map"].tolist()
        assert np.array_equal(DI.checksum(BI.loop_noise(loop, S)), g["f64_sum_noise_" + loop]), loop
        for k in BI.KEYS:
            assert g[f"{loop}_{k}"].shape == (BI.B, S) and g[f"{loop}_{k}"].dtype == np.float32
        # total = sum of the columns + the prior, in the reference's own fp32 (its sum order is torch's: a few ulps of the total)
        tot = g[loop + "_vb"].astype(np.float64).sum(1) + g[loop + "_prior_bpd"]
        assert np.abs(tot - g[loop + "_total_bpd"]).max() < 4 * np.spacing(np.float32(g[loop + "_total_bpd"].max()))
    assert [make_diffuser(l).num_timesteps for l in BI.LOOPS] == [5, 200, 200]
    # the truncated schedule stops far from pure noise, so its prior is O(1); on the full ones it cancels
    assert np.isclose(make_diffuser("tr").alphas_cumprod[-1], float(g["f64_tr_last_alphas_cumprod"]), rtol=1e-13)
    assert 0.3 < float(g["f64_tr_last_alphas_cumprod"]) < 0.9
    assert g["tr_prior_bpd"].min() > 0.05 and g["s200_prior_bpd"].max() < 1e-4 and g["s5_prior_bpd"].max() < 1e-4


def test_float64_restatement_reproduces_the_terms_of_case_a(golden):
    """tests/bpd_ref.py on case A's stored model output (diff_losses.npz) gives the vb / xstart_mse / mse the reference's own
    _vb_terms_bpd, mean_flat and _predict_eps_from_xstart gave on it, within REF_GATE; the planted mistakes are mistakes here too"""
    import diff_loss_ref as DR
    g, gl = golden("diff_bpd"), golden("diff_losses")
    a = DI.case_a(golden("diff_cond"))
    d = make_diffuser("s200")
    x_t = DR.q_sample(d, a["x_start"], a["t"], a["noise"])
    args = (d, gl["a_model_output"], a["x_start"], x_t, a["noise"], a["t"])
    r = BR.terms(*args)
    for k in BI.KEYS:
        err = float((np.abs(r[k] - g["a_" + k]) / np.maximum(1.0, np.abs(g["a_" + k]))).max())
        print(f"bpd_ref case A {k}: {r[k]} reference {g['a_' + k]} err {err:.3e}")
        assert err < REF_GATE[k], (k, err)
    assert np.abs(r["pred_xstart"]).max() <= 1.0
    assert np.abs(g["a_vb"] - gl["a_vb"]).max() < 1e-6                       # the term training_losses returned for the same rows
    assert BR.terms(*args, unclamped=True)["xstart_mse"][2] > 100 * r["xstart_mse"][2]          # t = 199: x_t / sqrt_ac is O(100)
    assert abs(BR.terms(*args, mse_of_model_eps=True)["mse"][2] - r["mse"][2]) > 0.5
    assert abs(BR.terms(*args, drop_t0=True)["vb"][0] - r["vb"][0]) > 0.1


@pytest.mark.parametrize("loop", BI.LOOPS)
def test_float64_prior_reproduces_the_reference(golden, loop):
    """_prior_bpd: relative on the truncated schedule; on the full schedules -1 - lv + exp(lv) cancels to ~1e-9 per element in fp32, so
    the reference's own 6e-6 bits carry ~1 % of rounding noise and the comparison is absolute (generator: 4.4e-8 measured)"""
    g = golden("diff_bpd")
    p = BR.prior_bpd(make_diffuser(loop), BI.loop_inputs(golden("diff_cond"))["x_start"])
    ref = g[loop + "_prior_bpd"].astype(np.float64)
    print(f"prior {loop}: float64 {p} reference {ref}")
    if loop == "tr":
        assert (np.abs(p - ref) / ref).max() < 20 * 1.3e-8 + 6e-8          # 20 x the measured gap + one fp32 ulp of the stored value
    else:
        assert np.abs(p - ref).max() < BI.PRIOR_GATE["abs200"]


def test_gates_are_not_below_the_reference_vs_float64_gap():
    """the gaps tests/golden/make_golden_bpd.py printed (rel. to max(1, |value|)): loops vb 2.1e-7, xstart_mse 1.8e-7, mse 2.0e-7,
    total 1.5e-7, prior 4.4e-8 absolute; case A terms 1.5e-7 / 2.2e-8 / 5.3e-8"""
    gap = {"vb": 2.1e-7, "xstart_mse": 1.8e-7, "mse": 2.0e-7, "total_bpd": 1.5e-7, "prior_bpd": 4.4e-8}
    for k, v in gap.items():
        assert BI.LOOP_GATE[k] >= v, k
        if k in BI.TERM_GATE:
            assert BI.TERM_GATE[k] >= v, k
    assert BI.PRIOR_GATE["abs200"] >= gap["prior_bpd"] and BI.LOOP_ABS_GATE >= 8.9e-9


def kw(B=2, T=8):
    torch = pytest.importorskip("torch")
    return torch.zeros(B, 128, T), {"precomputed_aligned_embeddings": torch.zeros(B, 768, T)}


@pytest.mark.parametrize("entry", ["calc_bpd_loop", "_vb_terms_bpd"])
def test_refusals_fire_before_any_launch(entry):
    torch = pytest.importorskip("torch")
    x, emb = kw()
    model = types.SimpleNamespace(rt=NoLaunchRt())

    def call(d, model=model, **k):
        if entry == "calc_bpd_loop":
            return d.calc_bpd_loop(model, x, **k)
        return d._vb_terms_bpd(model, x, x, torch.tensor([0, 1]), **k)

    d = make_diffuser("s5")
    with pytest.raises(ValueError, match="clip_denoised"):
        call(d, clip_denoised=False, model_kwargs=emb)
    with pytest.raises(NotImplementedError, match="not a likelihood"):
        call(make_diffuser("s5", conditioning_free=True), model_kwargs=emb)
    with pytest.raises(NotImplementedError, match="three-product trunk"):
        call(d, model=types.SimpleNamespace(rt=NoLaunchRt(trunk_fp16=1)), model_kwargs=emb)
    with pytest.raises(ValueError, match="precomputed_aligned_embeddings"):
        call(d, model_kwargs={"aligned_conditioning": x})
    with pytest.raises(ValueError, match="precomputed_aligned_embeddings"):
        call(d)
    if entry == "_vb_terms_bpd":
        with pytest.raises(ValueError):
            d._vb_terms_bpd(model, x, x, torch.tensor([0, 5]), model_kwargs=emb)


def test_calc_bpd_loop_does_not_take_the_sampling_loops_refusal():
    """a conditioning_free=False diffuser's sampling loops stay refused (_check); the likelihood loop of that same diffuser reaches the
    runtime instead - here a runtime that records the call"""
    torch = pytest.importorskip("torch")
    x, emb = kw()
    d = make_diffuser("s5")
    with pytest.raises(NotImplementedError, match="conditioning_free=False sampling"):
        d.p_sample_loop(types.SimpleNamespace(rt=NoLaunchRt()), (2, 128, 8), model_kwargs=emb)
    calls = []

    class Rt(NoLaunchRt):
        def diff_schedule(self, tmap):
            calls.append(("schedule", list(tmap)))
            return 3

        def diff_calc_bpd(self, sched, x_start, code_emb, **k):
            calls.append(("calc_bpd", sched, tuple(x_start.shape), k))
            return {"total_bpd": "sentinel"}

    out = d.calc_bpd_loop(types.SimpleNamespace(rt=Rt()), x, model_kwargs=emb, seed=9, sample_ids=[4, 5], rows_per_pass=7)
    assert out == {"total_bpd": "sentinel"}
    assert calls[0] == ("schedule", list(d.timestep_map))
    assert calls[1][:3] == ("calc_bpd", 3, (2, 128, 8))
    assert calls[1][3] == dict(noise=None, seed=9, sample_ids=[4, 5], rows_per_pass=7)


def test_prior_bpd_needs_a_runtime():
    torch = pytest.importorskip("torch")
    with pytest.raises(RuntimeError, match="Runtime"):
        make_diffuser("s5")._prior_bpd(torch.zeros(1, 128, 8))


def test_diffusion_bpd_refuses_the_fp16_trunk_first():
    torch = pytest.importorskip("torch")
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    fake = types.SimpleNamespace(rt=NoLaunchRt(trunk_fp16=1), device="cpu")
    with pytest.raises(NotImplementedError, match="three-product trunk"):
        SynthesizerTrn.diffusion_bpd(fake, None, None, dict(raw_mel=torch.zeros(2, 128, 8)))


def test_the_c_abi_declares_and_exports_the_new_entries():
    from detail_tts_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "detail_hip.h")).read()
    lib = _lib.load()
    for s in SYMBOLS:
        assert f"int {s}(dtts_handle* h, int id," in hdr, s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
    for cite in ("vqvae/utils/diffusion.py:1114-1169", ":903-928", "vqvae/utils/diffusion.py:1098-1112", ":402-405"):
        assert cite in hdr, cite
    assert "noise stage 7" in hdr and "rows_per_pass" in hdr
    # the new noise stage is no other site's
    common = open(os.path.join(ROOT, "detail_tts_amd", "csrc", "common.h")).read()
    import re
    stages = dict(re.findall(r"(STAGE_\w+) = (\d+)", common))
    assert stages["STAGE_DIFF_BPD"] == "7" and list(stages.values()).count("7") == 1
    from oracle import philox
    assert 7 not in (philox.STAGE_GPT_SAMPLE, philox.STAGE_DIFF_INIT, philox.STAGE_DIFF_STEP, philox.STAGE_FLOW_PRIOR)
