"""GPU: DDIM inversion and partial-depth resampling in the diffusion decoder - ddim_reverse_sample / p_mean_variance / p_sample / ddim_sample
and the progressive loops on SpacedDiffusion, ddim_reverse_sample_loop (dtts_diff_invert), t_start on the sampling loops
(dtts_diff_sample_from), SynthesizerTrn.invert_mel / resynthesize - against the reference's own runs (ddim_reverse.npz:
tests/golden/make_golden_invert.py; sampler_chains.npz).  Gates: tests/invert_inputs.py; measurements:
profiles/ddim_reverse_measured_errors.txt."""
import numpy as np
import pytest

import invert_inputs as II
from conftest import tol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = II.N_STEPS


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def tt(i, B=1):
    return torch.full((B,), int(i), dtype=torch.long)


@pytest.fixture(scope="module")
def synth(weights):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(weights, folded=True)


@pytest.fixture(scope="module")
def S(golden):
    return golden("sampler_chains")


@pytest.fixture(scope="module")
def R(golden):
    return golden("ddim_reverse")


def _diffuser(n=N, sampler="ddim"):
    from detail_tts_amd.vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    return SpacedDiffusion(space_timesteps(4000, [n]), betas=get_named_beta_schedule("linear", 4000), conditioning_free=True,
                           conditioning_free_k=2.0, sampler=sampler)


@pytest.fixture(scope="module")
def kw(S):
    return {"precomputed_aligned_embeddings": dev(S["code_emb"])}


@pytest.fixture(scope="module")
def inverted(synth, S, kw):
    """ddim_reverse_sample_loop from ddim0_final through all 10 steps, with the trajectory: computed once, read by several tests"""
    r = _diffuser().ddim_reverse_sample_loop(synth.diffusion, dev(S["ddim0_final"]), kw, return_trajectory=True)
    return {k: host(v) for k, v in r.items()}


@pytest.mark.parametrize("x3", [1, 0])
def test_ddim_reverse_sample_teacher_forced_golden(synth, S, R, kw, x3):
    """ddim_reverse_sample at t = 0, 4, 9 with x TEACHER-FORCED from the fixture (step 0: both clamp branches and the 200-fold
    amplification of eps'; step 4: both branches; step 9: alphas_cumprod_next = 0), `sample` and `pred_xstart` against the reference's,
    on both kernel sets."""
    d = _diffuser()
    synth.rt.set_option("conv_x3", x3)
    try:
        for j, t in enumerate(II.STEPS):
            x = S["ddim0_final"] if t == 0 else R[f"rev_x_before_{t}"]
            r = d.ddim_reverse_sample(synth.diffusion, dev(x), tt(t), model_kwargs=kw)
            es, e0 = maxabs(II.sub(r["sample"]), R["chain_x"][t]), maxabs(II.sub(r["pred_xstart"]), R["chain_x0"][j])
            print(f"\n[ddim_reverse_sample t={t}, conv_x3={x3}] sample {es:.2e}, pred_xstart {e0:.2e}")
            tol(f"invert_step{t}_sample_x3={x3}_maxabs", es, II.STEP_SAMPLE_GATE[t])
            tol(f"invert_step{t}_x0_x3={x3}_maxabs", e0, II.STEP_X0_GATE[t])
    finally:
        synth.rt.set_option("conv_x3", 1)


def test_p_mean_variance_golden(synth, S, R, kw):
    """the four tensors of p_mean_variance at t = 9 and t = 0 on sampler_chains' p_x_before_*; x is left alone"""
    d = _diffuser()
    for t in II.PMV_STEPS:
        x = dev(S[f"p_x_before_{t}"])
        r = d.p_mean_variance(synth.diffusion, x, tt(t), model_kwargs=kw)
        assert sorted(r) == sorted(II.PMV_KEYS) and np.array_equal(host(x), S[f"p_x_before_{t}"])
        for k in II.PMV_KEYS:
            e = maxabs(II.sub(r[k], II.PMV_CH_STRIDE), R[f"pmv_{t}_{k}"])
            print(f"\n[p_mean_variance t={t}] {k} {e:.2e}")
            tol(f"pmv_t{t}_{k}_maxabs", e, II.PMV_GATE[(t, k)])
        assert maxabs(host(r["variance"]), np.exp(host(r["log_variance"]).astype(np.float64))) < 1e-6          # variance <= 1: expf's few ulp


@pytest.mark.parametrize("name", ["ddim0", "ddim05", "p"])
def test_p_sample_and_ddim_sample_reproduce_the_stored_steps(synth, S, kw, name):
    """SpacedDiffusion.p_sample / ddim_sample at steps 9, 8, 0 of sampler_chains.npz (device Philox noise where the step draws any),
    within test_sampler_steps_teacher_forced_golden's gates"""
    d = _diffuser(sampler="p" if name == "p" else "ddim")
    seed, sid = int(S["seed"]), [int(S["sample_id"])]
    for i in (9, 8, 0):
        x = dev(S[f"{name}_x_before_{i}"])
        if name == "p":
            r = d.p_sample(synth.diffusion, x, tt(i), model_kwargs=kw, seed=seed, sample_ids=sid)
        else:
            r = d.ddim_sample(synth.diffusion, x, tt(i), model_kwargs=kw, eta=float(S[f"{name}_eta"]), seed=seed, sample_ids=sid)
        e0, e1 = maxabs(host(r["pred_xstart"]), S[f"{name}_x0_{i}"]), maxabs(host(r["sample"]), S[f"{name}_x_after_{i}"])
        print(f"\n[{name} step {i}] pred_xstart {e0:.2e}, sample {e1:.2e}")
        assert e0 < 5e-3 and e1 < (2e-4 if i == 0 else 2e-3), (i, e0, e1)    # test_sampler_steps_teacher_forced_golden's gates


@pytest.mark.parametrize("name", ["ddim05", "p"])
def test_progressive_generators_yield_the_single_step_chain(synth, S, kw, name):
    """N dicts; the last `sample` is the single-step entry iterated, bit for bit, and lies within the 10-step chain gate of
    test_gpu_sampler.py of the reference's final sample"""
    d = _diffuser(sampler="p" if name == "p" else "ddim")
    seed, sid = int(S["seed"]), [int(S["sample_id"])]
    x_T = dev(S[f"{name}_x_init"])
    if name == "p":
        gen = d.p_sample_loop_progressive(synth.diffusion, (1, 128, 48), noise=x_T, model_kwargs=kw, seed=seed, sample_ids=sid)
        step = lambda x, i: d.p_sample(synth.diffusion, x, tt(i), model_kwargs=kw, seed=seed, sample_ids=sid)  # noqa: E731
    else:
        gen = d.ddim_sample_loop_progressive(synth.diffusion, (1, 128, 48), noise=x_T, model_kwargs=kw, eta=0.5, seed=seed, sample_ids=sid)
        step = lambda x, i: d.ddim_sample(synth.diffusion, x, tt(i), model_kwargs=kw, eta=0.5, seed=seed, sample_ids=sid)  # noqa: E731
    outs = list(gen)
    assert len(outs) == N and all(sorted(o) == ["pred_xstart", "sample"] for o in outs)
    x = x_T
    for i in range(N - 1, -1, -1):
        x = step(x, i)["sample"]
    assert torch.equal(outs[-1]["sample"], x)
    e = maxabs(host(x), S[f"{name}_final"])
    tol(f"progressive_{name}_chain_maxabs", e, {"ddim05": 5e-4, "p": 3e-4}[name])


def test_invert_loop_equals_the_single_step_iterated(synth, S, kw, inverted):
    """ddim_reverse_sample_loop (one device call, the code-path table of all steps built up front) against ddim_reverse_sample called
    ten times (a one-step table each): bit for bit, trajectory and pred_xstart included - the table's launches choose no summation
    order by their width"""
    d = _diffuser()
    x = dev(S["ddim0_final"])
    for t in range(N):
        r = d.ddim_reverse_sample(synth.diffusion, x, tt(t), model_kwargs=kw)
        x = r["sample"]
        assert np.array_equal(host(x), inverted["trajectory"][t]), t
        assert np.array_equal(host(r["pred_xstart"]), inverted["pred_xstart"][t]), t
    assert np.array_equal(host(x), inverted["sample"]) and np.array_equal(inverted["sample"], inverted["trajectory"][-1])
    # a shorter inversion is the prefix of the longer one
    x5 = _diffuser().ddim_reverse_sample_loop(synth.diffusion, dev(S["ddim0_final"]), kw, depth=5)
    assert np.array_equal(host(x5), inverted["trajectory"][4])


def test_invert_loop_against_the_reference_chain(R, inverted):
    """the free-running inversion against the reference's chain at the compared depths (the trajectory), and its pred_xstart"""
    assert np.isfinite(inverted["trajectory"]).all()
    for depth in II.CHAIN_DEPTHS:
        e = maxabs(II.sub(inverted["trajectory"][depth - 1]), R["chain_x"][depth - 1])
        print(f"\n[inversion chain, depth {depth}] max-abs {e:.2e}")
        tol(f"invert_chain_depth{depth}_maxabs", e, II.CHAIN_GATE[depth])
    for depth in range(1, N + 1):                                           # printed only: the deeper levels are too sensitive to gate
        print(f"[inversion chain, depth {depth}] max-abs {maxabs(II.sub(inverted['trajectory'][depth - 1]), R['chain_x'][depth - 1]):.2e}")


# Split loop against whole loop.  The whole loop evaluates its code-path table J = 36 // (B + Nu) steps per launch from step n - 1 down
# (Nu: distinct lengths), and the split-K of those launches follows their width ((B + Nu) x steps rows: 1 from 22 rows up).  dtts_diff_sample_from makes
# the whole loop's launches, so the SECOND half always reads the whole loop's bits.  The FIRST half is today's dtts_diff_sample_ex with
# n_steps, whose last launch is narrower than the whole loop's where n_steps is no multiple of J: its bits are the whole loop's when
# both launches take the same split.  The two batches below are such shapes for n = 10: three distinct lengths (J = 6; first half of 4
# steps: 24 rows against 36, no split in either) for s = 5, three equal lengths (J = 9; first half of 9 steps: the whole loop's first
# launch itself) for s = 0.
SPLIT_CASES = {5: [48, 20, 33], 0: [48, 48, 48]}


@pytest.mark.parametrize("s", [5, 0])
@pytest.mark.parametrize("name,eta", [("ddim", 0.0), ("ddim", 0.5), ("p", 0.0)])
def test_split_loop_equals_whole_loop(synth, name, eta, s):
    """today's loop with n_steps = n - 1 - s, then t_start = s from its result, against the uninterrupted loop from the same x_init: bit
    for bit (the Philox noise is keyed by the step index)"""
    rt = synth.rt
    d = _diffuser(sampler=name)
    lens = SPLIT_CASES[s]
    B, T = len(lens), max(lens)
    rs = np.random.RandomState(60 + s)
    ce, x_init = dev(rs.randn(B, 768, T) * 0.5), dev(rs.randn(B, 128, T))
    sids = [30 + b for b in range(B)]
    sched = rt.diff_schedule(d.timestep_map)
    sampler = 0 if name == "p" else 1
    whole = rt.diff_sample_ex(ce, 81, sids, sched=sched, sampler=sampler, eta=eta, lens=lens, x_init=x_init, denorm=False)
    first = rt.diff_sample_ex(ce, 81, sids, sched=sched, sampler=sampler, eta=eta, lens=lens, x_init=x_init, n_steps=N - 1 - s, denorm=False)
    loop = d.p_sample_loop if name == "p" else d.ddim_sample_loop
    args = dict(model_kwargs={"precomputed_aligned_embeddings": ce}, seed=81, sample_ids=sids, lens=lens)
    if name != "p":
        args["eta"] = eta
    second = loop(synth.diffusion, (B, 128, T), noise=first, t_start=s, **args)
    assert bool(torch.isfinite(whole).all()) and not torch.equal(first, whole)
    assert torch.equal(second, whole), maxabs(host(second), host(whole))
    if s == 5:
        # t_start = n - 1 is today's call
        assert torch.equal(loop(synth.diffusion, (B, 128, T), noise=x_init, t_start=N - 1, **args), whole)
        assert torch.equal(loop(synth.diffusion, (B, 128, T), noise=x_init, **args), whole)


def test_t_start_from_the_reference_level_5(synth, S, R, kw):
    """ddim_sample_loop(t_start=5) from the reference's OWN x at the level of step 5 of its 10-step chain against its final sample"""
    x = _diffuser().ddim_sample_loop(synth.diffusion, (1, 128, 48), noise=dev(R["split_x5"]), model_kwargs=kw, t_start=II.SPLIT_LEVEL,
                                     seed=int(S["seed"]), sample_ids=[int(S["sample_id"])])
    e = maxabs(host(x), S["ddim0_final"])
    print(f"\n[t_start=5 from the reference's level 5] max-abs {e:.2e}")
    tol("t_start5_from_reference_level_maxabs", e, II.SPLIT_GATE)


def test_ragged_inversion_rows_equal_alone(synth):
    """lens = [48, 20, 33]: each row of the inversion against the row run alone (the batch's launches differ from a single row's in
    tiles and split-K, so within test_ragged_batch8_ddim_eta_rows_equal_alone's gate); columns at or beyond lens stay what x_start
    holds there, as ddim_sample_loop leaves its x_init's"""
    d = _diffuser()
    lens = [48, 20, 33]
    B, T, depth = len(lens), max(lens), 5
    rs = np.random.RandomState(71)
    ce = (rs.randn(B, 768, T) * 0.5).astype(np.float32)
    xs = np.clip(rs.randn(B, 128, T) * 0.5, -1, 1).astype(np.float32)
    xb = host(d.ddim_reverse_sample_loop(synth.diffusion, dev(xs), {"precomputed_aligned_embeddings": dev(ce)}, depth=depth, lens=lens))
    for b, L in enumerate(lens):
        alone = host(d.ddim_reverse_sample_loop(synth.diffusion, dev(xs[b:b + 1, :, :L]),
                                                {"precomputed_aligned_embeddings": dev(ce[b:b + 1, :, :L])}, depth=depth))
        assert np.isfinite(alone).all()
        e = maxabs(xb[b, :, :L], alone[0])
        print(f"\n[ragged inversion, row {b}] batch vs alone: max-abs {e:.2e}")
        tol(f"invert_ragged_row{b}_vs_alone_maxabs", e, II.RAGGED_ROW_GATE)
        assert np.array_equal(xb[b, :, L:], xs[b, :, L:])
        assert maxabs(xb[b, :, :L], xs[b, :, :L]) > 1e-2


def _request():
    rs = np.random.RandomState(90)
    refer = torch.from_numpy((rs.randn(1, 128, 40) * 2 - 5).astype(np.float32))
    text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (1, 6)), np.zeros((1, 1), np.int64)], 1).astype(np.int32))
    return dict(text=text, text_length=torch.tensor([7]), refer=refer, refer_lengths=torch.tensor([40]))


def test_invert_mel_and_resynthesize_equal_their_pieces(synth, S):
    """invert_mel / resynthesize against the same pieces called by hand, bit for bit; another prompt changes the mel; T % 4 != 0 is
    refused"""
    from detail_tts_amd.vqvae.model_24k import denormalize_torch_mel, normalize_torch_mel
    q = _request()
    mel = denormalize_torch_mel(dev(S["ddim0_final"]))                      # a raw log-mel [1,128,48]
    inv = synth.invert_mel(mel, [48], q["text"], q["text_length"], q["refer"], q["refer_lengths"], diffusion_steps=N, depth=5)
    assert inv["depth"] == 5 and inv["diffusion_steps"] == N and tuple(inv["x"].shape) == (1, 128, 48) and tuple(inv["codes"].shape) == (1, 12)
    # by hand
    d = _diffuser()
    codes, _ = synth.encode(mel, [48])
    refer = q["refer"].cuda()
    lat = synth.gpt(refer, q["refer_lengths"], q["text"], q["text_length"], codes, torch.tensor([12 * 1024]), return_latent=True, clip_inputs=False)
    emb = synth.diffusion.timestep_independent(lat, synth.diffusion.get_conditioning(refer), 48)
    assert torch.equal(codes, inv["codes"]) and torch.equal(emb, inv["emb"])
    x = d.ddim_reverse_sample_loop(synth.diffusion, normalize_torch_mel(mel), {"precomputed_aligned_embeddings": emb}, depth=5)
    assert torch.equal(x, inv["x"])
    out = synth.resynthesize(inv, q["text"], q["text_length"], vocode=False)
    hand = denormalize_torch_mel(d.ddim_sample_loop(synth.diffusion, (1, 128, 48), noise=x, model_kwargs={"precomputed_aligned_embeddings": emb},
                                                    t_start=5))
    assert torch.equal(out, hand) and bool(torch.isfinite(out).all())
    wav, mel2 = synth.resynthesize(inv, q["text"], q["text_length"])
    assert torch.equal(mel2, out) and tuple(wav.shape) == (1, 1, 12 * 1024) and bool(torch.isfinite(wav).all())
    # another prompt: the code embedding is rebuilt from the stored codes under it
    other = (np.random.RandomState(91).randn(1, 128, 52) * 2 - 5).astype(np.float32)
    out2 = synth.resynthesize(inv, q["text"], q["text_length"], refer=torch.from_numpy(other), refer_lengths=torch.tensor([52]), vocode=False)
    assert maxabs(host(out2), host(out)) > 1e-2
    # depth = all steps: pure eps', a whole loop with noise = x
    full = synth.invert_mel(mel, [48], q["text"], q["text_length"], q["refer"], q["refer_lengths"], diffusion_steps=N)
    assert full["depth"] == N
    whole = denormalize_torch_mel(d.ddim_sample_loop(synth.diffusion, (1, 128, 48), noise=full["x"],
                                                     model_kwargs={"precomputed_aligned_embeddings": emb}))
    assert torch.equal(synth.resynthesize(full, q["text"], q["text_length"], vocode=False), whole)
    with pytest.raises(ValueError):
        synth.invert_mel(mel[:, :, :46], [46], q["text"], q["text_length"], q["refer"], q["refer_lengths"], diffusion_steps=N)


def test_round_trip_from_depth_5_equals_the_reference_round_trip(synth, S, R, kw, inverted):
    """inversion to depth 5, then resynthesize (ddim, eta = 0, t = 5 .. 0) under the fixture's code embedding: the reference's stored
    round trip - and NOT the input (guidance and the clamp are not invertible: the reference misses x_start by rt_miss = 0.88)"""
    from detail_tts_amd.vqvae.model_24k import normalize_torch_mel
    inv = dict(x=dev(inverted["trajectory"][II.ROUND_TRIP_DEPTH - 1]), depth=II.ROUND_TRIP_DEPTH, diffusion_steps=N, codes=None,
               emb=kw["precomputed_aligned_embeddings"])
    mel = synth.resynthesize(inv, None, None, vocode=False)
    e = maxabs(II.sub(mel), (R["rt_final"].astype(np.float64) + 1) / 2 * (2.7 + 11.512925465) - 11.512925465)
    print(f"\n[round trip from depth 5] de-normalised mel max-abs {e:.2e}")
    tol("round_trip_depth5_denorm_maxabs", e, II.ROUND_TRIP_GATE * II.DENORM_SCALE)
    miss = maxabs(host(normalize_torch_mel(mel)), S["ddim0_final"])
    assert miss > 0.5 * float(R["rt_miss"]) > 0.1, miss
