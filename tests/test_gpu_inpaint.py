"""GPU: mel inpainting in the diffusion decoder - the blend kernel alone (dtts_op_inpaint_blend) bit for bit against the NumPy fp32
restatement (tests/inpaint_ref.py) and its Philox streams against oracle/philox.py; the loop (dtts_diff_inpaint through
SpacedDiffusion.p_sample_loop / ddim_sample_loop) against the plain loops and against the reference-driven chains of inpaint.npz
(tests/golden/make_golden_inpaint.py); SynthesizerTrn.inpaint_mel.  Gates: tests/inpaint_inputs.py; measurements:
profiles/inpaint_measured_errors.txt."""
import numpy as np
import pytest

import inpaint_inputs as PI
import inpaint_ref as IR
from conftest import tol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = PI.N_STEPS
T = PI.T


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def synth(weights):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(weights, folded=True)


@pytest.fixture(scope="module")
def S(golden):
    return golden("sampler_chains")


@pytest.fixture(scope="module")
def G(golden):
    return golden("inpaint")


def _diffuser(n=N, sampler="ddim"):
    from detail_tts_amd.vqvae.utils.diffusion import SpacedDiffusion, get_named_beta_schedule, space_timesteps
    return SpacedDiffusion(space_timesteps(4000, [n]), betas=get_named_beta_schedule("linear", 4000), conditioning_free=True,
                           conditioning_free_k=2.0, sampler=sampler)


@pytest.fixture(scope="module")
def kw(S):
    return {"precomputed_aligned_embeddings": dev(S["code_emb"])}


# ------------------------------------------------------------------------------------------------ a. the kernel alone
MASKS = {"all": lambda L: np.ones(L, bool), "none": lambda L: np.zeros(L, bool), "first": lambda L: np.arange(L) == 0,
         "last": lambda L: np.arange(L) == L - 1, "alternating": lambda L: np.arange(L) % 2 == 0}
SENTINEL = np.float32(-77.25)


def _blend_case(rt, C, lens, mask, i, renoise, nan_span=False, seed=5):
    """one launch on a ragged batch against the restatement row by row; frames beyond a row's length hold the sentinel -> device x"""
    d = _diffuser()
    B = len(lens)
    rs = np.random.RandomState(seed + 31 * C + 7 * i + sum(lens))
    u, known, zk, zr = (rs.randn(B, C, T).astype(np.float32) for _ in range(4))
    keep = np.zeros((B, T), bool)
    for b, L in enumerate(lens):
        keep[b, :L] = MASKS[mask](L)
        keep[b, L:] = rs.rand(T - L) < 0.5                                  # a mask beyond the length is not read
        u[b, :, L:] = SENTINEL
    if nan_span:
        known[np.broadcast_to(~keep[:, None, :], known.shape)] = np.nan
    k = IR.coefs(d, i)
    got = host(rt.op_inpaint_blend(dev(u), dev(known), torch.from_numpy(keep), k, lens=lens, step0=i == 0, renoise=renoise,
                                   known_noise=dev(zk), renoise_noise=dev(zr) if renoise else None))
    for b, L in enumerate(lens):
        want = IR.blend(u[b, :, :L], known[b, :, :L], keep[b, :L], k, step0=i == 0, renoise=renoise, zk=zk[b, :, :L], zr=zr[b, :, :L])
        assert np.array_equal(got[b, :, :L], want), (b, L, maxabs(got[b, :, :L], want))
        assert np.all(got[b, :, L:] == SENTINEL), (b, L)
    return got, (u, known, keep, zk, zr, k)


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("i,renoise", [(0, False), (4, False), (4, True), (9, True)])
def test_blend_equals_the_restatement_bit_for_bit(synth, mask, i, renoise):
    """step 0 (a pure copy) and steps above it, renoise on and off, every mask, lens 48 / 44 / 5 / 1 inside T = 48 (C = 128: more than
    one block per row and a grid-stride loop), frames beyond len untouched"""
    _blend_case(synth.rt, 128, [48, 44, 5, 1], mask, i, renoise)


@pytest.mark.parametrize("i,renoise", [(0, False), (4, True)])
def test_blend_ends_mid_philox_block(synth, i, renoise):
    """C = 3, len = 5: C len = 15 ends inside the fourth Philox block; len = 1, 2, 48 beside it"""
    for mask in MASKS:
        _blend_case(synth.rt, 3, [5, 1, 2, 48], mask, i, renoise)


def test_blend_padded_row_equals_compact_row(synth):
    """a row of length 44 inside T = 48 against the same row as a T = 44 tensor: the same bits"""
    rt = synth.rt
    got, (u, known, keep, zk, zr, k) = _blend_case(rt, 128, [44], "alternating", 4, True)
    c = lambda a: dev(a[:, :, :44])  # noqa: E731
    compact = host(rt.op_inpaint_blend(c(u), c(known), torch.from_numpy(keep[:, :44].copy()), k, renoise=True, known_noise=c(zk),
                                       renoise_noise=c(zr)))
    assert np.array_equal(compact, got[:, :, :44])


def test_blend_never_reads_known_in_the_span(synth):
    """NaN where keep is False leaves no NaN in the output: the blend is a select"""
    for i, renoise in ((0, False), (4, False), (4, True)):
        got, _ = _blend_case(synth.rt, 128, [48, 44, 5], "alternating", i, renoise, nan_span=True)
        assert np.isfinite(got).all()


def test_blend_philox_streams(synth):
    """with Philox keys: eps_known is stream 8 and eps_renoise stream 9 of oracle/philox.py at step field i + r N, indexed over the
    row's own [C, len]; the two streams and two repeats differ.  2e-5: test_gpu_diff_losses.py's gate for drawn normals."""
    from oracle import philox
    rt = synth.rt
    C, lens, seed, sids = 128, [48, 44, 5], 77, [3, 11, 4]
    B = len(lens)
    zero = torch.zeros((B, C, T), device="cuda")
    keep_all, keep_none = torch.ones((B, T), dtype=torch.bool), torch.zeros((B, T), dtype=torch.bool)
    one = (1.0, 1.0, 1.0, 1.0)
    draws = {}
    for r in (0, 1):
        step = 4 + r * N
        # known = 0, every frame kept: x = 1 * 0 + 1 * eps_known
        zk = host(rt.op_inpaint_blend(zero, zero, keep_all, one, lens=lens, seed=seed, sample_ids=sids, philox_step=step))
        # u = 0, nothing kept, renoise: x = 1 * 0 + 1 * eps_renoise
        zr = host(rt.op_inpaint_blend(zero, zero, keep_none, one, lens=lens, renoise=True, seed=seed, sample_ids=sids, philox_step=step))
        for stage, z in ((8, zk), (9, zr)):
            for b, L in enumerate(lens):
                want = philox.normal(seed, sids[b], stage, step, C * L).reshape(C, L)
                e = maxabs(z[b, :, :L], want)
                tol(f"inpaint_philox_stage{stage}_r{r}_row{b}_maxabs", e, 2e-5)
                assert np.all(z[b, :, L:] == 0.0)
            draws[(stage, r)] = z[0]
    keys = list(draws)
    for a in range(len(keys)):
        for b in range(a):
            assert maxabs(draws[keys[a]], draws[keys[b]]) > 1.0, (keys[a], keys[b])
    # both streams in one launch: kept frames carry (eps_known + eps_renoise), the others eps_renoise
    keep = torch.from_numpy(MASKS["alternating"](T)[None].repeat(B, 0))
    both = host(rt.op_inpaint_blend(zero, zero, keep, one, lens=lens, renoise=True, seed=seed, sample_ids=sids, philox_step=4))
    want = np.where(host(keep)[0][None, :], draws[(8, 0)] + draws[(9, 0)], draws[(9, 0)])
    assert np.array_equal(both[0], want)


# ------------------------------------------------------------------------------------------------ b. the loop
def _loop(d, name):
    return d.p_sample_loop if name == "p" else d.ddim_sample_loop


@pytest.mark.parametrize("name,eta", [("ddim", 0.0), ("ddim", 0.5), ("p", 0.0)])
def test_nothing_kept_is_the_plain_loop(synth, S, kw, name, eta):
    """keep all False, U = 1: ddim_sample_loop / p_sample_loop bit for bit - from the drawn x_T, from a given one, under t_start = 5,
    and with eta > 0 (repeat 0 of the sampler's noise is the plain loop's key)"""
    d = _diffuser(sampler=name)
    loop = _loop(d, name)
    args = dict(model_kwargs=kw, seed=int(S["seed"]), sample_ids=[int(S["sample_id"])])
    if name == "ddim":
        args["eta"] = eta
    known, none = dev(S["ddim0_final"]), torch.zeros((1, T), dtype=torch.bool)
    x_T = dev(S["ddim0_x_init"])
    for extra in (dict(), dict(noise=x_T), dict(noise=x_T, t_start=5)):
        plain = loop(synth.diffusion, (1, 128, T), **extra, **args)
        got = loop(synth.diffusion, (1, 128, T), known=known, keep=none, **extra, **args)
        assert bool(torch.isfinite(plain).all()) and torch.equal(got, plain), (extra.keys(), maxabs(host(got), host(plain)))


@pytest.mark.parametrize("sampler,eta", [(0, 0.0), (1, 0.5)])
def test_nothing_kept_from_a_drawn_x_T_is_diff_sample_ex(synth, sampler, eta):
    """the entries themselves on a ragged batch, lens (48, 20, 33): dtts_diff_inpaint with keep all False, U = 1, from the top with no
    x_init equals dtts_diff_sample_ex (no x_init, denorm off) bit for bit - both draw x_T, the short rows through the
    compact-then-scatter route, and run the same loop"""
    from detail_tts_amd.vqvae.utils.diffusion import space_timesteps
    rt = synth.rt
    lens, sids, seed = [48, 20, 33], [3, 11, 4], 7
    rs = np.random.RandomState(21)
    ce, known = dev(rs.randn(3, 768, T) * 0.5), dev(np.clip(rs.randn(3, 128, T) * 0.5, -1, 1))
    sched = rt.diff_schedule(sorted(space_timesteps(4000, [N])))
    plain = rt.diff_sample_ex(ce, seed, sids, sched=sched, sampler=sampler, eta=eta, lens=lens, x_init=None, denorm=False)
    got = rt.diff_inpaint(known, torch.zeros((3, T), dtype=torch.bool), ce, seed, sids, sched=sched, sampler=sampler, eta=eta, resample=1,
                          first_step=None, x_init=None, lens=lens)
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0.1
    assert torch.equal(got, plain), maxabs(host(got), host(plain))


@pytest.mark.parametrize("name,U", PI.CHAINS)
def test_mixed_mask_keeps_known_and_changes_the_span(synth, S, kw, name, U):
    """kept frames are known's bits, the span differs from the plain loop's and from known, two calls give the same bits, a NaN in the
    span of known is never read, and U = 2 differs from U = 1"""
    d = _diffuser(sampler=name)
    loop = _loop(d, name)
    args = dict(model_kwargs=kw, seed=int(S["seed"]), sample_ids=[int(S["sample_id"])])
    keep = PI.keep_mask()
    known = S["ddim0_final"].copy()
    known[:, :, PI.SPAN] = np.nan
    got = loop(synth.diffusion, (1, 128, T), known=dev(known), keep=torch.from_numpy(keep), resample=U, **args)
    again = loop(synth.diffusion, (1, 128, T), known=dev(known), keep=torch.from_numpy(keep[0]), resample=U, **args)      # keep [T]
    assert torch.equal(got, again)
    g = host(got)
    assert np.isfinite(g).all() and np.array_equal(g[:, :, keep[0]], S["ddim0_final"][:, :, keep[0]])
    plain = host(loop(synth.diffusion, (1, 128, T), **args))
    assert maxabs(g[:, :, PI.SPAN], plain[:, :, PI.SPAN]) > 1e-2 and maxabs(g[:, :, PI.SPAN], S["ddim0_final"][:, :, PI.SPAN]) > 1e-2
    if U == 2:
        one = host(loop(synth.diffusion, (1, 128, T), known=dev(known), keep=torch.from_numpy(keep), **args))
        assert maxabs(g[:, :, PI.SPAN], one[:, :, PI.SPAN]) > 1e-2


def test_ragged_batch_keeps_every_rows_frames(synth):
    """B = 2, lens (48, 40): runs, each row's kept frames inside its length are known's bits, frames beyond a length are untouched
    (zero: no x_init), and row 0 is the row alone within the ragged-row gate of test_gpu_invert.py"""
    import invert_inputs as II
    d = _diffuser()
    lens = [48, 40]
    rs = np.random.RandomState(12)
    ce = (rs.randn(2, 768, T) * 0.5).astype(np.float32)
    known = np.clip(rs.randn(2, 128, T) * 0.5, -1, 1).astype(np.float32)
    keep = np.ones((2, T), bool)
    keep[0, 16:32] = False
    keep[1, 8:20] = False
    args = dict(seed=3, resample=2)
    got = host(d.ddim_sample_loop(synth.diffusion, (2, 128, T), model_kwargs={"precomputed_aligned_embeddings": dev(ce)}, known=dev(known),
                                  keep=torch.from_numpy(keep), lens=lens, sample_ids=[5, 6], **args))
    assert np.isfinite(got).all()
    for b, L in enumerate(lens):
        kb = keep[b] & (np.arange(T) < L)
        assert np.array_equal(got[b][:, kb], known[b][:, kb]), b
        assert np.all(got[b, :, L:] == 0.0)
        assert maxabs(got[b][:, ~keep[b]], known[b][:, ~keep[b]]) > 1e-2
    alone = host(d.ddim_sample_loop(synth.diffusion, (1, 128, T), model_kwargs={"precomputed_aligned_embeddings": dev(ce[:1])},
                                    known=dev(known[:1]), keep=torch.from_numpy(keep[:1]), sample_ids=[5], **args))
    tol("inpaint_ragged_row0_vs_alone_maxabs", maxabs(got[0], alone[0]), II.RAGGED_ROW_GATE)


# ------------------------------------------------------------------------------------------------ c. parity with the reference's steps
@pytest.mark.parametrize("name,U", PI.CHAINS)
def test_chains_against_the_reference(synth, S, G, kw, name, U):
    """the loop under the fixture's three noise arrays against the chain the reference's own ddim_sample / p_mean_variance produced
    with the NumPy blend between its steps: x after the last repeat of steps 7 and 4 (the trajectory) and the final x.  The kept
    frames of the final x are known's bits."""
    c = PI.name(name, U)
    d = _diffuser(sampler=name)
    sn, kn, rn = (dev(a) for a in PI.noises(name, U))
    keep, known = PI.keep_mask(), dev(S["ddim0_final"])
    x, traj = _loop(d, name)(synth.diffusion, (1, 128, T), noise=dev(S["ddim0_x_init"]), model_kwargs=kw, known=known,
                             keep=torch.from_numpy(keep), resample=U, step_noise=sn, known_noise=kn, renoise=rn, return_trajectory=True)
    assert tuple(traj.shape) == (9 * U + 1, 1, 128, T) and torch.equal(traj[-1], x)
    assert np.array_equal(host(x)[:, :, keep[0]], S["ddim0_final"][:, :, keep[0]])
    last = {i: e for e, i, r, reps in IR.evaluations(N - 1, U) if r == reps - 1}
    worst = 0.0
    for i in PI.STORED_AFTER:
        e = maxabs(PI.sub(traj[last[i]]), G[f"{c}_x_after_{i}"])
        print(f"\n[inpaint chain {c}] x after step {i}: max-abs {e:.2e} (fixture's fp32-against-float64 gap {float(G['f64_gap_' + c]):.2e})")
        worst = max(worst, e)
    tol(f"inpaint_chain_{c}_maxabs", worst, PI.CHAIN_GATE[c])


# ------------------------------------------------------------------------------------------------ d. the model
def _request(B=1):
    rs = np.random.RandomState(90)
    refer = torch.from_numpy((rs.randn(B, 128, 40) * 2 - 5).astype(np.float32))
    text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, 6)), np.zeros((B, 1), np.int64)], 1).astype(np.int32))
    return dict(text=text, text_length=torch.tensor([7] * B), refer=refer, refer_lengths=torch.tensor([40] * B))


@pytest.fixture(scope="module")
def mel(S):
    from detail_tts_amd.vqvae.model_24k import denormalize_torch_mel
    return denormalize_torch_mel(dev(S["ddim0_final"]))                      # a raw log-mel [1,128,48]


def test_inpaint_mel_keeps_the_callers_bits(synth, mel):
    """kept frames of mel' are the input mel's bits with vocode=False and with a wav returned; the span is new and finite; spans= and
    the equivalent keep= agree; codes=None is codes=encode(mel); p and ddim, U = 2 and t_start run"""
    q = _request()
    a = (mel, [T], q["text"], q["text_length"], q["refer"], q["refer_lengths"])
    keep = torch.from_numpy(PI.keep_mask())
    kd = keep.cuda()[0]
    out = synth.inpaint_mel(*a, spans=[[PI.SPAN_CODES]], diffusion_steps=N, vocode=False)
    assert tuple(out.shape) == (1, 128, T) and bool(torch.isfinite(out).all())
    assert torch.equal(out[:, :, kd], mel[:, :, kd]) and maxabs(host(out[:, :, ~kd]), host(mel[:, :, ~kd])) > 1e-2
    assert torch.equal(synth.inpaint_mel(*a, keep=keep, diffusion_steps=N, vocode=False), out)
    codes, _ = synth.encode(mel, [T])
    assert torch.equal(synth.inpaint_mel(*a, keep=keep, codes=codes, diffusion_steps=N, vocode=False), out)
    wav, mel2 = synth.inpaint_mel(*a, keep=keep, diffusion_steps=N)
    assert torch.equal(mel2, out) and tuple(wav.shape) == (1, 1, 12 * 1024) and bool(torch.isfinite(wav).all())
    # other codes in the span change it, the kept frames stay
    other = codes.clone()
    other[:, 4:8] = (other[:, 4:8] + 17) % 1024
    out2 = synth.inpaint_mel(*a, keep=keep, codes=other, diffusion_steps=N, vocode=False)
    assert torch.equal(out2[:, :, kd], mel[:, :, kd]) and maxabs(host(out2), host(out)) > 1e-3
    for extra in (dict(sampler="p"), dict(resample=2), dict(t_start=5), dict(eta=0.5, seed=4, sample_ids=[9])):
        o = synth.inpaint_mel(*a, keep=keep, diffusion_steps=N, vocode=False, **extra)
        assert bool(torch.isfinite(o).all()) and torch.equal(o[:, :, kd], mel[:, :, kd]), extra
        assert maxabs(host(o[:, :, ~kd]), host(out[:, :, ~kd])) > 1e-3, extra
    # nothing kept with t_start=None: the plain loop under these codes
    from detail_tts_amd.vqvae.model_24k import denormalize_torch_mel
    none = synth.inpaint_mel(*a, keep=torch.zeros((1, T), dtype=torch.bool), diffusion_steps=N, vocode=False)
    emb = synth._code_embedding(codes, q["text"], q["text_length"], q["refer"], q["refer_lengths"])
    plain = _diffuser().ddim_sample_loop(synth.diffusion, (1, 128, T), model_kwargs={"precomputed_aligned_embeddings": emb})
    assert torch.equal(none, denormalize_torch_mel(plain))


def test_inpaint_mel_with_a_voice_and_alignment_spans(synth, mel):
    """speaker=voice gives the refer call's bits; spans taken from an align result are accepted"""
    q = _request()
    voice = synth.get_conditioning_latents(q["refer"], q["refer_lengths"])
    codes, _ = synth.encode(mel, [T])
    al = synth.align(q["text"], q["text_length"], codes, None, q["refer"], q["refer_lengths"])[0]
    owned = [s for s in al["spans"] if s is not None]               # per text column; token_spans and a word's span have the same form
    assert owned
    first, last = owned[0]
    from_align = synth.inpaint_mel(mel, [T], q["text"], q["text_length"], q["refer"], q["refer_lengths"], spans=[[owned[0]]],
                                   diffusion_steps=N, vocode=False)
    assert bool(torch.isfinite(from_align).all())
    assert torch.equal(from_align[:, :, :4 * first], mel[:, :, :4 * first]) and torch.equal(from_align[:, :, 4 * last + 4:], mel[:, :, 4 * last + 4:])
    if any(s is None for s in al["spans"]):                         # the whole list with its None entries (columns without a code)
        whole = synth.inpaint_mel(mel, [T], q["text"], q["text_length"], q["refer"], q["refer_lengths"], spans=[al["spans"]],
                                  diffusion_steps=N, vocode=False)
        assert bool(torch.isfinite(whole).all())
    spans = [[PI.SPAN_CODES]]
    want = synth.inpaint_mel(mel, [T], q["text"], q["text_length"], q["refer"], q["refer_lengths"], spans=spans, diffusion_steps=N, vocode=False)
    got = synth.inpaint_mel(mel, [T], q["text"], q["text_length"], spans=spans, diffusion_steps=N, vocode=False, speaker=voice)
    assert torch.equal(got, want)
    first, last = spans[0][0]
    assert torch.equal(got[:, :, :4 * first], mel[:, :, :4 * first]) and torch.equal(got[:, :, 4 * last + 4:], mel[:, :, 4 * last + 4:])
    with pytest.raises(ValueError):
        synth.inpaint_mel(mel, [T], q["text"], q["text_length"], q["refer"], q["refer_lengths"], spans=spans, speaker=voice)


def test_inpaint_mel_in_the_fp16_trunk_mode(synth, mel):
    """the fp16 trunk mode runs and keeps the kept frames exact"""
    q = _request()
    keep = torch.from_numpy(PI.keep_mask())
    kd = keep.cuda()[0]
    synth.rt.set_option("trunk_fp16", 1)
    try:
        out = synth.inpaint_mel(mel, [T], q["text"], q["text_length"], q["refer"], q["refer_lengths"], keep=keep, diffusion_steps=N,
                                resample=2, vocode=False)
    finally:
        synth.rt.set_option("trunk_fp16", 0)
    fp32 = synth.inpaint_mel(mel, [T], q["text"], q["text_length"], q["refer"], q["refer_lengths"], keep=keep, diffusion_steps=N,
                             resample=2, vocode=False)
    assert bool(torch.isfinite(out).all()) and torch.equal(out[:, :, kd], mel[:, :, kd])
    assert not torch.equal(out, fp32)
