"""GPU: text-to-audio alignment through every layer - UnifiedVoice.attentions / text_alignment against the REFERENCE's own
get_logits(get_attns=True) in float64 (tests/golden/make_golden_attentions.py -> gpt_attentions.npz), SynthesizerTrn.align and
infer(return_alignment=True), ragged batches, the latents-in forms and the refusals.

The model runs the PEAKED weights of tests/align_inputs.py (the q and k columns of every c_attn times the factor the fixture stores):
under the plain seed-0 weights the maps are almost flat and a wrong scale or a shifted key would pass.  The gates are 20 x the largest
errors measured on the MI355X (profiles/align_measured_errors.txt) and are asserted to be at most a tenth of `mut_min`, the smallest
deviation the fixture script found under a key shifted by one, a query taken one column later, a window-only denominator and reversed
heads.  The stored paths are stable under noise of that size (the fixture script asserts it), so a device within the gates has to
find the reference's path; the path is also held to the NumPy DP on the device's own attn.

What pins the path step: under the UNIFORM weights the mean over 160 random-weight heads is nearly flat, the start-text column is a
faint sink and the reference's path is column 0 throughout (no factor or seed gives a uniform path that both moves and survives the
noise; make_golden_attentions.py) - that comparison sees little.  The WEIGHTED cases put 0.9 of the weight on two heads
(align_inputs.head_weights); their paths move (case A: 3 columns per row, ending at 6 and 10 of 15; case B: 11 columns, ending at the
last, 128 of 129), and the fixture script and test_the_weighted_paths_move assert that they do.  The ragged, latents-in and infer tests
run under those weights as well, and hold every row's path to the NumPy DP over that row's own n x m."""
import functools

import numpy as np
import pytest

import align_inputs as AI
from conftest import load_golden, tol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# max |device - reference float64|, each about 20 x the largest figure measured on the MI355X (profiles/align_measured_errors.txt).  The
# reference's own float32 run is 1.1e-6 away from its float64 run on the per-head maps (make_golden_attentions.py prints it).
GATE = 3e-5          # per-head maps of layers 0 and 9: measured 1.49e-6 (ten layers of fp32 activations in front of the last softmax)
MEAN_GATE = 5.6e-6   # a layer's head mean: measured 2.8e-7
ATTN_GATE = 1e-6     # attn under the uniform weights, the mean over 160 heads: measured 4.1e-8
MASS_GATE = 8.4e-6   # text_mass, a row sum of up to 129 of them: measured 4.2e-7
ATTN_W_GATE = 1.2e-5 # attn under the concentrated weights, close to two heads' own maps (compare GATE): measured 5.7e-7
MASS_W_GATE = 1.1e-5 # ... and its row sums: measured 5.4e-7
ROWSUM_GATE = 3.5e-6 # |sum_s P - 1|: measured 1.7e-7


@pytest.fixture(scope="module")
def fx():
    return load_golden("gpt_attentions")


@pytest.fixture(scope="module")
def forced():
    return load_golden("gpt_forced")


@pytest.fixture(scope="module")
def model(fx):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    from detail_tts_amd.weights import select_inference_params, synthetic_state_dict
    state = AI.peaked_gpt_weights(synthetic_state_dict(0, optional=True), float(fx["factor"]))
    return SynthesizerTrn(select_inference_params(state), folded=True)


@functools.lru_cache(maxsize=None)
def cases():
    g = load_golden("gpt_forced")
    AI.SEED_B = int(load_golden("gpt_attentions")["b_seed"])
    return dict(a=AI.case_a(g), b=AI.case_b(g))


def args_of(case):
    """(refer cuda, cond_lengths, text [B, Lt], text_lengths, code rows) as the mirrors take them"""
    B = case["text"].shape[0]
    return (torch.from_numpy(case["refer"]).cuda(), [case["refer"].shape[2]] * B, case["text"], [case["text"].shape[1]] * B,
            [r for r in case["codes"]])


def test_the_gate_is_a_tenth_of_what_a_wrong_kernel_moves(fx):
    assert max(GATE, MEAN_GATE, ATTN_GATE, MASS_GATE, ATTN_W_GATE, MASS_W_GATE) <= float(fx["mut_min"]) / 10, (GATE, float(fx["mut_min"]))


def test_the_weighted_paths_move(fx):
    """a constant path satisfies a path comparison whatever n, m or scores the path step was given: every weighted path of the fixture
    visits at least 3 columns and ends in column m // 3 or later (case B: in the last column), so those comparisons see the arguments.
    The uniform paths ARE constant (column 0), and this is where that is written down."""
    for tag in "ab":
        m = fx[f"{tag}_attn_w"].shape[2]
        assert all(AI.path_moves(p, m) for p in fx[f"{tag}_path_w"]), tag
        assert (fx[f"{tag}_path"] == 0).all(), (tag, "the uniform path moves now: say so in the docstrings")
    assert int(fx["b_path_w"][0, -1]) == fx["b_attn_w"].shape[2] - 1, "case B's weighted path no longer ends in the last column"


def test_attentions_against_the_reference(model, fx):
    refer, cl, text, tl, codes = args_of(cases()["a"])
    maps = model.gpt.attentions(refer, cl, text, np.stack(codes), text_lengths=tl)
    assert len(maps) == 10 and all(tuple(m.shape) == (2, 16, 30, 30) for m in maps)
    got = np.stack([m.cpu().numpy() for m in maps]).astype(np.float64)
    tol("align_heads_layers_0_9_maxabs", np.abs(got[[0, 9]] - fx["a_heads"]).max(), GATE)
    tol("align_head_mean_all_layers_maxabs", np.abs(got.mean(axis=2) - fx["a_mean"]).max(), MEAN_GATE)
    tol("align_row_sums_maxabs", np.abs(got.sum(axis=4) - 1.0).max(), ROWSUM_GATE)
    assert (np.triu(got, 1) == 0).all(), "a key s > t is not exactly 0"
    two = model.gpt.attentions(refer, cl, text, np.stack(codes), text_lengths=tl, layers=[9, 0])
    assert len(two) == 2 and torch.equal(two[0], maps[9]) and torch.equal(two[1], maps[0]), "`layers` picks and orders the maps"


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
def test_text_alignment_against_the_reference(model, fx, tag, weighted):
    case = cases()[tag]
    refer, cl, text, tl, codes = args_of(case)
    sfx = "_w" if weighted else ""
    out = model.gpt.text_alignment(refer, cl, text, tl, codes, head_weights=fx["head_weights"] if weighted else None)
    attn, mass, path = out["attn"].cpu().numpy(), out["text_mass"].cpu().numpy(), out["path"].cpu().numpy()
    assert attn.shape == fx[f"{tag}_attn{sfx}"].shape and path.dtype == np.int32
    tol(f"align_{tag}{sfx}_attn_maxabs", np.abs(attn.astype(np.float64) - fx[f"{tag}_attn{sfx}"]).max(), ATTN_W_GATE if weighted else ATTN_GATE)
    tol(f"align_{tag}{sfx}_text_mass_maxabs", np.abs(mass.astype(np.float64) - fx[f"{tag}_text_mass{sfx}"]).max(),
        MASS_W_GATE if weighted else MASS_GATE)
    assert np.array_equal(path, fx[f"{tag}_path{sfx}"]), (tag, sfx, "the path differs from the reference's")
    scores = torch.log(out["attn"].clamp_min(1e-12)).cpu().numpy()
    for b in range(attn.shape[0]):
        assert np.array_equal(path[b], AI.monotone_path(scores[b])), (tag, sfx, b, "the path is not the NumPy DP of the device's own attn")
    again = model.gpt.text_alignment(refer, cl, text, tl, codes, head_weights=fx["head_weights"] if weighted else None)
    assert all(torch.equal(out[k], again[k]) for k in out), "two calls differ"


@pytest.fixture(scope="module")
def ragged(forced):
    """B = 3: texts of 13 / 5 / 9 ids, 12 / 20 / 3 codes, prompts of 64 / 40 / 64 frames"""
    a = AI.case_a(forced)
    rs = np.random.RandomState(3)
    texts = [a["text"][0], a["text"][1][:5], rs.randint(1, 255, 9)]
    codes = [a["codes"][0], rs.randint(0, 8192, 20), a["codes"][1][:3]]
    refer = torch.from_numpy(np.repeat(a["refer"][:1], 3, 0)).cuda()
    return refer, [64, 40, 64], texts, codes


def padded(texts):
    t = np.zeros((len(texts), max(len(x) for x in texts)), np.int64)
    for b, x in enumerate(texts):
        t[b, : len(x)] = x
    return t, [len(x) for x in texts]


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
def test_ragged_rows_equal_the_rows_alone(model, fx, ragged, weighted):
    refer, rl, texts, codes = ragged
    t, tl = padded(texts)
    hw = fx["head_weights"] if weighted else None
    out = model.gpt.text_alignment(refer, rl, t, tl, codes, head_weights=hw)
    scores = torch.log(out["attn"].clamp_min(1e-12)).cpu().numpy()
    paths = out["path"].cpu().numpy()
    if weighted:      # the comparisons below have something to see: the paths of the rows (12 x 15, 20 x 7, 3 x 11) are not all constant
        cols = [len(set(paths[b, : len(codes[b])].tolist())) for b in range(3)]
        print("distinct columns on the ragged rows' weighted paths:", cols)
        assert max(cols) >= 3, (cols, "every ragged path stays put: pick other rows")
    for b in range(3):
        n, m = len(codes[b]), len(texts[b]) + 2
        assert np.array_equal(paths[b, :n], AI.monotone_path(scores[b], n, m)), (b, "not the NumPy DP over the row's own n x m")
        alone = model.gpt.text_alignment(refer[b:b + 1, :, : rl[b]].contiguous(), [rl[b]], texts[b][None], [len(texts[b])], [codes[b]],
                                         head_weights=hw)
        assert tuple(alone["attn"].shape) == (1, n, m)
        assert torch.equal(out["attn"][b, :n, :m], alone["attn"][0]) and torch.equal(out["text_mass"][b, :n], alone["text_mass"][0]), b
        assert torch.equal(out["path"][b, :n], alone["path"][0]) and bool((out["path"][b, n:] == -1).all()), b
        assert bool((out["attn"][b, n:] == 0).all()) and bool((out["attn"][b, :, m:] == 0).all()), (b, "outside the row's window")


def test_cond_latents_and_speaker_forms_give_the_refer_form_bits(model, fx, ragged):
    refer, rl, texts, codes = ragged
    t, tl = padded(texts)
    hw = fx["head_weights"]           # the weights under which the paths move
    want = model.gpt.text_alignment(refer, rl, t, tl, codes, head_weights=hw)
    voice = model.get_conditioning_latents(refer, rl)
    got = model.gpt.text_alignment(None, None, t, tl, codes, cond_latents=voice.gpt, head_weights=hw)
    assert all(torch.equal(want[k], got[k]) for k in want)
    maps = model.gpt.attentions(refer, rl, t, codes, text_lengths=tl, layers=[4])
    maps_c = model.gpt.attentions(None, None, t, codes, text_lengths=tl, layers=[4], cond_latents=voice.gpt)
    assert torch.equal(maps[0], maps_c[0])
    a = model.align(t, tl, codes, refer=refer, refer_lengths=rl, head_weights=hw)
    s = model.align(t, tl, codes, speaker=voice, head_weights=hw)
    assert len(a) == 3
    for b in range(3):
        assert np.array_equal(a[b]["path"], want["path"][b, : len(codes[b])].cpu().numpy()) and np.array_equal(a[b]["path"], s[b]["path"])
        assert a[b]["stats"] == s[b]["stats"] and a[b]["token_times"] == s[b]["token_times"]
        assert len(a[b]["token_spans"]) == len(texts[b]) and 0.0 <= a[b]["stats"]["coverage"] <= 1.0
    # rows without any code: empty paths, and no pass is run
    e = model.align(t, tl, [np.zeros(0, np.int64)] * 3, refer=refer, refer_lengths=rl)
    assert [len(x["path"]) for x in e] == [0, 0, 0] and all(x["stats"]["coverage"] == 0.0 and x["stats"]["mean_text_mass"] is None for x in e)
    # a rectangle with code_lengths is the list form
    rect = np.zeros((3, 20), np.int64)
    for b, c in enumerate(codes):
        rect[b, : len(c)] = c
    r = model.align(t, tl, rect, [len(c) for c in codes], refer, rl, head_weights=hw)
    assert all(np.array_equal(r[b]["path"], a[b]["path"]) for b in range(3))


def test_infer_with_alignment_returns_the_plain_waveform_and_aligns_its_codes(model, fx, ragged):
    refer, rl, texts, _ = ragged
    hw = fx["head_weights"]           # the weights under which the paths move
    t, tl = padded(texts[:2])
    kw = dict(batch=True, seed=3, sample_ids=[21, 22], max_generate_length=10, suppress_eos=True, diffusion_steps=2, return_candidates=True)
    args = (torch.from_numpy(t), tl, refer[:2].cpu(), rl[:2])
    wav, cand = model.infer(*args, **kw)
    wav2, cand2, al = model.infer(*args, **kw, return_alignment=True, align_options=dict(head_weights=hw))
    assert torch.equal(wav.view(torch.int32), wav2.view(torch.int32)), "return_alignment changed the waveform"
    assert np.array_equal(cand["codes"], cand2["codes"]) and len(al) == 2
    codes = [cand["codes"][b, 0, : int(cand["ncodes"][b, 0]) - 1] for b in range(2)]
    direct = model.align(torch.from_numpy(t), tl, codes, refer=refer[:2], refer_lengths=rl[:2], head_weights=hw)
    print("distinct columns on infer's weighted paths:", [len(set(x["path"].tolist())) for x in al])
    assert any(len(set(x["path"].tolist())) > 1 for x in al), "both of infer's paths stay put: the comparison below sees nothing"
    for b in range(2):
        assert np.array_equal(al[b]["path"], direct[b]["path"]) and al[b]["stats"] == direct[b]["stats"]
        assert len(al[b]["path"]) == len(codes[b])
    # forced codes and a voice compose with it
    fk = dict(batch=True, seed=3, sample_ids=[21, 22], diffusion_steps=2, forced_codes=[np.arange(6) + 50, np.arange(9) + 7])
    voice = model.get_conditioning_latents(refer[:2], rl[:2])
    w0 = model.infer(torch.from_numpy(t), tl, None, None, speaker=voice, **fk)
    w1, al1 = model.infer(torch.from_numpy(t), tl, None, None, speaker=voice, **fk, return_alignment=True)
    assert torch.equal(w0.view(torch.int32), w1.view(torch.int32)) and [len(x["path"]) for x in al1] == [6, 9]
    # ... and so do an acoustic prompt and beams (both already run the teacher-forced pass on the generated codes alone)
    base = dict(batch=True, seed=3, sample_ids=[21, 22], max_generate_length=8, suppress_eos=True, diffusion_steps=2, return_lengths=True)
    for extra in (dict(prompt_codes=np.stack([np.arange(5) + 11, np.arange(5) + 400])), dict(decode_options=dict(num_beams=2))):
        w0, lens0 = model.infer(*args, **base, **extra)
        w1, lens1, al1 = model.infer(*args, **base, **extra, return_alignment=True)
        assert torch.equal(w0.view(torch.int32), w1.view(torch.int32)) and lens0 == lens1, extra
        assert [1024 * len(x["path"]) for x in al1] == lens1, extra
    # infer_gpt takes it too
    g0 = model.infer_gpt(*args, batch=True, seed=3, sample_ids=[21, 22], forced_codes=fk["forced_codes"])
    g1, alg = model.infer_gpt(*args, batch=True, seed=3, sample_ids=[21, 22], forced_codes=fk["forced_codes"], return_alignment=True)
    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32))
    assert all(np.array_equal(x["path"], y["path"]) for x, y in zip(alg, model.align(torch.from_numpy(t), tl, fk["forced_codes"], refer=refer[:2], refer_lengths=rl[:2])))


def test_refusals_raise_before_any_launch(model, ragged):
    from conv_tile_probe import launches_of
    refer, rl, texts, codes = ragged
    t, tl = padded(texts)
    voice = model.get_conditioning_latents(refer, rl)
    big = [np.zeros(1500, np.int64)] * 3
    bad = [("head_weights shape", lambda: model.gpt.text_alignment(refer, rl, t, tl, codes, head_weights=np.ones((10, 15), np.float32)), "head_weights"),
           ("head_weights rows", lambda: model.gpt.text_alignment(refer, rl, t, tl, codes, layers=[1, 2], head_weights=np.ones((10, 16), np.float32)), "head_weights"),
           ("layer out of range", lambda: model.gpt.text_alignment(refer, rl, t, tl, codes, layers=[10]), "layers"),
           ("layer twice", lambda: model.gpt.attentions(refer, rl, t, codes, text_lengths=tl, layers=[3, 3]), "layers"),
           ("1 GiB cap", lambda: model.gpt.attentions(refer, rl, t, big, text_lengths=tl), "layers"),
           ("speaker and refer", lambda: model.align(t, tl, codes, refer=refer, refer_lengths=rl, speaker=voice), "speaker")]
    for name, call, says in bad:
        def attempt():
            with pytest.raises(ValueError) as e:
                call()
            return str(e.value)
        msg, ran = launches_of(model.rt, attempt, level=2)
        assert says in msg and ran == {}, (name, msg, ran)
    # the unit entry's head dim (tests/test_gpu_attn_probs.py has the rest of its refusals)
    from detail_tts_amd.runtime import DttsError
    with pytest.raises(DttsError, match="head dim 48"):
        model.rt.op_attn_probs(torch.zeros((1, 192, 8), device="cuda"), 1, 64, 0, 64, 0, 1.0, [8], [0], [8], [0], [8])
    # ... and the refusal that stays: the reference's forward(return_attentions=True) has no value to mirror
    with pytest.raises(NotImplementedError):
        model.gpt.forward(refer, rl, t, tl, np.zeros((3, 4), np.int64), [4096] * 3, return_attentions=True)
