"""GPU parity: UnifiedVoice.inference_speech_valle (reference gpt/model.py:546-579) - a decode session whose prefill covers
[cond | text | 1, 8192, prompt] - against the codes and per-step hidden states the REFERENCE produced under the Philox
multinomial (tests/golden/make_golden_valle.py -> gpt_valle.npz), and against the session's own other routes."""
import numpy as np
import pytest

from conftest import tol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

G = 8
# decode-time latents vs the reference's final_norm output of every step: 20 x the largest error of the first MI355X run of these
# cases (profiles/valle_measured_errors.txt: 7.0e-6 max |diff| on values of magnitude ~3)
HIDDEN_GATE = 1.4e-4
# a row in a ragged batch vs that row alone: the gate test_gpu_gpt.py's batch tests put on a row's latents
ALONE_GATE = 2e-4
KW = dict(top_p=0.8, temperature=0.8, length_penalty=1.0, repetition_penalty=2.0, max_generate_length=G)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def rt(weights):
    from detail_tts_amd.runtime import Runtime
    return Runtime(weights, folded=True, parts=("gpt",))


@pytest.fixture(scope="module")
def uv(rt):
    from detail_tts_amd.config import load_config
    from detail_tts_amd.gpt.model import UnifiedVoice
    return UnifiedVoice(rt, load_config()["gpt"])


@pytest.fixture(scope="module")
def gv(golden):
    return golden("gpt_valle")


# name -> (rows of refer2 / text2, prompt key, extra keywords)
CASES = {
    "m0": (1, "prompt_m0", dict(do_sample=True, num_return_sequences=1, **KW)),
    "m1": (1, "prompt_m1", dict(do_sample=True, num_return_sequences=1, **KW)),
    "typical": (1, "prompt_m17", dict(do_sample=True, num_return_sequences=1, typical_sampling=True, typical_mass=0.9, **KW)),
    "batch2": (2, "prompt_m5", dict(do_sample=True, num_return_sequences=1, **KW)),
    "greedy": (1, "prompt_m5", dict(do_sample=False, num_return_sequences=1, length_penalty=1.0, repetition_penalty=2.0, max_generate_length=G)),
    "nrs2": (1, "prompt_m5", dict(do_sample=True, num_return_sequences=2, **KW)),
    "input_tokens": (1, "prompt_m5", dict(do_sample=True, num_return_sequences=1, **KW)),
    "long": (1, "prompt_m130", dict(do_sample=True, num_return_sequences=1, **KW)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_codes_and_hidden_states_equal_the_reference(uv, gv, name):
    """Token for token the reference's codes; the decode-time latents against the reference's hidden state of every step.  `long` is
    m = 130: Lp = 141 prefix columns (more than the 128 queries of a prefill attention block and than two of its 64-key tiles,
    csrc/attention.hip) and Lp + G = 149 takes the KV capacity from 128 to 256 columns.  `batch2`'s row 1 has a 3-id text: the reference
    has no text mask, so its batch is a rectangle and the zeros behind the shorter text are ids like any other (a ragged lp is
    test_ragged_rows_equal_each_row_alone's)."""
    rows, pkey, kw = CASES[name]
    assert int(gv["m_long"]) == 130 and int(gv["G"]) == G
    sid = int(gv[f"{name}_sample_id"])
    if name == "input_tokens":
        kw = dict(kw, input_tokens=gv["input_tokens"])
    out = uv.inference_speech_valle(torch.from_numpy(gv["refer2"][:rows]).cuda(), None, gv["text2"][:rows], gv[pkey][:rows],
                                    seed=int(gv["seed"]), sample_ids=[sid + b for b in range(rows)], **kw)
    ref = gv[f"{name}_codes"]
    assert np.array_equal(out.cpu().numpy(), ref), (name, out, ref)
    hid = gv[f"{name}_hidden"]                                # [steps, rows, C]: the state token k0 + i is drawn from
    lat = uv.last_latents.cpu().numpy()                       # [rows, C, G]
    k0 = gv["input_tokens"].shape[1] if name == "input_tokens" else 0
    assert hid.shape[0] == G - k0 and hid.shape[1] == lat.shape[0]
    err = max(float(np.abs(lat[:, :, k0 + i] - hid[i]).max()) for i in range(hid.shape[0]))
    print(f"valle_{name}_hidden_maxabs {err:.3e}")
    tol(f"valle_{name}_hidden_maxabs", err, HIDDEN_GATE)
    assert float(np.abs(hid).max()) > 0.5


def test_ragged_rows_equal_each_row_alone(rt, gv):
    """Per-row prompt lengths (an extension: the reference takes a rectangle) and per-row text lengths in one session: m = 3 with a
    5-id text next to m = 9 with a 3-id text, so n_p, lp and the position offsets all differ by row."""
    refer = dev(gv["refer2"])
    texts = [gv["text2"][0], gv["text2"][1][:4]]
    prompts = [gv["prompt_m17"][0][:3], gv["prompt_m17"][1][:9]]
    seed = int(gv["seed"])
    codes, ncodes, lat = rt.gpt_generate(refer, [40, 33], texts, seed, [21, 22], max_generate_length=G, prompt_codes=prompts)
    lat = lat.clone()
    for b in range(2):
        c1, n1, l1 = rt.gpt_generate(refer[b:b + 1].contiguous(), [[40, 33][b]], [texts[b]], seed, [21 + b], max_generate_length=G,
                                     prompt_codes=[prompts[b]])
        assert np.array_equal(codes[b], c1[0]) and ncodes[b] == n1[0], (b, codes[b], c1[0])
        tol(f"valle_ragged_row{b}_vs_alone_maxabs", float((lat[b] - l1[0]).abs().max()), ALONE_GATE)
    assert ncodes.min() > 0


def test_prefill_route_equals_the_forced_step_route(rt, gv):
    """The prompt in the parallel prefill == the same tokens fed through the decode loop one forced step each.  The step route is a
    tortoise session ([8192] at mel position 0, no fill id, no closing stop token), so the prefill route runs with the handle's test
    option gpt_prompt_raw (mel stream [8192, c_1 .. c_m]); both draw from the same forced uniforms.  Pins that the two routes agree
    on mel positions, KV cache columns and the repetition-penalty history."""
    m = 5
    refer, text, prompt = dev(gv["refer2"][:1]), gv["text2"][0], gv["prompt_m5"][0]
    u = np.random.RandomState(3).rand(1, G).astype(np.float32)
    u_steps = np.concatenate([np.zeros((1, m), np.float32), u], 1)
    steps, _, lat_s = rt.gpt_generate(refer, None, [text], 1, [0], max_generate_length=m + G, forced_codes=[prompt], forced_fill=-1,
                                      forced_uniforms=dev(u_steps), suppress_eos=True)
    lat_s = lat_s.clone()
    assert np.array_equal(steps[0, :m], prompt)
    rt.set_option("gpt_prompt_raw", 1)
    try:
        pre, _, lat_p = rt.gpt_generate(refer, None, [text], 1, [0], max_generate_length=G, forced_uniforms=dev(u), suppress_eos=True,
                                        prompt_codes=[prompt])
    finally:
        rt.set_option("gpt_prompt_raw", 0)
    assert np.array_equal(pre[0], steps[0, m:]), (pre, steps)
    tol("valle_prefill_vs_steps_latents_maxabs", float((lat_p[0] - lat_s[0, :, m:]).abs().max()), ALONE_GATE)


def test_kernel_paths_agree_on_a_prompted_session(rt, gv):
    """A prompted 5-row session on the persistent token kernel with 128 and 64 workgroups (bit-identical codes AND latents, as
    test_gpu_gpt.py demands of unprompted sessions) and on the launch-per-GEMV chain (same codes, latents to summation-order noise)."""
    rs = np.random.RandomState(11)
    B = 5
    refer = (rs.randn(B, 128, 48) * 2 - 5).astype(np.float32)
    rl = [48 - 3 * b for b in range(B)]
    texts = [np.concatenate([rs.randint(3, 255, 3 + b), [0]]).astype(np.int32) for b in range(B)]
    prompts = [rs.randint(0, 8192, 2 + 3 * b) for b in range(B)]
    args = (dev(refer), rl, texts, 77, list(range(30, 30 + B)))
    kw = dict(max_generate_length=G, prompt_codes=prompts)
    c128, n128, l128 = rt.gpt_generate(*args, **kw)
    l128 = l128.clone()
    c64, n64, l64 = rt.gpt_generate(*args, token_wgs=64, **kw)
    assert np.array_equal(c128, c64) and np.array_equal(n128, n64)
    assert torch.equal(l128, l64)
    rt.set_option("gpt_token_kernel", 0)
    try:
        cc, nc, lc = rt.gpt_generate(*args, **kw)
    finally:
        rt.set_option("gpt_token_kernel", 1)
    assert np.array_equal(c128, cc) and np.array_equal(n128, nc)
    assert float((l128 - lc).abs().max()) < 2e-4


def test_only_a_generated_stop_token_finishes_a_prompted_row(rt, gv):
    """A prompted row is not finished after its prefill - the reference's prompt stream [1, 8192, codes] holds no stop token, and prompt
    codes are refused outside [0, 8192) - so the row generates (the fixture's codes are there), and only a GENERATED 8193 - forced at
    step 3 here - finishes it: 4 tokens, padded with 8193."""
    refer, text, prompt = dev(gv["refer2"][:1]), gv["text2"][0], gv["prompt_m1"][0]
    sid, seed, ref = int(gv["m1_sample_id"]), int(gv["seed"]), gv["m1_codes"][0]
    assert 8193 not in ref[:3].tolist()
    samp = dict(top_k=50, top_p=0.8, temperature=0.8, repetition_penalty=2.0)
    codes, ncodes, _ = rt.gpt_generate(refer, None, [text], seed, [sid], max_generate_length=G, prompt_codes=[prompt], **samp)
    assert ncodes[0] > 0 and np.array_equal(codes[0, : len(ref)], ref)
    codes, ncodes, _ = rt.gpt_generate(refer, None, [text], seed, [sid], max_generate_length=G, prompt_codes=[prompt],
                                       forced_codes=[np.array([-1, -1, -1, 8193])], forced_fill=-1, **samp)
    assert ncodes[0] == 4 and codes[0, :3].tolist() == ref[:3].tolist() and codes[0, 3:].tolist() == [8193] * (G - 3)


def test_library_refuses_bad_prompts(rt, gv):
    """the C entry's own refusals (the Python layer refuses most of these earlier: tests/test_host_valle.py), each naming the field"""
    import ctypes as C
    from detail_tts_amd import _lib
    from detail_tts_amd.runtime import DttsError
    refer = dev(gv["refer2"][:1])
    text = np.ascontiguousarray(gv["text2"][:1], np.int32)
    tl, rl, sid = np.array([text.shape[1]], np.int32), np.array([40], np.int32), np.array([0], np.int32)
    lat = torch.zeros((1, 768, G), device="cuda")
    codes, ncodes = np.zeros((1, G), np.int32), np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(_lib.c_int_p)

    def call(prompt, lens, stride, g=G):
        o = _lib.DttsGptOptions()
        rt.lib.dtts_gpt_options_init(C.byref(o))
        o.sample_ids, o.max_generate_length = p(sid), g
        if prompt is not None:
            o.prompt_codes = p(prompt)
        if lens is not None:
            o.prompt_lens = p(lens)
        o.prompt_stride = stride
        rt._rc(rt.lib.dtts_gpt_generate(rt.h, C.c_void_p(refer.data_ptr()), p(rl), 40, p(text), p(tl), text.shape[1], 1, C.byref(o),
                                        p(codes), p(ncodes), C.c_void_p(lat.data_ptr()), G, rt._stream()))

    three = np.array([[5, 6, 7]], np.int32)
    with pytest.raises(DttsError, match="prompt_lens"):
        call(None, np.array([3], np.int32), 3)                        # prompt_lens without prompt_codes
    with pytest.raises(DttsError, match="prompt_lens"):
        call(three, np.array([-1], np.int32), 3)                      # m < 0
    with pytest.raises(DttsError, match="prompt_codes"):
        call(np.array([[5, 8192, 7]], np.int32), np.array([3], np.int32), 3)      # a code outside the table
    long = np.zeros((1, 1593), np.int32)
    with pytest.raises(DttsError, match="prompt_lens"):
        call(long, np.array([1593], np.int32), 1593)                  # 1593 + 3 + 8 = 1604 > 1603 positions
    call(three, np.array([3], np.int32), 3)                           # ... and a good one runs
    assert ncodes[0] > 0


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model(weights):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(weights, folded=True)


def rms(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(d * d)))


def test_infer_with_prompt_codes_vs_the_reference_composition(model, gv):
    """SynthesizerTrn.infer(prompt_codes=...) vs the reference's infer with line 782 calling inference_speech_valle (the prompt is
    encode()'s codes of a 40-frame mel; the diffusion latents come from the teacher-forced pass on the generated codes alone), at the
    small e2e fixtures' size and gate; and infer without prompt_codes returns the same bits before and after."""
    text = torch.from_numpy(gv["e2e_text"])
    args = (text, torch.tensor([text.shape[1]]), torch.from_numpy(gv["e2e_refer"]), torch.tensor([gv["e2e_refer"].shape[2]]))
    kw = dict(seed=int(gv["seed"]), sample_ids=[int(gv["e2e_infer_sample_id"])], max_generate_length=G)
    before = model.infer(*args, **kw).clone()
    prompt, _ = model.encode(torch.from_numpy(gv["e2e_prompt_mel"]), [40])
    assert np.array_equal(prompt.cpu().numpy().reshape(1, -1), gv["e2e_prompt"])
    wav = model.infer(*args, prompt_codes=prompt.reshape(1, -1), **kw).cpu().numpy()
    assert wav.shape == gv["e2e_infer_wav"].shape
    tol("valle_e2e_infer_wav_rms", rms(wav, gv["e2e_infer_wav"]), 1e-7)
    assert float(np.sqrt(np.mean(np.square(gv["e2e_infer_wav"], dtype=np.float64)))) > 1e-5
    after = model.infer(*args, **kw)
    assert torch.equal(before, after)


def test_infer_gpt_with_prompt_codes_vs_the_reference_composition(model, gv):
    text = torch.from_numpy(gv["e2e_text"])
    wav = model.infer_gpt(text, torch.tensor([text.shape[1]]), torch.from_numpy(gv["e2e_refer"]), torch.tensor([gv["e2e_refer"].shape[2]]),
                          seed=int(gv["seed"]), sample_ids=[int(gv["e2e_gpt_sample_id"])], max_generate_length=G,
                          prompt_codes=gv["e2e_prompt"]).cpu().numpy()
    assert wav.shape == gv["e2e_gpt_wav"].shape
    tol("valle_e2e_infer_gpt_wav_rms", rms(wav, gv["e2e_gpt_wav"]), 1e-7)
