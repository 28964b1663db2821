"""Host side of UnifiedVoice.inference_speech_valle (acoustic-prompt decode): prompt id assembly, the refusals that come before any
library call, the dtts_gpt_options layout, and the fixture's own consistency.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from detail_tts_amd.gpt import prompt as P      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prompt_id_assembly():
    """gpt/model.py:552, 561-564 with :132-136: the mel stream is [1, 8192, codes] (no stop token: the reference keeps the inputs of
    build_aligned_inputs_and_targets), n_p = m + 2 positions, lp = 1 + (Lt + 2) + n_p prefix columns, the penalty history {1, 8192} +
    the codes, and the first generated token's input sits at mel position n_p."""
    rows = P.prompt_rows([np.array([], np.int64), np.array([7]), np.array([5, 5, 8191, 0])], 3)
    lay = P.prompt_layout(rows, [6, 6, 4], 8)
    assert [r.tolist() for r in lay["mel_ids"]] == [[1, 8192], [1, 8192, 7], [1, 8192, 5, 5, 8191, 0]]
    assert lay["n_p"] == [2, 3, 6] and lay["pos_off"] == lay["n_p"]
    assert lay["lp"] == [1 + 8 + 2, 1 + 8 + 3, 1 + 6 + 6]
    assert lay["seen"] == [[1, 8192], [1, 7, 8192], [0, 1, 5, 8191, 8192]]
    assert all(8193 not in s for s in lay["seen"])                  # the stop token is NOT in the penalty history
    # a rectangle (array or tensor) is B rows of one length
    assert [r.tolist() for r in P.prompt_rows(torch.tensor([[1, 2], [3, 4]]), 2)] == [[1, 2], [3, 4]]
    assert [len(r) for r in P.prompt_rows(np.zeros((2, 0), np.int64), 2)] == [0, 0]
    codes, lens = P.pack_prompt([np.array([9, 8]), np.array([], np.int64)], 2, [6, 6], 8)
    assert codes.dtype == np.int32 and codes.tolist() == [[9, 8], [0, 0]] and lens.tolist() == [2, 0]
    codes, lens = P.pack_prompt(np.zeros((1, 0), np.int64), 1, [6], 8)
    assert codes.shape == (1, 1) and lens.tolist() == [0]            # an empty prompt still hands the library a pointer


def test_position_table_limit_is_exact():
    """mel_pos_embedding has 1603 rows: m + 3 + G = 1603 fits, 1604 is refused (a session touches m + 2 + G rows; one is kept spare)"""
    G = 8
    P.prompt_layout(P.prompt_rows(np.zeros((1, 1603 - 3 - G), np.int64), 1), [6], G)
    with pytest.raises(ValueError, match="1604"):
        P.prompt_layout(P.prompt_rows(np.zeros((1, 1604 - 3 - G), np.int64), 1), [6], G)


def test_code_range_and_row_count():
    for bad in ([[0, 8192]], [[-1]], [[8193]]):
        with pytest.raises(ValueError, match="outside"):
            P.prompt_rows(np.array(bad), 1)
    with pytest.raises(ValueError, match="rows"):
        P.prompt_rows(np.zeros((2, 3), np.int64), 1)
    with pytest.raises(ValueError, match="shape"):
        P.prompt_rows(np.zeros((3,), np.int64), 1)


class _NoLibrary:
    """a Runtime whose library must never be touched"""
    def __init__(self):
        from detail_tts_amd.runtime import Runtime
        self._pad_text, self._prompt = Runtime._pad_text, Runtime._prompt

    @property
    def lib(self):
        raise AssertionError("library call before the prompt was checked")


@pytest.mark.parametrize("entry", ["gpt_generate", "gpt_prefill"])
def test_runtime_refuses_bad_prompts_before_any_library_call(entry):
    from detail_tts_amd.runtime import Runtime
    fn = getattr(Runtime, entry)
    refer = torch.zeros((1, 128, 8))
    args = (refer, None, [np.arange(6)], 0, [0])
    G = 8
    with pytest.raises(ValueError, match="1604"):
        fn(_NoLibrary(), *args, max_generate_length=G, prompt_codes=np.zeros((1, 1604 - 3 - G), np.int64))
    with pytest.raises(ValueError, match="outside"):
        fn(_NoLibrary(), *args, max_generate_length=G, prompt_codes=[np.array([5, 9000])])
    with pytest.raises(ValueError, match="rows"):
        fn(_NoLibrary(), *args, max_generate_length=G, prompt_codes=np.zeros((2, 3), np.int64))
    # at exactly the table's size the checks pass and the call goes on (to the tensor check, then to the library)
    with pytest.raises(Exception) as e:
        fn(_NoLibrary(), *args, max_generate_length=G, prompt_codes=np.zeros((1, 1603 - 3 - G), np.int64))
    assert not isinstance(e.value, ValueError)


class _NoDevice:
    """a model whose runtime must never be touched"""
    @property
    def rt(self):
        raise AssertionError("device work before the arguments were checked")


def test_infer_refuses_prompt_codes_with_forced_codes_or_candidates():
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    args = (torch.zeros((1, 4), dtype=torch.long), [4], torch.zeros((1, 128, 8)), [8])
    prompt = np.zeros((1, 3), np.int64)
    for fn in (SynthesizerTrn.infer, SynthesizerTrn.infer_gpt):
        with pytest.raises(ValueError, match="forced_codes"):
            fn(_NoDevice(), *args, prompt_codes=prompt, forced_codes=[np.arange(3)])
        with pytest.raises(ValueError, match="outside"):
            fn(_NoDevice(), *args, prompt_codes=np.full((1, 3), 8192))
    with pytest.raises(ValueError, match="num_candidates"):
        SynthesizerTrn.infer(_NoDevice(), *args, prompt_codes=prompt, num_candidates=2)


def test_unified_voice_has_the_reference_signature():
    import inspect
    from detail_tts_amd.gpt.model import UnifiedVoice
    names = list(inspect.signature(UnifiedVoice.inference_speech_valle).parameters)
    assert names[:10] == ["self", "speech_conditioning_latent", "cond_lengths", "text_inputs", "mel_codes", "input_tokens",
                          "num_return_sequences", "max_generate_length", "typical_sampling", "typical_mass"]
    for extra in ("text_lengths", "seed", "sample_ids", "suppress_eos", "forced_uniforms", "hf_generate_kwargs"):
        assert extra in names


def test_gpt_options_layout_carries_the_prompt_fields():
    """The three prompt fields sit behind token_wgs, in the header's order, and are NULL / 0 after dtts_gpt_options_init."""
    from detail_tts_amd import _lib
    names = [n for n, _ in _lib.DttsGptOptions._fields_]
    assert names[-4:] == ["token_wgs", "prompt_codes", "prompt_lens", "prompt_stride"]
    hdr = open(os.path.join(ROOT, "include", "detail_hip.h")).read()
    body = hdr[hdr.index("typedef struct dtts_gpt_options {"):hdr.index("} dtts_gpt_options;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    hdr_names = re.findall(r"(\w+)\s*(?:,|;)", body)          # every declarator: the word in front of a ',' or ';'
    assert hdr_names == names, (hdr_names, names)
    lib = _lib.load()
    o = _lib.DttsGptOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    lib.dtts_gpt_options_init(C.byref(o))
    assert o.struct_size == C.sizeof(_lib.DttsGptOptions)
    assert not o.prompt_codes and not o.prompt_lens and o.prompt_stride == 0
    assert _lib.DttsGptOptions.prompt_codes.offset > _lib.DttsGptOptions.token_wgs.offset


def test_fixture_is_self_consistent(golden):
    g = golden("gpt_valle")
    G = int(g["G"])
    rows = dict(m0=1, m1=1, typical=1, batch2=2, greedy=1, nrs2=2, input_tokens=1, long=1)
    m = dict(m0=0, m1=1, typical=17, batch2=5, greedy=5, nrs2=5, input_tokens=5, long=130)
    assert sorted(g["cases"].tolist()) == sorted(rows)
    for name, r in rows.items():
        codes, hid = g[f"{name}_codes"], g[f"{name}_hidden"]
        k = g["input_tokens"].shape[1] if name == "input_tokens" else 0
        assert codes.shape == (r, G), name
        assert hid.shape == (G - k, r, 768) and np.isfinite(hid).all(), name
        assert int(g[f"{name}_prompt_m"]) == m[name]
        assert bool(g[f"{name}_f64_agree"]), name                   # the float64 re-run of the reference returned the same codes
        assert codes.min() >= 0 and codes.max() <= 8193
    assert g["input_tokens_codes"][0, :2].tolist() == g["input_tokens"][0].tolist() == [11, 12]
    assert int(g["m_long"]) == 130 and g["prompt_m130"].shape == (2, 130)
    assert g["text2"].shape == (2, 6) and g["text2"][1, 3:].tolist() == [0, 0, 0]
    for k in ("prompt_m0", "prompt_m1", "prompt_m5", "prompt_m17", "prompt_m130", "e2e_prompt"):
        assert g[k].size == 0 or (g[k].min() >= 0 and g[k].max() < 8192)
    assert g["e2e_prompt"].shape == (1, 10) and g["e2e_prompt_mel"].shape == (1, 128, 40)
    for k in ("e2e_infer", "e2e_gpt"):
        n = g[f"{k}_codes"].shape[1] - 1                            # codes[:, :-1]
        assert g[f"{k}_wav"].shape == (1, 1, 1024 * n) and np.isfinite(g[f"{k}_wav"]).all()
