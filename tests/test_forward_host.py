"""Host side of UnifiedVoice.forward's loss mode (no GPU): the optional gpt.text_head tensors, their packing, the host preprocessing
(clip_inputs, set_mel_padding, aligned inputs and targets, gpt/model.py:453-470) and what tests/golden/gpt_forward.npz holds."""
import numpy as np
import pytest

HEAD = ("gpt.text_head.weight", "gpt.text_head.bias")


@pytest.fixture(scope="module")
def state_opt():
    from detail_tts_amd.weights import synthetic_state_dict
    return synthetic_state_dict(0, optional=True)


def test_optional_tensors_leave_every_other_tensor_bit_equal(weights, state_opt):
    """synthetic_state_dict(0, optional=True) = synthetic_state_dict(0) + the two head tensors: the same keys in the same order in front,
    the GPT's tensors bit-equal in state-dict form, and EVERY tensor bit-equal after folding (the session's `weights` is
    select_inference_params(synthetic_state_dict(0)))."""
    from detail_tts_amd.weights import inference_param_spec, optional_param_spec, select_inference_params, synthetic_state_dict
    assert tuple(optional_param_spec()) == HEAD
    assert not set(HEAD) & set(inference_param_spec())                 # test_weight_spec_counts pins that spec's total
    assert list(state_opt) == list(inference_param_spec()) + list(HEAD)
    assert state_opt[HEAD[0]].shape == (257, 768) and state_opt[HEAD[1]].shape == (257,)
    assert state_opt[HEAD[0]].dtype == np.float32 and float(np.abs(state_opt[HEAD[0]]).max()) > 0
    plain_gpt = synthetic_state_dict(0, only_prefixes=("gpt.",))
    assert set(plain_gpt) == {k for k in state_opt if k.startswith("gpt.")} - set(HEAD)
    for k, v in plain_gpt.items():
        assert np.array_equal(v, state_opt[k]), k
    sel = select_inference_params(state_opt)
    assert set(sel) == set(weights) | set(HEAD)
    for k, v in weights.items():
        assert np.array_equal(v, sel[k]), k
    # the head alone comes out the same too (its own Philox stream)
    alone = synthetic_state_dict(0, only_prefixes=("gpt.text_head.",), optional=True)
    assert list(alone) == list(HEAD) and all(np.array_equal(alone[k], state_opt[k]) for k in HEAD)
    assert not synthetic_state_dict(0, only_prefixes=("gpt.text_head.",))


def test_select_keeps_the_head_when_present_and_never_asks_for_it(weights, state_opt):
    from detail_tts_amd.weights import select_inference_params
    sel = select_inference_params(state_opt)
    assert all(np.array_equal(sel[k], state_opt[k]) for k in HEAD)
    no_head = {k: v for k, v in state_opt.items() if k not in HEAD}
    assert set(select_inference_params(no_head)) == set(weights)
    half = {k: v for k, v in state_opt.items() if k != HEAD[1]}        # a head without its bias is no head
    assert set(select_inference_params(half)) == set(weights)
    bad = dict(state_opt)
    bad[HEAD[0]] = np.zeros((256, 768), np.float32)
    with pytest.raises(ValueError, match="gpt.text_head.weight"):
        select_inference_params(bad)


def test_packed_head_has_coutp_384_and_a_zero_tail(weights, state_opt):
    from detail_tts_amd.packing import pack_all, packed_cout
    P = dict(weights)
    names_without = list(pack_all(P, parts=("gpt",)).entries)
    assert not [n for n in names_without if "text_head" in n]
    P.update({k: state_opt[k] for k in HEAD})
    pk = pack_all(P, parts=("gpt",)).entries
    assert [n for n in pk if n not in names_without] == ["gpt.text_head.wp", "gpt.text_head.bp"]
    wp, bp = pk["gpt.text_head.wp"], pk["gpt.text_head.bp"]
    assert packed_cout(257) == 384 and wp.shape == (1, 768, 384) and bp.shape == (384,)
    assert np.array_equal(wp[0, :, :257], state_opt[HEAD[0]].T) and np.array_equal(bp[:257], state_opt[HEAD[1]])
    assert not wp[:, :, 257:].any() and not bp[257:].any()
    assert 257 > 384 - 128                                              # launch_gpt_score's precondition: the V tail sits in the last chunk


def test_host_preprocessing_on_a_hand_written_example():
    from detail_tts_amd.gpt.model import forward_inputs
    from forward_targets import aligned_inputs_and_targets
    text = [[5, 6, 7, 8], [9, 10, 0, 0]]
    codes = [[1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11, 12]]
    tl, wl = [3, 2], [4 * 1024 + 5, 2 * 1024]
    src = np.array(codes)
    t, c = forward_inputs(text, tl, src, wl)
    assert np.array_equal(src, codes)                                   # the caller's codes are not padded in place
    assert t.dtype == np.int32 and c.dtype == np.int32
    assert t.tolist() == text                                           # text_lengths is not read without clip_inputs
    assert c.tolist() == [[1, 2, 3, 4, 5, 8193], [7, 8, 9, 8193, 8193, 8193]]
    ti, tt, mi, mt = aligned_inputs_and_targets(t, c)
    assert ti.tolist() == [[255, 5, 6, 7, 8, 0], [255, 9, 10, 0, 0, 0]]
    assert tt.tolist() == [[5, 6, 7, 8, 0, 0], [9, 10, 0, 0, 0, 0]]
    assert mi.tolist() == [[8192, 1, 2, 3, 4, 5, 8193, 8193], [8192, 7, 8, 9, 8193, 8193, 8193, 8193]]
    assert mt.tolist() == [[1, 2, 3, 4, 5, 8193, 8193, 8193], [7, 8, 9, 8193, 8193, 8193, 8193, 8193]]
    # clip_inputs: text to text_lengths.max() = 3 columns, codes to wav_lengths.max() // 1024 = 4, THEN set_mel_padding
    t2, c2 = forward_inputs(text, tl, codes, wl, clip_inputs=True)
    assert t2.tolist() == [[5, 6, 7], [9, 10, 0]]
    assert c2.tolist() == [[1, 2, 3, 4], [7, 8, 9, 8193]]
    ti2, tt2, mi2, mt2 = aligned_inputs_and_targets(t2, c2)
    assert ti2.tolist() == [[255, 5, 6, 7, 0], [255, 9, 10, 0, 0]] and tt2.tolist() == [[5, 6, 7, 0, 0], [9, 10, 0, 0, 0]]
    assert mi2.tolist() == [[8192, 1, 2, 3, 4, 8193], [8192, 7, 8, 9, 8193, 8193]]
    assert mt2.tolist() == [[1, 2, 3, 4, 8193, 8193], [7, 8, 9, 8193, 8193, 8193]]
    # a wav_length that reaches the last column leaves the row alone; one row, 1-D input
    t3, c3 = forward_inputs([1, 2], [2], [4, 5, 6], [2 * 1024])
    assert t3.tolist() == [[1, 2]] and c3.tolist() == [[4, 5, 6]]
    with pytest.raises(ValueError):
        forward_inputs(text, tl, codes, [1024])


def test_forward_rejects_what_the_device_does_not_do():
    """types, raw_mels and text_first=False raise in both modes, return_attentions=True in the loss mode (with return_latent=True it is
    ignored, as it always was), before anything touches the runtime"""
    torch = pytest.importorskip("torch")
    from detail_tts_amd.config import load_config
    from detail_tts_amd.gpt.model import UnifiedVoice
    uv = UnifiedVoice(None, load_config()["gpt"])
    a = (torch.zeros(1, 128, 8), [8], [[1, 2]], [2], [[3, 4]], [2048])
    for kw in (dict(types=torch.zeros(1)), dict(raw_mels=torch.zeros(1, 80, 8)), dict(text_first=False), dict(return_attentions=True)):
        for latent in ((False,) if "return_attentions" in kw else (False, True)):
            with pytest.raises(NotImplementedError, match="types, raw_mels, text_first=False and return_attentions=True"):
                uv.forward(*a, return_latent=latent, **kw)


def test_golden_file_holds_what_its_script_says(golden):
    f, g = golden("gpt_forward"), golden("gpt_forced")
    rows = f["logit_rows"]
    assert rows.tolist() == list(range(0, 8190, 37)) + [8190, 8191, 8192, 8193] and np.gcd(37, 32) == 1
    for tag, B, Lt, n in (("a", 2, 13, 12), ("b", 1, 127, 127)):
        k = lambda name: f[f"{tag}_{name}"]
        assert k("text").shape == (B, Lt) and k("codes").shape == (B, n) and k("text").dtype == np.int32 and k("codes").dtype == np.int32
        assert k("refer_lens").shape == k("text_lens").shape == k("wav_lens").shape == (B,)
        assert k("loss").shape == (2,) and k("loss").dtype == np.float32
        assert k("text_logprob").shape == (B, Lt + 2) and k("mel_logprob").shape == (B, n + 2)
        assert k("logit_pos").tolist() == [0, (n + 2) // 2, n + 1] and k("logits").shape == (B, 3, len(rows))
        assert k("text").min() >= 0 and k("text").max() < 257 and k("codes").min() >= 0 and k("codes").max() < 8192
        # the stored losses are the plain means of the stored per-position values, over ALL B * positions
        assert abs(-float(k("text_logprob").astype(np.float64).mean()) - float(k("loss")[0])) < 1e-5
        assert abs(-float(k("mel_logprob").astype(np.float64).mean()) - float(k("loss")[1])) < 1e-5
        assert (k("text_logprob") < 0).all() and (k("mel_logprob") < 0).all()
    assert np.array_equal(f["a_text"][0], g["text"][0]) and np.array_equal(f["a_codes"][0], g["codes"][0])
    assert np.array_equal(f["a_text"][1, :7], g["text"][0][:7]) and not f["a_text"][1, 7:].any()
    assert not np.array_equal(f["a_codes"][1], f["a_codes"][0])
    assert f["a_refer_lens"].tolist() == [64, 40] and f["a_wav_lens"].tolist() == [12 * 1024, 5 * 1024] and f["a_text_lens"].tolist() == [13, 7]
    rs = np.random.RandomState(int(f["b_seed"]))
    assert np.array_equal(rs.randint(1, 255, (1, 127)), f["b_text"]) and np.array_equal(rs.randint(0, 8192, (1, 127)), f["b_codes"])
    assert f["b_wav_lens"].tolist() == [127 * 1024] and 127 + 2 == 128 + 1                # one past gpt_score's 128-column tile
