"""GPU: two branches of SynthesizerTrn.infer_stream that no other test reaches - a request too large for one decode session inside a
stream (17 rows: session after session on stage A's thread) and the per-request trace - at the smallest sizes (5 codes, 2 diffusion
steps, 16 mel frames)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TRACE_KEYS = {"host_a0", "host_a1", "host_a2", "host_b0", "host_b1", "ev_a0", "ev_a1", "ev_b0", "ev_b1", "ev_c1"}
KW = dict(max_generate_length=5, suppress_eos=True, diffusion_steps=2)


@pytest.fixture(scope="module")
def model(weights):
    from detail_tts_amd.vqvae.model_24k import SynthesizerTrn
    return SynthesizerTrn(weights, folded=True)


@pytest.fixture(scope="module")
def reqs():
    rs = np.random.RandomState(41)
    out = []
    for i, B in enumerate([1, 17, 2, 3]):
        Tr = 64 + 2 * i
        refer = torch.from_numpy((rs.randn(B, 128, Tr) * 2 - 5).astype(np.float32))
        text = torch.from_numpy(np.concatenate([rs.randint(3, 255, (B, 4)), np.zeros((B, 1), np.int64)], 1).astype(np.int32))
        out.append(dict(text=text, text_length=torch.full((B,), 5), refer=refer, refer_lengths=torch.tensor([Tr - (b % 4) for b in range(B)]),
                        seed=900 + i, sample_ids=[100 * i + b for b in range(B)]))
    return out


def _blocking(model, r):
    return model.infer(r["text"], r["text_length"], r["refer"], r["refer_lengths"], batch=True, seed=r["seed"], sample_ids=r["sample_ids"],
                       return_lengths=True, **KW)


@pytest.fixture(scope="module")
def streamed(model, reqs):
    """one traced run of the stream -> (results, trace)"""
    model.stream_trace = []
    try:
        outs = list(model.infer_stream(iter(reqs), **KW))
        torch.cuda.synchronize()            # every event of the trace is complete
        return outs, model.stream_trace
    finally:
        model.stream_trace = None


def test_stream_with_a_request_of_more_than_one_session_equals_infer(model, reqs, streamed):
    outs, _ = streamed
    assert len(outs) == len(reqs)
    for r, (wav, lens) in zip(reqs, outs):
        ref, rlens = _blocking(model, r)
        assert lens == rlens == [4 * 1024] * r["text"].shape[0]
        assert wav.shape == ref.shape and torch.equal(wav, ref)
        assert bool(torch.isfinite(wav).all()) and float(wav.pow(2).mean().sqrt()) > 1e-5


def test_stream_trace_has_one_complete_entry_per_request(reqs, streamed):
    _, trace = streamed
    assert len(trace) == len(reqs)
    for tr in trace:
        assert set(tr) == TRACE_KEYS
        assert tr["host_a0"] <= tr["host_a1"] <= tr["host_a2"] <= tr["host_b0"] <= tr["host_b1"]
        assert tr["ev_a0"].elapsed_time(tr["ev_a1"]) > 0 and tr["ev_b0"].elapsed_time(tr["ev_b1"]) > 0 and tr["ev_b1"].elapsed_time(tr["ev_c1"]) > 0


def test_paired_sessions_equal_single_ones(model, reqs):
    """groups [1], [17], [2, 3]: the last two requests share one 5-row session (launch-per-GEMV decode kernels on both sides)"""
    model.rt.set_option("gpt_token_kernel", 0)
    try:
        chain = list(model.infer_stream(iter(reqs), **KW))
        paired = list(model.infer_stream(iter(reqs), pair_stage_a=True, **KW))
    finally:
        model.rt.set_option("gpt_token_kernel", 1)
    assert len(chain) == len(paired) == len(reqs)
    for (w0, l0), (w1, l1) in zip(chain, paired):
        assert l0 == l1 and torch.equal(w0, w1)


def test_closed_early_leaves_the_handle_usable(model, reqs):
    gen = model.infer_stream(iter(reqs), **KW)
    wav, lens = next(gen)
    gen.close()
    again, alens = _blocking(model, reqs[0])
    assert lens == alens and torch.equal(again, wav)
