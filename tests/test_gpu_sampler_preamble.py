"""GPU: the sampling step's preamble after the x-path fold - inp_block and the x half of integrating_conv composed at bind time into
one k = 3 conv, the code half of integrating_conv precomputed with the integrator, and the integrator's step-invariant front (layer 0:
GroupNorm + SiLU + c1) evaluated once per request.

One ragged batch for every test: B = 3, lens = [193, 77, 193] - 193 is one column past the 192-column conv tile, 77 lies inside the
first tile, and the two equal lengths share one unconditional integrator row (Nu = 2), so the per-sample residual index of the chunk-
opening conv is exercised.  cfg_streams = 1 puts the six stack samples into one chunk that crosses the cond | uncond boundary, 2 starts
chunks at stack samples 0 and 3.  n_steps = 9: at B + Nu = 5 the precompute takes 7 steps per launch, one full chunk and one partial."""
import numpy as np
import pytest

from conv_tile_probe import launches_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LENS = [193, 77, 193]
B, T = len(LENS), max(LENS)
STEP = 33
N_STEPS = 9
INTEG_STEPS_PER_LAUNCH = 7          # 36 samples per launch / (B + Nu = 5)

# test_sampler_routes_agree: max-abs difference of diff_sample (precomputed table) and nine diff_step calls (in-step route) on the
# inputs above, measured on the parent commit (both routes exist there; they differ in split-K and batch width) per (conv_x3,
# cfg_streams).  The gate is 4 x that value.  Both trees' measurements: profiles/sampler_preamble_errors.txt
ROUTES_PARENT = {(1, 1): 7.152557e-07, (1, 2): 5.960464e-07, (0, 1): 1.549721e-06, (0, 2): 1.549721e-06}


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def rt(weights):
    from detail_tts_amd.runtime import Runtime
    return Runtime(weights, folded=True, parts=("diffusion",))


def make_batch():
    rs = np.random.RandomState(53)
    return dict(x=rs.randn(B, 128, T).astype(np.float32), ce=(rs.randn(B, 768, T) * 0.5).astype(np.float32),
                noise=rs.randn(N_STEPS, B, 128, T).astype(np.float32))


@pytest.fixture(scope="module")
def batch():
    return make_batch()


@pytest.fixture(scope="module")
def oracle_rows(weights, batch):
    """DiffusionTts.forward of every row alone, conditional and conditioning-free: computed once, read by the forward test."""
    from oracle import diffusion as D
    ts = [D.make_schedule()["timestep_map"][STEP]]
    rows = []
    for b, L in enumerate(LENS):
        xb, cb = batch["x"][b:b + 1, :, :L], batch["ce"][b:b + 1, :, :L]
        rows.append((D.diffusion_forward(weights, xb, ts, cb)[0], D.diffusion_forward(weights, xb, ts, conditioning_free=True)[0]))
    return rows


class options:
    """set_option for the duration of a block; the defaults (conv_x3 = 1, cfg_streams = 0) are restored on the way out"""

    def __init__(self, rt, conv_x3=1, cfg_streams=0):
        self.rt, self.v = rt, dict(conv_x3=conv_x3, cfg_streams=cfg_streams)

    def __enter__(self):
        for k, v in self.v.items():
            self.rt.set_option(k, v)

    def __exit__(self, *exc):
        self.rt.set_option("conv_x3", 1)
        self.rt.set_option("cfg_streams", 0)


@pytest.mark.parametrize("conv_x3", [1, 0])
@pytest.mark.parametrize("ns", [1, 2])
def test_forward_of_ragged_batch_against_oracle_rows(rt, batch, oracle_rows, conv_x3, ns):
    """diff_forward of the batch, conditional and cond_free, on both kernel sets and both chunkings: every row against the numpy oracle of
    that row alone, at test_tiny_and_ragged_lengths' gate."""
    with options(rt, conv_x3, ns):
        oc = host(rt.diff_forward(dev(batch["x"]), STEP, dev(batch["ce"]), lens=LENS))
        ou = host(rt.diff_forward(dev(batch["x"]), STEP, cond_free=True, lens=LENS))
    for b, L in enumerate(LENS):
        ec, eu = maxabs(oc[b, :, :L], oracle_rows[b][0]), maxabs(ou[b, :, :L], oracle_rows[b][1])
        print(f"\n[conv_x3={conv_x3}, cfg_streams={ns}, row {b}] cond {ec:.2e} uncond {eu:.2e}")
        assert np.isfinite(oc[b, :, :L]).all() and np.isfinite(ou[b, :, :L]).all()
        assert ec < 3e-4 and eu < 3e-4, (conv_x3, ns, b, ec, eu)


def routes_difference(rt, batch, ns, conv_x3=1):
    """max-abs difference over the live columns between diff_sample (integrator table built in front of the loop) and N_STEPS
    successive diff_step calls (no table: the code-path term is evaluated inside every step) from the same x_T and the same noise"""
    with options(rt, conv_x3, ns):
        ce = dev(batch["ce"])
        xs = host(rt.diff_sample(ce, 7, list(range(B)), lens=LENS, n_steps=N_STEPS, x_init=dev(batch["x"]), step_noise=dev(batch["noise"]),
                                 denorm=False))
        x = dev(batch["x"])
        for k in range(N_STEPS):
            x = rt.diff_step(x, ce, 49 - k, 7, list(range(B)), lens=LENS, noise=dev(batch["noise"][k]))
        xr = host(x)
    assert all(np.isfinite(xs[b, :, :L]).all() and np.isfinite(xr[b, :, :L]).all() for b, L in enumerate(LENS))
    return max(maxabs(xs[b, :, :L], xr[b, :, :L]) for b, L in enumerate(LENS))


@pytest.mark.parametrize("conv_x3", [1, 0])
@pytest.mark.parametrize("ns", [1, 2])
def test_sampler_routes_agree(rt, batch, ns, conv_x3):
    """The table route and the in-step route compute the same nine steps (ROUTES_PARENT: the gate is 4 x the parent's difference).  On
    the exact fp32 kernels (conv_x3 = 0) the table route reads the integrator's shared layer 0 front through the GroupNorm
    coefficient pass' sample modulo and the conv's input sample index, over one full and one partial precompute launch."""
    e = routes_difference(rt, batch, ns, conv_x3)
    parent = ROUTES_PARENT[(conv_x3, ns)]
    print(f"\n[conv_x3={conv_x3}, cfg_streams={ns}] diff_sample vs {N_STEPS} x diff_step: max-abs {e:.3e} (parent {parent:.3e})")
    assert e < 4 * parent, (conv_x3, ns, e)


@pytest.mark.parametrize("ns", [1, 2])
def test_sampler_batch_equals_rows_alone(rt, batch, ns):
    """diff_sample of the batch against every row run alone, at test_sampler_varlen_batch_equals_single's gate.  Rows 0 and 2 have the
    same length and share one unconditional integrator row: each must match its OWN single-row run, not the other's."""
    ce = dev(batch["ce"])
    with options(rt, 1, ns):
        xb = host(rt.diff_sample(ce, 99, [11, 12, 13], lens=LENS, n_steps=2, denorm=True))
    alone = [host(rt.diff_sample(ce[b:b + 1, :, :L].contiguous(), 99, [11 + b], n_steps=2, denorm=True))[0] for b, L in enumerate(LENS)]
    for b, L in enumerate(LENS):
        e = maxabs(xb[b, :, :L], alone[b])
        print(f"\n[cfg_streams={ns}, row {b}] batch vs alone: max-abs {e:.2e}")
        assert e < 1e-4, (ns, b, e)
    assert maxabs(xb[0], alone[2]) > 1e-2 and maxabs(xb[2], alone[0]) > 1e-2


def launch_counts(rt, batch, ns, n_steps):
    """launches of one diff_sample: (convs, split passes, GroupNorm passes)"""
    ce = dev(batch["ce"])
    with options(rt, 1, ns):
        _, ran = launches_of(rt, lambda: host(rt.diff_sample(ce, 5, list(range(B)), lens=LENS, n_steps=n_steps, denorm=True)), level=2)
    convs = sum(n for name, n in ran.items() if name.startswith("conv_"))
    return convs, ran.get("split_planes_kernel", 0), ran.get("gn_split_planes_kernel", 0)


@pytest.mark.parametrize("n_steps", [2, N_STEPS])
@pytest.mark.parametrize("ns", [1, 2])
def test_preamble_launches_are_gone(rt, batch, ns, n_steps):
    """Per step and chunk: 48 convs (the chunk-opening x-path conv, 10 layers x 4, 3 tail blocks x 2, the out conv) and 37 GroupNorm
    passes; per step ONE split pass (x_t; the attention writes its output as planes at this T).  Per precompute launch (c of them): 12
    convs (three layers x 4, less layer 0's c1, plus the code half of integrating_conv), 8 GroupNorm passes (less layer 0's first) and
    one split pass (the integrator's output, for the code-half conv); once per request: layer 0's first GroupNorm pass and c1.
    The parent ran (2 + 48 NS) n_steps + 12 c convs, 3 n_steps split passes and 37 NS n_steps + 9 c GroupNorm passes."""
    c = -(-n_steps // INTEG_STEPS_PER_LAUNCH)
    convs, splits, gns = launch_counts(rt, batch, ns, n_steps)
    print(f"\n[cfg_streams={ns}, n_steps={n_steps}] convs {convs}, split passes {splits}, GroupNorm passes {gns}")
    assert convs == 48 * ns * n_steps + 12 * c + 1
    assert splits == n_steps + c
    assert gns == 37 * ns * n_steps + 8 * c + 1


@pytest.mark.parametrize("conv_x3", [1, 0])
def test_composed_x_path_weights_at_one_code(rt, weights, conv_x3):
    """Batch 1, T = 4 (one code), the unconditional code path: what reaches the trunk is the composed k = 3 conv on x (both edge columns
    see the zero padding) plus a T-constant code term."""
    from oracle import diffusion as D
    rs = np.random.RandomState(59)
    x = rs.randn(1, 128, 4).astype(np.float32)
    with options(rt, conv_x3, 0):
        out = host(rt.diff_forward(dev(x), STEP, cond_free=True))
    ref = D.diffusion_forward(weights, x, [D.make_schedule()["timestep_map"][STEP]], conditioning_free=True)
    e = maxabs(out, ref)
    print(f"\n[conv_x3={conv_x3}] max-abs {e:.2e}")
    assert np.isfinite(out).all() and e < 3e-4, (conv_x3, e)
