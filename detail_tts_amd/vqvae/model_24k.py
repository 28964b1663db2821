"""SynthesizerTrn / Generator / do_spectrogram_diffusion mirrors (reference: vqvae/model_24k.py).

`SynthesizerTrn.infer` keeps the reference signature (vqvae/model_24k.py:774) and its batch-1 behaviour by default;
keyword-only extras select a real batch (`batch=True`: every row is an independent utterance, bit-for-bit what it
would be alone), the noise seed / per-utterance stream ids, and forced codes (parity tests).
"""
from __future__ import annotations

import contextlib
import itertools
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ..config import COND_FREE_K, INFER_DIFFUSION_STEPS, MAX_GENERATE_LENGTH, MEL_MIN, NOISE_SCALE, REPETITION_PENALTY, TEMPERATURE, \
    TOP_P, TORCH_MEL_MAX, TRAINED_DIFFUSION_STEPS, load_config
from ..gpt.decode_options import beam_request
from ..gpt.sampling import check_forced_caps, repeat_rows, resolve_sampling, session_cap
from ..gpt.candidates import check_choose, check_num_candidates, expand_sample_ids, rank_candidates
from ..gpt.prompt import check_prompt_args, prompt_rows
from ..gpt.model import UnifiedVoice
from .. import _lib as _lib_slots
from ..pipeline import drain_session, group_requests, normalize_request, split_latents, split_session, stage_b, stage_c, stream_stage_a
from ..runtime import Runtime
from ..voice import check_clips, check_speaker, make_voice, model_dims
from .diff_model import DiffusionTts
from .inpaint import check_inpaint_args, splice_codes  # noqa: F401  (splice_codes: the host helper beside inpaint_mel)
from .utils.diffusion import SAMPLERS, SpacedDiffusion, check_timesteps, get_named_beta_schedule, space_timesteps


def normalize_torch_mel(mel):
    return 2 * ((mel - MEL_MIN) / (TORCH_MEL_MAX - MEL_MIN)) - 1


def denormalize_torch_mel(norm_mel):
    return ((norm_mel + 1) / 2) * (TORCH_MEL_MAX - MEL_MIN) + MEL_MIN


def do_spectrogram_diffusion(diffusion_model, diffuser, latents, conditioning_latents, temperature=1, verbose=True, *, seed=0,
                             sample_ids=None, lengths=None):
    """vqvae/model_24k.py:479-492: latents [B,n,768], conditioning_latents [B,1536] -> normalised mel [B,128,4n].
    temperature scales the initial noise (`torch.randn(output_shape) * temperature`, :488)."""
    out_len = latents.shape[1] * 4
    emb = diffusion_model.timestep_independent(latents, conditioning_latents, out_len, False, lengths=lengths)
    lens = None if lengths is None else [4 * int(n) for n in lengths]
    noise = None
    if temperature != 1:
        rt = diffusion_model.rt
        B = latents.shape[0]
        ids = list(range(B)) if sample_ids is None else list(sample_ids)
        noise = torch.zeros((B, 128, out_len), device=rt.device, dtype=torch.float32)
        for b in range(B):                  # each row's noise is indexed over its own [128, len] (the single-utterance order)
            L = out_len if lens is None else lens[b]
            z = rt.op_philox_normal(128 * L, seed, [ids[b]], 2, 0)           # STAGE_DIFF_INIT
            noise[b, :, :L] = z.reshape(128, L) * float(temperature)
    mel = diffuser.p_sample_loop(diffusion_model, (latents.shape[0], 128, out_len), noise=noise,
                                 model_kwargs={"precomputed_aligned_embeddings": emb}, progress=verbose, seed=seed,
                                 sample_ids=sample_ids, lens=lens)
    return mel[:, :, :out_len]


def sampling_args(diffusion_steps=None, sampler="p", eta=0.0):
    """Host-side check of infer()'s sampling arguments, before any launch -> (schedule key, sampler id, eta).
    diffusion_steps: None = 50 (the reference's infer_diffuser), else 1 .. 4000 steps of space_timesteps(4000, [N]) (2 .. 4000 for
    "dpmsolver++", which needs steps >= its order 2); sampler: "p" (ancestral, the reference's p_sample_loop), "ddim" (ddim_sample_loop
    with `eta` >= 0) or "dpmsolver++" (k_diffusion_sample_loop's DPM-Solver++(2M), eta must be 0).  The schedule key is the sorted model
    timesteps for "p" / "ddim" and the step count N for "dpmsolver++" (Runtime.sampler_schedule)."""
    n = INFER_DIFFUSION_STEPS if diffusion_steps is None else diffusion_steps
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= TRAINED_DIFFUSION_STEPS:
        raise ValueError(f"diffusion_steps must be an integer in [1, {TRAINED_DIFFUSION_STEPS}], not {diffusion_steps!r}")
    if sampler == "dpm++2m":
        raise NotImplementedError("sampler 'dpm++2m' is not implemented on the device (in k-diffusion it names Karras-sigma "
                                  "sample_dpmpp_2m): the reference's own DPM-Solver++(2M) path is sampler='dpmsolver++'")
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be 'p', 'ddim' or 'dpmsolver++', not {sampler!r}")
    try:
        eta = float(eta)
    except (TypeError, ValueError):
        raise ValueError(f"eta must be a number >= 0, not {eta!r}") from None
    if not eta >= 0.0 or eta == float("inf"):
        raise ValueError(f"eta must be a finite number >= 0, not {eta!r}")
    if sampler == "dpmsolver++":
        if int(n) < 2:
            raise ValueError(f"dpmsolver++ needs diffusion_steps >= 2 (its order), not {diffusion_steps!r}")
        if eta != 0.0:
            raise ValueError(f"dpmsolver++ draws no noise: eta must be 0, not {eta!r}")
        return int(n), SAMPLERS[sampler], 0.0
    return sorted(space_timesteps(TRAINED_DIFFUSION_STEPS, [int(n)])), SAMPLERS[sampler], eta


TRUNK_PRECISIONS = {"fp32": 0, "fp16": 1}

TRAIN_DIFFUSION_STEPS = 200         # vqvae/model_24k.py:560-561 (desired_diffusion_steps)
FORWARD_TARGETS = {"vqvae": "forward_vq", "gpt": "forward_gpt", "diff": "forward_diff"}      # cfg['train']['target'] -> stage loss (:740-751)


def draw_timesteps(seed, batch, steps=TRAIN_DIFFUSION_STEPS):
    """forward_diff's `t` when the caller gives none: `batch` integers in [0, steps) from numpy's RandomState(seed) on the host.  They
    cannot equal torch.randint's draw (vqvae/model_24k.py:673): a caller who wants the reference's numbers passes its t and noise."""
    return [int(v) for v in np.random.RandomState(int(seed) % (1 << 32)).randint(0, steps, size=int(batch))]


def draw_segment_starts(seed, lengths, seg):
    """forward_flowvae's `ids_slice` when the caller gives none: floor(u * (len - seg + 1)) per row (rand_slice_segments,
    vqvae/modules/commons.py:76-83) with u from numpy's RandomState(seed) on the host.  They cannot equal torch.rand's draw: a caller
    who wants the reference's numbers passes its ids_slice and noise."""
    u = np.random.RandomState(int(seed) % (1 << 32)).random_sample(len(lengths))
    return [min(int(np.floor(float(v) * (int(n) - seg + 1))), int(n) - seg) for v, n in zip(u, lengths)]


def check_flowvae_args(y_shape, y_lengths, seg, ids_slice=None):
    """Host-side checks of forward_flowvae, before any launch -> (lengths, ids_slice or None).  ValueError when T % 4 != 0 (the
    reference asserts it), when a row is shorter than the segment (the reference would slice garbage there) and when a given
    ids_slice leaves [0, len - seg]."""
    B, T = int(y_shape[0]), int(y_shape[-1])
    if T % 4 != 0:
        raise ValueError(f"forward_flowvae needs a frame count divisible by 4 (the reference asserts it), not {T}")
    yl = [int(v) for v in torch.as_tensor(y_lengths).reshape(-1).tolist()]
    if len(yl) != B:
        raise ValueError(f"forward_flowvae: {len(yl)} lengths for {B} rows")
    for b, n in enumerate(yl):
        if n > T:
            raise ValueError(f"forward_flowvae: row {b} has length {n} > {T} frames")
        if n < seg:
            raise ValueError(f"forward_flowvae: row {b} has {n} frames, fewer than the segment's {seg} (train.segment_size // data.hop_length)")
    if ids_slice is None:
        return yl, None
    ids = [int(v) for v in torch.as_tensor(ids_slice).reshape(-1).tolist()]
    if len(ids) != B or any(i < 0 or i > n - seg for i, n in zip(ids, yl)):
        raise ValueError(f"forward_flowvae: ids_slice {ids} must hold one start in [0, len - {seg}] per row (lengths {yl})")
    return yl, ids


def trunk_precision_arg(trunk_precision):
    """Host-side check of infer()'s `trunk_precision`, before any launch -> None (what the model's config says) or the value of option
    "trunk_fp16" for this call: "fp32" = the three-product split-precision trunk, "fp16" = the reference's use_fp16 mode
    (vqvae/diff_model.py:299-309): layers[1:] of the trunk as single fp16 products with fp32 accumulation."""
    if trunk_precision is None:
        return None
    if trunk_precision not in TRUNK_PRECISIONS:
        raise ValueError(f"trunk_precision must be 'fp32' or 'fp16' (or None: the model's config), not {trunk_precision!r}")
    return TRUNK_PRECISIONS[trunk_precision]


class Generator:
    """vqvae/model_24k.py:221-296"""

    def __init__(self, rt):
        self.rt = rt

    def forward(self, x, g=None, lengths=None):
        g2 = None if g is None else g.reshape(g.shape[0], -1).float().contiguous()      # `if g is not None` (:271-273)
        return self.rt.generator(x.float().contiguous(), g2, lengths)

    __call__ = forward

    HALO = 16      # frames of context on each side: the generator's receptive field is 13.2 frames

    def stream(self, x, g, chunk=64):
        """Chunked synthesis for long utterances: yields wav pieces [B,1,256*n] whose concatenation equals
        forward(x, g) to fp32 rounding.  The generator is purely convolutional, so every chunk is computed inside a window with
        a 16-frame halo and only its interior is emitted; peak memory is one window instead of the whole utterance."""
        x = x.float().contiguous()
        g2 = g.reshape(g.shape[0], -1).float().contiguous()
        T, H = x.shape[-1], self.HALO
        for t0 in range(0, T, chunk):
            t1 = min(T, t0 + chunk)
            a, b = max(0, t0 - H), min(T, t1 + H)
            w = self.rt.generator(x[:, :, a:b].contiguous(), g2)
            yield w[:, :, (t0 - a) * 256:(t1 - a) * 256]


def write_wav(path, wav, sample_rate=24000):
    """torchaudio.save(path, wav, 24000) of api.py:50 without torchaudio: mono / [C, S] float tensor in [-1, 1] -> 16-bit PCM."""
    import wave
    w = torch.as_tensor(wav).detach().float().cpu()
    if w.dim() == 1:
        w = w[None]
    pcm = (w.clamp(-1.0, 1.0) * 32767.0).round().to(torch.int16).t().contiguous().numpy()
    with wave.open(str(path), "wb") as f:
        f.setnchannels(w.shape[0])
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(pcm.tobytes())


class MultiPeriodDiscriminator:
    """vqvae/model_24k.py:407-431 on the device, forward values only: DiscriminatorS and DiscriminatorP of periods 2, 3, 5, 7, 11.

    `state` is the checkpoint's 'D' state dict (train.py:146; weight-norm pairs or the parametrizations form, torch or numpy), or None
    (load_state_dict later).  `model=` a SynthesizerTrn (or a Runtime): the weights are bound to its handle, next to the model's, which
    flowvae_stage_losses needs; otherwise `device=` makes a handle that holds nothing else.  The packed weights (about 50 M floats) are
    a blob of their own: the model's blob is what it is without them."""

    periods = (2, 3, 5, 7, 11)

    def __init__(self, state=None, *, model=None, device=None, cfg=None, use_spectral_norm=False, folded=False):
        if use_spectral_norm:
            raise NotImplementedError("use_spectral_norm=True is not implemented on the device (the reference trains with weight_norm)")
        if model is not None and device is not None:
            raise ValueError("MultiPeriodDiscriminator: give model= or device=, not both")
        if model is not None:
            self.rt = model.rt if hasattr(model, "rt") else model
        else:
            self.rt = Runtime({}, cfg, device=device or "cuda:0", parts=(), folded=True)
        self.device = self.rt.device
        self.bound = False
        if state is not None:
            self.load_state_dict(state, folded=folded)

    def load_state_dict(self, state, strict=True, folded=False):
        self.rt.bind_discriminator(state, folded=folded)
        self.bound = True
        return self

    def eval(self):
        return self

    def to(self, device):
        if torch.device(device) != self.device:
            raise NotImplementedError("re-create the discriminator on the target device (weights are bound to one GPU)")
        return self

    def forward(self, y, y_hat):
        """y, y_hat [B,1,t], t >= 12 -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs): 6 scores [B, H p] and 6 lists of maps [B, C, H, p] ([B, C, T]
        for DiscriminatorS; 7 maps there, 6 in each DiscriminatorP) per side, cuda fp32, in the reference's shapes.  The maps are
        permuted views of one buffer laid out [2B, p, C, H]; real and generated run as one batch, each weight read once."""
        y, y_hat = torch.as_tensor(y), torch.as_tensor(y_hat)
        if y.dim() != 3 or y.shape[1] != 1 or tuple(y.shape) != tuple(y_hat.shape):
            raise ValueError(f"MultiPeriodDiscriminator: y and y_hat must share one shape [B, 1, t], not {list(y.shape)} and {list(y_hat.shape)}")
        if y.shape[2] < 12:
            raise ValueError(f"MultiPeriodDiscriminator: t = {y.shape[2]}; t must be at least 12 (every reflect pad shorter than the signal)")
        y = y.to(self.device, torch.float32).contiguous()
        y_hat = y_hat.to(self.device, torch.float32).contiguous()
        B = y.shape[0]
        _, maps = self.rt.disc_forward(y, y_hat)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        m = 0
        for d in range(1 + len(self.periods)):
            fr, fg = [], []
            for _ in range(7 if d == 0 else 6):
                a = maps[m]                                        # [2B, p, C, H]
                v = a[:, 0] if d == 0 else a.permute(0, 2, 3, 1)   # [2B, C, T] / [2B, C, H, p]
                fr.append(v[:B]); fg.append(v[B:])
                m += 1
            fmap_rs.append(fr); fmap_gs.append(fg)
            y_d_rs.append(torch.flatten(fr[-1], 1, -1))            # (h, w) order, as the reference flattens [B, 1, H, p]
            y_d_gs.append(torch.flatten(fg[-1], 1, -1))
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs

    __call__ = forward


class SynthesizerTrn:
    def __init__(self, state, cfg=None, device="cuda:0", folded=False):
        self.cfg = load_config(cfg)
        self.rt = Runtime(state, self.cfg, device=device, folded=folded)
        self.device = self.rt.device
        self.gpt = UnifiedVoice(self.rt, self.cfg["gpt"])
        self.diffusion = DiffusionTts(self.rt, self.cfg["diffusion"])
        self.dec = Generator(self.rt)
        self.text_loss_weight = self.cfg["train"]["text_weight"]      # vqvae/model_24k.py:603-604
        self.mel_loss_weight = self.cfg["train"]["mel_weight"]
        self.infer_diffuser = SpacedDiffusion(space_timesteps(TRAINED_DIFFUSION_STEPS, [INFER_DIFFUSION_STEPS]),
                                              betas=get_named_beta_schedule("linear", TRAINED_DIFFUSION_STEPS),
                                              conditioning_free=True, conditioning_free_k=COND_FREE_K, sampler="dpm++2m")
        self.rt.timestep_map = list(self.infer_diffuser.timestep_map)
        # vqvae/model_24k.py:560-580: the training / validation diffuser, 200 of the 4000 steps, no guidance (its sampling loops stay refused)
        self.desired_diffusion_steps = TRAIN_DIFFUSION_STEPS
        self.diffuser = SpacedDiffusion(space_timesteps(TRAINED_DIFFUSION_STEPS, [TRAIN_DIFFUSION_STEPS]),
                                        betas=get_named_beta_schedule("linear", TRAINED_DIFFUSION_STEPS),
                                        conditioning_free=False, conditioning_free_k=COND_FREE_K)
        self.diffuser.rt = self.infer_diffuser.rt = self.rt
        self.target = self.cfg["train"].get("target")                 # :631
        self.stage_ms = None          # set to {} to collect per-stage hipEvent timings of the next infer() call
        self._voc_stream = None       # second stream of infer(stream_vocoder=True)
        self._gpt_stream = None       # high-priority stage-A stream of infer_stream()
        self._a_pool = None           # ... and its issuing thread
        self.stream_trace = None      # set to [] to collect the per-request timeline of infer_stream()
        self.vocoder_done = None
        self.vocoder_ticket = 0
        self.saturated_requests = 0   # requests of infer_stream whose stage C was re-run on the exact fp32 kernels

    def eval(self):
        return self

    def _check_trunk_precision(self, trunk_precision):
        """-> the per-call value of option "trunk_fp16" (None: none); "fp16" without the split-precision kernels is refused here"""
        prec = trunk_precision_arg(trunk_precision)              # (the value itself: no device, no model state)
        if prec == 1 and not self.rt.get_option("conv_x3"):
            raise ValueError("trunk_precision='fp16' needs the split-precision kernels (option conv_x3 = 1): the exact fp32 kernels "
                             "have no one-product mode")
        return prec

    @contextlib.contextmanager
    def _trunk_precision(self, prec):
        """option "trunk_fp16" = prec around the launches of ONE diffusion; the previous value is back when the block ends, whatever
        happened inside (the kernel choice is made at launch time, so the enqueued work keeps it)"""
        if prec is None:
            yield
            return
        prev = self.rt.get_option("trunk_fp16")
        self.rt.set_option("trunk_fp16", prec)
        try:
            yield
        finally:
            self.rt.set_option("trunk_fp16", prev)

    def to(self, device):
        if torch.device(device) != self.device:
            raise NotImplementedError("re-create the model on the target device (weights are bound to one GPU)")
        return self

    # ------------------------------------------------------------------------------------------------------------
    def infer(self, text, text_length, refer, refer_lengths, noise_scale=NOISE_SCALE, *, batch=False, seed=None, sample_ids=None,
              forced_codes=None, max_generate_length=MAX_GENERATE_LENGTH, top_k=50, suppress_eos=False, return_lengths=False,
              stream_vocoder=False, vocoder_chunk=256, wait=True, check_range=True, diffusion_steps=None, sampler="p", eta=0.0,
              trunk_precision=None, num_candidates=1, choose=None, return_candidates=False, prompt_codes=None, decode_options=None,
              speaker=None, return_alignment=False, align_options=None, speed=None, durations=None, span_rates=None, sampling=None):
        """vqvae/model_24k.py:774-810.  Returns wav [B,1,1024*n_max] (B=1 unless batch=True).

        sampling: stage A's sampling settings, per row (gpt/sampling.py states the keys, ranges and refusals): None (today's path: the
        reference's constants and the call's top_k), a dict (every row), or a list of B entries, each None or a dict of temperature,
        top_p, top_k, repetition_penalty, typical_mass, max_generate_length, do_sample and decode_options' eight non-beam keys.  A
        missing key takes the call's top_k / max_generate_length / decode_options, else the reference's constant.  The rows decode in
        ONE session, each under its own settings and finished at its own cap (the device sampler reads the row's slot of its control
        block); with num_candidates the settings repeat with the rows.  Not with num_beams > 1.  None, {} or a list of None: today's
        launches and bits.  With forced_codes nothing is sampled here (the codes go straight to the teacher-forced pass), so the
        settings are checked and otherwise not used; a row cap below the length of its forced row is a ValueError.  How any setting
        sounds under a trained checkpoint is unmeasured.

        speed / durations / span_rates (at most one; duration.py): how fast the voice speaks.  The reference's
        DiffusionTts.timestep_independent expands the code embedding to any frame count (F.interpolate nearest,
        vqvae/diff_model.py:252) and only do_spectrogram_diffusion fixes 4 frames per code; here row b gets T_b frames, a multiple of 4:
        speed (a rate, or one per row, in [0.25, 4]) -> T_b = max(4, 4 int(n_b / speed_b + 0.5)) under torch's own nearest map;
        durations (per row the frames of every code, >= 0; a sum off a multiple of 4 extends the last speaking code) and span_rates
        (per row (first_code, last_code, rate) spans, inclusive as return_alignment hands them out; a code outside every span keeps its
        4 frames) need forced_codes - re-render the codes of an earlier call with one word held longer.  Checked on the host before
        any launch.  Under a plan the waveform is [B,1,256*max(T_b)], the returned lengths are 256 T_b and return_alignment's times
        follow the map; it composes with every other keyword (num_candidates: the plan applies to the winners).  speed None, or 1.0
        with the other two absent: today's launches and bits.  Audio quality at other rates is unmeasured (no trained checkpoint).

        return_alignment: the call also returns, as its LAST value, the text-to-audio alignment of the synthesised codes - one
        dictionary per row, as align() gives it (per-token and per-word code spans and times, and the coverage / skipped /
        longest_stay figures that show a decode which skipped or repeated text).  One extra teacher-forced pass over the generated
        codes alone (what infer already runs behind a prompt or beams) with the attention read-out, enqueued behind stage C; it
        composes with prompt_codes, num_candidates (the chosen rows), beams, forced_codes and speaker.  align_options: None or a dict of
        align()'s layers / head_weights / space_id.  False (the default): no extra launch, the same bits.

        speaker: a Voice (get_conditioning_latents; voice.py) in the place of the prompt mel - refer and refer_lengths are then None
        (both given, or neither: ValueError before any launch).  S = 1 serves every row, else S has to be B.  Neither prompt encoder
        is launched: stage A takes the voice's gpt member (UnifiedVoice.compute_embeddings' cond_latents), stage B its diffusion
        member.  With a voice made from the same [B,128,Tr] prompt the call returns the `refer` call's bits; every other option
        composes with it.  None: today's path, untouched.

        decode_options: None or a dict of HF generate()'s remaining decode-time keywords, which the reference's inference_speech_*
        would hand to HF (gpt/decode_options.py: no_repeat_ngram_size, min_length, min_new_tokens, exponential_decay_length_penalty,
        suppress_tokens, begin_suppress_tokens, min_p, epsilon_cutoff), checked on the host before any launch and served by the device
        sampler.  None or {}: today's decode, bit for bit.  With num_candidates > 1 every candidate decodes under the options; its
        score stays the unconstrained model's log-probability.

        prompt_codes ([B, m] or a list of B one-dimensional arrays of mel codes, e.g. encode()'s of a prompt mel; not with forced_codes or
        num_candidates > 1): the reference's own composition with line 782 calling UnifiedVoice.inference_speech_valle - stage A continues
        the code sequence from the acoustic prompt (one prefill over [cond | text | prompt], gpt/prompt.py) and the diffusion latents
        come from the teacher-forced pass on the GENERATED codes alone (:795-799, gpt_latents), not from the session's decode-time latents,
        which have the prompt in context.  None: today's path, untouched.

        num_candidates = N in 1 .. 16 (not with forced_codes): stage A samples N code sequences per utterance (rows expanded with
        repeat_interleave; candidate c of utterance b draws from Philox stream sample_ids[b] + c * 2**20, so candidate 0 IS the N = 1
        decode), scores each with the model's own log-probability from the decode-time latents (dtts_gpt_score: one fused launch, no second
        GPT pass) and keeps the best (gpt/candidates.py rank_candidates: mean log-probability, candidates that drew the stop token
        first, ties to the lowest index), or candidate choose[b].  Stages B and C run on the B winners with the original sample_ids:
        when candidate 0 wins the waveform is the N = 1 call's bit for bit.  return_candidates: the call also returns
        dict(codes [B,N,G], ncodes [B,N], scores [B,N], stopped [B,N], chosen [B]) as its last value.  The default (N = 1, no
        return_candidates) launches no scoring and is unchanged.  Whether best-of-N improves the audio is unmeasured (no trained
        checkpoint).

        diffusion_steps / sampler / eta: stage B's schedule (None = the reference's 50 steps) and sampler ("p" = the reference's
        ancestral p_sample_loop, "ddim" = ddim_sample_loop with `eta`, "dpmsolver++" = the DPM-Solver++(2M) the reference's own
        infer_diffuser configures, k_diffusion_sample_loop); see sampling_args.  Fewer steps cost proportionally less.

        trunk_precision: "fp32" / "fp16" for THIS call's diffusion (None = what the config's diffusion.use_fp16 / diffusion.enable_fp16
        says): "fp16" is the reference's use_fp16 mode, layers[1:] of the trunk as single fp16 products (trunk_precision_arg); the
        model's own setting is back when the call returns.

        stream_vocoder: stage C runs on a second HIP stream, its generator window by window (`vocoder_chunk` mel frames + halo,
        dtts_vocoder_stream; 0 = one shot).  With wait=False the call returns while stage C is still running - `self.vocoder_done` is the event
        to wait on before reading the waveform - so the NEXT call's GPT decode and diffusion (first stream) overlap this call's
        vocoder (BASELINE configs[4]: long-form batches, overlapped diffusion / vocoder streams).

        check_range (with wait=True): the call waits for its own waveform and raises if stage C's split-precision planes saturated on
        THIS request (dtts_vocoder_check; the reference computes those convs in fp32).  With wait=False (or check_range=False) the call
        stays asynchronous: wait on `self.vocoder_done`, then call `self.check_vocoder()` before reading the waveform."""
        sched_ts, sampler_id, eta = sampling_args(diffusion_steps, sampler, eta)
        prec = SynthesizerTrn._check_trunk_precision(self, trunk_precision)
        ncand = check_num_candidates(num_candidates, forced_codes)
        check_prompt_args(prompt_codes, forced_codes, ncand)
        processors, beam = beam_request(decode_options, forced_codes=forced_codes, num_candidates=ncand, return_candidates=return_candidates)
        st = normalize_request(text, text_length, refer, refer_lengths, seed, sample_ids, forced_codes, batch=batch, speaker=speaker,
                               dims=None if speaker is None else model_dims(self.cfg), speed=speed, durations=durations,
                               span_rates=span_rates)
        B, rl, texts, seed, sample_ids, forced_codes = st.B, st.rl, st.texts, st.seed, st.sids, st.forced
        if sampling is not None and not batch and not hasattr(sampling, "items"):
            sampling = sampling[:1]
        samp_rows = resolve_sampling(sampling, B, top_k=top_k, max_generate_length=max_generate_length, decode_options=processors,
                                     num_beams=(beam or {}).get("num_beams"))      # (ValueError: before any launch)
        caps = None if samp_rows is None else [r["max_generate_length"] for r in samp_rows]
        check_forced_caps(samp_rows, forced_codes)
        if prompt_codes is not None:       # (ValueError on a bad row count or code: before any launch)
            prompt_codes = prompt_rows(prompt_codes if batch else prompt_codes[:1], B)
        choose = check_choose(choose, B, ncand)
        candidates = (ncand > 1 or return_candidates) and forced_codes is None
        if return_candidates and not candidates:
            raise ValueError("return_candidates: forced_codes leave no candidates to report")
        cand_ids = expand_sample_ids(sample_ids, ncand) if candidates else None      # (ValueError on colliding streams: before any launch)
        cond = None                        # the conditioning encoder's output, handed in when the request carries a voice
        if st.voice is not None:
            st.voice = st.voice.for_batch(B)
            refer, cond = None, st.voice.gpt
        else:
            refer = st.refer = st.refer.to(self.device, torch.float32).contiguous()
        ev, cand = [], None

        def mark(name):
            if self.stage_ms is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record(torch.cuda.current_stream(self.device))
                ev.append((name, e))

        mark("start")
        # ---- stage A: codes + latents (:782-799)
        session = forced_codes is None and B * (ncand if candidates else 1) <= 16 and not beam
        if beam:        # HF's beam search on the device; the best hypothesis's latents come from the return_latent pass, as behind a prompt
            seqs, blens, _ = self.rt.gpt_generate_beams(refer, rl, texts, num_return_sequences=1, max_generate_length=max_generate_length,
                                                        repetition_penalty=REPETITION_PENALTY, suppress_eos=suppress_eos,
                                                        prompt_codes=prompt_codes, processors=processors or None, cond=cond, **beam)
            n, = split_session(blens[:, 0], [B])
            out_codes = [seqs[b, 0, : n[b]] for b in range(B)]
            st.lat, st.n = self.rt.gpt_latents(refer, rl, texts, out_codes, cond=cond), n
        elif forced_codes is None:
            kw = dict(max_generate_length=max_generate_length, top_k=top_k, top_p=TOP_P, temperature=TEMPERATURE,
                      repetition_penalty=REPETITION_PENALTY, suppress_eos=suppress_eos)
            if prompt_codes is not None:
                kw["prompt_codes"] = prompt_codes
            if processors:
                kw["processors"] = processors
            if samp_rows is not None:   # every row under its own settings; the session runs to its largest row cap
                max_generate_length = kw["max_generate_length"] = session_cap(samp_rows, max_generate_length)
                kw["rows"] = repeat_rows(samp_rows, ncand) if candidates and ncand > 1 else samp_rows
            a_refer, a_rl, a_texts, a_ids = refer, rl, texts, sample_ids
            if cond is not None:
                kw["cond"] = cond if not (candidates and ncand > 1) else cond.repeat_interleave(ncand, 0).contiguous()
            if candidates and ncand > 1:                            # HF's num_return_sequences expansion: every row N times
                a_refer = None if refer is None else refer.repeat_interleave(ncand, 0).contiguous()
                a_rl = [v for v in rl for _ in range(ncand)]
                a_texts = [t for t in texts for _ in range(ncand)]
            if candidates:
                a_ids = cand_ids
            if session:         # one decode session: prefill (+ first token), then 16-token chunks; finish flags polled per chunk
                self.rt.gpt_prefill(a_refer, a_rl, a_texts, seed, a_ids, **kw)
                mark("gpt_prefill")
                codes, ncodes, lat = drain_session(self.rt, max_generate_length, suppress_eos)
            else:
                codes, ncodes, lat = self.rt.gpt_generate(a_refer, a_rl, a_texts, seed, a_ids, **kw)
            if candidates:
                # the model's own log-probability of every candidate, from the latents its tokens were drawn from (stop token included)
                nc = [int(c) for c in ncodes]
                logp = self.rt.gpt_score(lat, [codes[r, : nc[r]] for r in range(B * ncand)]).cpu().numpy()
                stopped = [bool(codes[r, nc[r] - 1] == self.gpt.stop_mel_token) for r in range(B * ncand)]
                chosen, scores = [], np.zeros((B, ncand), np.float64)
                for b in range(B):
                    r0, r1 = b * ncand, (b + 1) * ncand
                    best, scores[b] = rank_candidates(logp[r0:r1], nc[r0:r1], stopped[r0:r1])
                    chosen.append(best if choose is None else choose[b])
                cand = dict(codes=codes.reshape(B, ncand, -1).copy(), ncodes=np.asarray(nc, np.int32).reshape(B, ncand), scores=scores,
                            stopped=np.asarray(stopped, bool).reshape(B, ncand), chosen=list(chosen))
                rows = [b * ncand + c for b, c in enumerate(chosen)]
                ncodes = ncodes[rows]
                if ncand > 1:                                       # the winners' latent rows, gathered on the device
                    lat = lat.index_select(0, torch.as_tensor(rows, device=self.device))
            n, = split_session(ncodes, [B], caps)
            if prompt_codes is None:
                split_latents(lat, [st], [n])
            else:       # behind a prompt they are not: the reference's return_latent pass sees the generated codes alone (:796-799)
                st.lat, st.n = self.rt.gpt_latents(refer, rl, texts, [codes[b, : n[b]] for b in range(B)], cond=cond), n
            if return_alignment:                                        # the chosen rows' codes, stop token cut
                out_codes = [codes[r, : n[b]] for b, r in enumerate(rows if candidates else range(B))]
        else:
            n = st.n = [len(c) for c in forced_codes]
            st.lat = self.rt.gpt_latents(refer, rl, texts, forced_codes, cond=cond)
            out_codes = forced_codes
        mark("gpt_decode" if session else "gpt")
        # ---- stage B (:802-804)
        mel, lens_t = stage_b(self, st, sampler_id, eta, prec, sched_ts=sched_ts, mark=mark)
        mark("diff_sample")
        # ---- stage C (:805-809)
        if stream_vocoder:
            cur = torch.cuda.current_stream(self.device)
            if self._voc_stream is None:
                self._voc_stream = torch.cuda.Stream(self.device)
            wav, self.vocoder_done, self.vocoder_ticket = stage_c(self.rt, self._voc_stream, cur, mel, st, lens_t, noise_scale, vocoder_chunk)
            if wait:
                cur.wait_event(self.vocoder_done)
        else:
            wav = self.rt.vocoder(mel, seed, sample_ids, lens=lens_t, noise_scale=noise_scale)
            self.vocoder_ticket = self.rt.vocoder_ticket()
        if wait and check_range and self.rt.vocoder_check_active():      # (check off - DTTS_X3_RANGE_CHECK=0, conv_x3 / voc_x3 = 0: nothing to wait for)
            torch.cuda.current_stream(self.device).synchronize()
            self.rt.vocoder_check(self.vocoder_ticket)
        mark("vocoder")
        if self.stage_ms is not None:
            torch.cuda.synchronize(self.device)
            for (_, a), (nm, b) in zip(ev[:-1], ev[1:]):
                self.stage_ms[nm] = self.stage_ms.get(nm, 0.0) + a.elapsed_time(b)
        ret = (wav,) + (([256 * t for t in lens_t],) if return_lengths else ()) + ((cand,) if return_candidates else ())
        if return_alignment:
            ret += (self._alignment_of(texts, out_codes, refer, rl, cond, **(align_options or {}), plan=st.plan),)
        return ret if len(ret) > 1 else wav

    def check_vocoder(self, ticket=None):
        """raise if the stage-C call `ticket` (default: the last one issued) saturated; the caller has waited for its waveform"""
        self.rt.vocoder_check(self.vocoder_ticket if ticket is None else ticket)

    # ------------------------------------------------------------------------------------------------------------
    def infer_stream(self, requests, noise_scale=NOISE_SCALE, *, max_generate_length=MAX_GENERATE_LENGTH, top_k=50, suppress_eos=False,
                     vocoder_chunk=0, pair_stage_a=False, on_saturation="rerun_fp32", diffusion_steps=None, sampler="p", eta=0.0,
                     trunk_precision=None, decode_options=None, sampling=None):
        """Batch server: `infer(..., batch=True)` over a sequence of request batches, software-pipelined over three HIP streams.

        requests: iterable of dicts with keys text [B,Lt], text_length [B], refer [B,128,Tr], refer_lengths [B] (or, in the place of those
        two, speaker = a Voice: see infer) and optionally seed, sampling (per-row sampling settings as infer takes them: a dict or one
        entry per row; `sampling=` of this call, None or a dict, serves the requests that carry none; requests paired into one decode
        session keep their own rows' settings), ready (a torch.cuda.Event: stage A's stream waits for it before it reads the request's
        device tensors - for a caller that made them on a stream of its own, as infer_many makes its voices), speed / durations / span_rates (see infer: the request's speaking rate; its
        yielded lengths are then 256 T_b),
        sample_ids, forced_codes (per-row code arrays fed through the KV-cache decode instead of sampling: tests / ragged benchmarks;
        <= 16 rows) (any B; up to 16 utterances share one decode session; with pair_stage_a two consecutive requests of <= 8 utterances
        are decoded as ONE session - stage A of requests i + 1 and i + 2 together under stage B of requests i - 1 and i).  Yields (wav [B,1,1024*n_max], lengths) per request, in order; every
        result is bit-identical to `infer(**request, batch=True)` with the same seed and sample ids.

        Stage A of request i+1 (GPT prefill + decode: a chain of short latency-bound kernels that leaves the chip mostly idle) runs
        on a high-priority stream under stage B of request i (50 diffusion steps: throughput-bound); stage C of request i runs on a
        third stream under stage B of request i+1.  Stage A is issued from a second host thread; the calling thread blocks only on a decode session's
        results (the code lengths size the diffusion) and on the waveform it is about to hand out, which is the PREVIOUS request's
        (one request of lag), so the diffusion stream never drains.  Device tensors handed over in a request must be complete (not pending on another stream):
        stage A reads them on its own stream.

        on_saturation: what happens to a request whose stage C saturated its split-precision planes (dtts_vocoder_check).  "rerun_fp32"
        (default): THAT request's stage C is run again on the exact fp32 kernels (option voc_x3 = 0, which cannot saturate) and its
        waveform is handed out as usual - the requests behind it, whose stages are already enqueued, are not lost;
        "raise": the error leaves the generator (and ends the stream).

        diffusion_steps / sampler / eta / trunk_precision: as in infer(), one schedule and one trunk mode for every request of the stream
        (the option is set around each request's diffusion launches only, on this thread: nothing leaks into other calls).

        decode_options: as in infer(), one set for every request of the stream (None or {}: today's decode).  A beam search
        (`num_beams` > 1) is refused with a ValueError before anything starts: a beam session cannot share its rows with another request."""
        assert on_saturation in ("rerun_fp32", "raise")
        processors, _ = beam_request(decode_options, stream=True)
        # sampling: every request dict may carry `sampling` (as infer takes it: a dict, or one entry per row); `sampling=` here is the
        # stream's default for requests without one (None or a dict).  Two requests paired into one session keep their own rows' settings.
        if sampling is not None and not hasattr(sampling, "items"):
            raise ValueError("infer_stream: the stream-wide `sampling` has to be None or a dict (a request dict takes the per-row list)")
        samp = dict(default=sampling, top_k=top_k, max_generate_length=max_generate_length, decode_options=processors)
        resolve_sampling(sampling, 1, **{k: v for k, v in samp.items() if k != "default"})      # (ValueError before anything starts)
        sched_ts, sampler_id, eta = sampling_args(diffusion_steps, sampler, eta)
        prec = SynthesizerTrn._check_trunk_precision(self, trunk_precision)
        dev = self.device
        cur = torch.cuda.current_stream(dev)
        sched = self.rt.sampler_schedule(sched_ts, sampler_id)      # built here, once: no table allocation inside the pipelined loop
        if self._gpt_stream is None:
            hi = torch.cuda.Stream.priority_range()[1] if hasattr(torch.cuda.Stream, "priority_range") else -1
            self._gpt_stream = torch.cuda.Stream(dev, priority=hi)
        if self._voc_stream is None:
            self._voc_stream = torch.cuda.Stream(dev)
        sa, sc = self._gpt_stream, self._voc_stream
        trace = self.stream_trace          # a list: per-request host times and stream events (tools/pipeline_trace.py)
        kw = dict(max_generate_length=max_generate_length, top_k=top_k, top_p=TOP_P, temperature=TEMPERATURE,
                  repetition_penalty=REPETITION_PENALTY, suppress_eos=suppress_eos)
        if processors:
            kw["processors"] = processors
        # Stage A here decodes NEXT TO the previous request's diffusion: its sessions of 5 .. 8 rows take the 64-workgroup token kernel
        # (gpt_token_n.hip: the same codes and latents bit for bit, 105 instead of 80 ms alone, but half the CUs for 1.3 x as long:
        # -5 .. -7 ms per pipelined request, profiles/r06_token_wgs.txt); a blocking infer() keeps the 128-workgroup kernel.
        # ... except the FIRST session of a stream: nothing runs next to it, so it takes the fastest decode (0: 128 workgroups, 80 ms)
        token_wgs = itertools.chain([0], itertools.repeat(int(os.environ.get("DTTS_STREAM_TOKEN_WGS", "64"))))

        # Stage A is issued from its own host thread: a kernel-launch call blocks once its stream's hardware queue is full, so one
        # thread could not enqueue request i+1's decode (12 K launches) while it is still feeding request i's diffusion (10 K).  The
        # library supports exactly this split (include/detail_hip.h, "Threads"); ctypes releases the GIL inside the calls.
        def stage_a(group):
            torch.cuda.set_device(dev)
            return stream_stage_a(self.rt, sa, group, kw, token_wgs, trace, dims=model_dims(self.cfg), samp=samp)

        def launch_bc(st):
            cur.wait_event(st.a_done)
            if st.refer is not None:
                st.refer.record_stream(cur)
            if st.ready is not None and st.voice is not None:        # (made on the caller's side stream, read here: see `ready`)
                for _, t in st.voice.members():
                    t.record_stream(cur)
            st.lat.record_stream(cur)
            if st.tr:
                st.tr["host_b0"] = time.perf_counter()
                st.tr["ev_b0"].record(cur)
            mel, lens_t = stage_b(self, st, sampler_id, eta, prec, sched=sched)
            wav, self.vocoder_done, self.vocoder_ticket = stage_c(self.rt, sc, cur, mel, st, lens_t, noise_scale, vocoder_chunk, tr=st.tr)
            return wav, [256 * t for t in lens_t], self.vocoder_done, self.vocoder_ticket, (mel, st, lens_t)

        def hand_out(out):
            """wait for this request's waveform; a saturated stage C is re-run on the exact fp32 kernels (this thread issues every stage-C
            launch, so the option flips between two of them; stage A on the other thread never reads it)"""
            out[2].synchronize()
            try:
                self.rt.vocoder_check(out[3])
            except Exception:
                if on_saturation == "raise":
                    raise
                self.saturated_requests += 1
                self.rt.set_option("voc_x3", 0)
                try:
                    wav, redo, _ = stage_c(self.rt, sc, cur, *out[4], noise_scale, vocoder_chunk, wait=False)
                finally:
                    self.rt.set_option("voc_x3", 1)
                redo.synchronize()
                return wav, out[1]
            return out[0], out[1]

        # requests -> stage-A groups: with pair_stage_a two consecutive requests of <= 8 utterances share a decode session.  Off by
        # default: a 16-row decode step costs 1.6x an 8-row one (161 vs 103 ms per 234 tokens alone), and under the three-stream
        # pipeline the longer chain measured 505 vs 482 ms per batch of 8 (bench.py, 10 steps).
        groups = group_requests(requests, bool(pair_stage_a))
        first = next(groups, None)
        if first is None:
            return
        if self._a_pool is None:
            self._a_pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="dtts-stage-a")
        fut = self._a_pool.submit(stage_a, first)
        pending = launched = None
        try:
            while fut is not None:
                sts, fut = fut.result(), None   # the only wait on the GPU: this group's codes (their lengths size stage B)
                g = next(groups, None)
                if g is not None:
                    fut = self._a_pool.submit(stage_a, g)            # the next group's stage A starts now, under this group's diffusion
                for st in sts:
                    out = launch_bc(st)         # stage B / C of this request: enqueued, not waited for
                    launched = out
                    if pending is not None:
                        yield hand_out(pending)                  # a saturated stage C concerns THIS request only (its waveform is complete now)
                    pending = out
            yield hand_out(pending)
        finally:
            # closed early or failed: the decode session in flight must end before this handle's stage-A entry points are used again
            if fut is not None:
                try:
                    fut.result()
                except Exception:
                    pass
            # ... and so must the abandoned request's vocoder (its own stream and scratch arena): a plain infer() right after would
            # otherwise run its stage C on the same arena under it
            if launched is not None:
                launched[2].synchronize()

    # ------------------------------------------------------------------------------------------------------------
    def infer_long(self, text, refer=None, refer_lengths=None, *, speaker=None, tokenizer=None, sentence_ids=None, clause_ids=(),
                   space_id=None, max_len=160, min_len=0, rows_per_call=8, seed=None, pauses_ms=None, trim_db=-40.0, keep_ms=20,
                   fade_ms=5, stream=False, return_chunks=False, forced_codes=None, max_generate_length=MAX_GENERATE_LENGTH, top_k=50,
                   suppress_eos=False, diffusion_steps=None, sampler="p", eta=0.0, trunk_precision=None, decode_options=None,
                   noise_scale=NOISE_SCALE, speed=None, sampling=None):
        """A text of any length in one voice -> one waveform [1,1,N] (longform.py; the reference has no long-form path).

        speed: one speaking rate in [0.25, 4] for every chunk (see infer; None or 1.0: today's path).  The join and the pauses are
        untouched; a chunk's dict then reports `frames` (its mel frames, samples // 256) and `codes` = None (the rate hides them).

        The text is cut into chunks at sentence ends (longform.split_units: a sentence of more than `max_len` units again after a
        clause mark, a space, or at max_len; sentences shorter than `min_len` merged), every chunk is a complete utterance - a row of
        infer(batch=True), through the stages exactly as they are - and each group of `rows_per_call` (1 .. 16) chunks goes through
        infer_stream as one request: group i + 1 decodes under group i's diffusion.  A group's waveforms are then joined on the device
        (csrc/wav_join.hip): every row cut to its loud span (frames of 256 samples whose RMS reaches `trim_db` dB re full scale, `keep_ms`
        kept around them; trim_db=None: nothing is cut), faded in and out linearly over `fade_ms`, and followed by pauses_ms[kind] of
        exact zeros, kind = how the chunk ended ("sentence", "clause", "word", "hard"; the text's last chunk, "end", has no pause;
        None: 400 / 200 / 60 / 0 ms).  A chunk that trimmed to nothing contributes no samples and keeps its pause.

        text: a pinyin string (split at 。！？!?. / ，,；;、：: / spaces; needs `tokenizer`, an object with .encode; a chunk is framed as the
        reference's api.py frames a text: " " + chunk + " ", encoded, one trailing 0), or a 1-D array of text ids (needs `sentence_ids`;
        `clause_ids` and `space_id` as the vocabulary has them; framed as [space_id] + ids + [space_id, 0], or ids + [0]).  A framed chunk
        of more than gpt.max_text_tokens ids is a ValueError naming its span.  The speaker: `speaker`, a Voice of S = 1, or a prompt mel
        `refer` [1,128,Tr] (+ refer_lengths), whose latents are computed ONCE (get_conditioning_latents) - both given, or neither:
        ValueError.  Every check is made before anything runs.

        Chunk k is row k % rows_per_call of request k // rows_per_call, every request carries the call's `seed` (None: drawn once) and
        chunk k has sample id k: a chunk's random streams do not depend on rows_per_call (its waveform is promised bit for bit only
        for the same grouping).  forced_codes: a list of one code array per chunk (tests, ragged benchmarks); such a call runs its groups
        as a loop of blocking infer(batch=True) calls and returns their bits - infer_stream decodes forced codes through the KV cache,
        which moves the last bits of the latents, and nothing is decoded that the next group could overlap
        (longform.group_waveforms).  Beams are refused as infer_stream refuses them; the remaining keywords are infer_stream's.

        stream=True: a generator of the groups' pieces [1,1,n_i], in order, each as its group completes - the first audio arrives after
        the first group.  stream=False: the same pieces concatenated (the same code, the same bits).  return_chunks: also one dict per
        chunk - with stream=True each piece comes with the dicts of its own chunks - of span (in the caller's text), kind, codes (the
        number of codes; max_generate_length - 1, the most a decode returns in front of its stop token, means the chunk ran into the limit
        and was cut short), samples (before trimming), begin,
        end, offset (in the whole output) and pause (samples).  The only host wait the call adds to infer_stream's is the read-back of
        a group's edges, when its waveform is being handed out anyway.

        The defaults - max_len, pauses, threshold, margin, fade - are the maintainer's choice and UNMEASURED: without a trained
        checkpoint nothing is known about seam and pause quality, the right trim level or the codes a chunk of max_len units needs."""
        from .. import longform
        sampling_args(diffusion_steps, sampler, eta)
        SynthesizerTrn._check_trunk_precision(self, trunk_precision)
        # sampling: None or ONE dict for every chunk (see infer), handed to the groups as it is; the per-row list is refused here
        if sampling is not None and not hasattr(sampling, "items"):
            raise ValueError("infer_long: `sampling` has to be None or a dict (the chunks are rows of one voice: one set of settings)")
        resolve_sampling(sampling, 1, top_k=top_k, max_generate_length=max_generate_length, decode_options=decode_options)
        plan = longform.prepare(self, text, refer, refer_lengths, speaker=speaker, tokenizer=tokenizer, sentence_ids=sentence_ids,
                                clause_ids=clause_ids, space_id=space_id, max_len=max_len, min_len=min_len, rows_per_call=rows_per_call,
                                seed=seed, pauses_ms=pauses_ms, trim_db=trim_db, keep_ms=keep_ms, fade_ms=fade_ms, forced_codes=forced_codes,
                                decode_options=decode_options, speed=speed)
        pieces = longform.run(self, plan, dict(noise_scale=noise_scale, max_generate_length=max_generate_length, top_k=top_k,
                                               suppress_eos=suppress_eos, diffusion_steps=diffusion_steps, sampler=sampler, eta=eta,
                                               trunk_precision=trunk_precision, decode_options=decode_options,
                                               **({} if sampling is None else dict(sampling=sampling))),
                             pipelined=forced_codes is None)
        if stream:
            return pieces if return_chunks else (p for p, _ in pieces)
        got = list(pieces)
        wav = torch.cat([p for p, _ in got], 2)
        return (wav, [c for _, cs in got for c in cs]) if return_chunks else wav

    def infer_many(self, utterances, *, rows_per_call=8, seed=None, sampling=None, max_generate_length=MAX_GENERATE_LENGTH, top_k=50,
                   suppress_eos=False, decode_options=None, diffusion_steps=None, sampler="p", eta=0.0, trunk_precision=None,
                   noise_scale=NOISE_SCALE, vocoder_chunk=0, on_saturation="rerun_fp32"):
        """Single utterances in, single waveforms out, batched in between (many.py): the entry a server calls.

        utterances: an iterable (a generator may be fed lazily: at most two requests are read ahead) of dicts with `text` (1-D ids);
        exactly one of `speaker` (a Voice of S = 1) and `refer` ([128, Tr] or [1, 128, Tr], optionally `refer_length`); optionally
        `sample_id` (default: the utterance's index), `sampling` (a dict, see infer; default: the call's `sampling`), `speed` and
        `forced_codes` (1-D; all rows of a request or none).  Yields (wav [1,1,n], n) per utterance, in input order, each request's
        rows as that request completes.

        Consecutive utterances form requests of rows_per_call rows (1 .. 16; the last may be short).  A prompt mel becomes a Voice once
        per distinct tensor object; each request carries speaker = Voice.cat(its rows' voices), the rows' own sampling settings - they
        decode in one session, each under its own (gpt/sampling.py) - the call's ONE seed (None: drawn once) and the sample ids, and goes
        through infer_stream as it is: request i + 1 decodes under request i's diffusion, and every row equals that row of the blocking
        infer(batch=True, speaker=Voice.cat(...), sampling=[...], seed=, sample_ids=[...]) on the same group, cut at its length.  All of
        a request's utterances are checked before it starts; the call's own arguments before anything starts.

        Batch-wide by construction: the diffusion schedule, sampler, trunk precision and noise_scale.  Out of scope: reordering by
        length, per-utterance seeds through stages B and C, cancellation."""
        from .. import many
        sampling_args(diffusion_steps, sampler, eta)
        SynthesizerTrn._check_trunk_precision(self, trunk_precision)
        return many.infer_many(self, utterances, rows_per_call=rows_per_call, seed=seed, sampling=sampling, noise_scale=noise_scale,
                               max_generate_length=max_generate_length, top_k=top_k, suppress_eos=suppress_eos, decode_options=decode_options,
                               diffusion_steps=diffusion_steps, sampler=sampler, eta=eta, trunk_precision=trunk_precision,
                               vocoder_chunk=vocoder_chunk, on_saturation=on_saturation)

    def join_group(self, wav, lens, kinds, plan, base=0, complete=True):
        """one group of infer_long: its waveform batch cut and joined on the device (longform.join_group) -> (piece [n], chunk dicts)"""
        from .. import longform
        return longform.join_group(self, wav, lens, kinds, plan, base, complete)

    EMPTY_CODE_FRAMES = 16

    def infer_gpt(self, text, text_length, refer, refer_lengths, noise_scale=NOISE_SCALE, *, batch=False, seed=None, sample_ids=None,
                  forced_codes=None, max_generate_length=MAX_GENERATE_LENGTH, top_k=50, suppress_eos=False, prompt_codes=None,
                  decode_options=None, speaker=None, return_alignment=False, align_options=None, sampling=None):
        """vqvae/model_24k.py:811-847: GPT codes -> quantizer.decode + vq_ref_enc -> vq_dec -> infer_flowvae (no diffusion).
        return_alignment / align_options: as in infer - (wav, alignment) with one dictionary per row; a row whose stop token came first
        has no codes and an empty path.
        prompt_codes (not with forced_codes): line 819 calls UnifiedVoice.inference_speech_valle, see infer.  decode_options: see infer.
        speaker: a Voice with a vq member in the place of (refer, refer_lengths), see infer: its gpt member conditions the decode, its vq
        member is g_vq."""
        check_prompt_args(prompt_codes, forced_codes, 1)
        processors, beam = beam_request(decode_options, forced_codes=forced_codes)
        st = normalize_request(text, text_length, refer, refer_lengths, seed, sample_ids, forced_codes, batch=batch, speaker=speaker,
                               dims=None if speaker is None else model_dims(self.cfg))
        if speaker is not None and speaker.vq is None:
            raise ValueError("infer_gpt: this Voice has no vq member (it was made by a model without VQ weights)")
        B, rl, seed, sample_ids = st.B, st.rl, st.seed, st.sids
        if sampling is not None and not batch and not hasattr(sampling, "items"):
            sampling = sampling[:1]
        rows = resolve_sampling(sampling, B, top_k=top_k, max_generate_length=max_generate_length, decode_options=processors,
                                num_beams=(beam or {}).get("num_beams"))      # per-row sampling settings, see infer
        check_forced_caps(rows, st.forced)
        pkw = {} if prompt_codes is None else dict(prompt_codes=prompt_rows(prompt_codes if batch else prompt_codes[:1], B))
        if processors:
            pkw["processors"] = processors
        if rows is not None:
            pkw["rows"] = rows
            max_generate_length = session_cap(rows, max_generate_length)
        g_vq = None
        if st.voice is not None:
            voice = st.voice.for_batch(B)
            refer, g_vq = None, voice.vq
            pkw["cond"] = voice.gpt
        else:
            refer = st.refer.to(self.device, torch.float32).contiguous()
        if st.forced is None and beam:
            seqs, blens, _ = self.rt.gpt_generate_beams(refer, rl, st.texts, num_return_sequences=1, max_generate_length=max_generate_length,
                                                        repetition_penalty=REPETITION_PENALTY, suppress_eos=suppress_eos, **pkw, **beam)
            code_list = [seqs[b, 0, : int(blens[b, 0]) - 1] for b in range(B)]
        elif st.forced is None:
            codes, ncodes, _ = self.rt.gpt_generate(refer, rl, st.texts, seed, sample_ids, max_generate_length=max_generate_length,
                                                    top_k=top_k, top_p=TOP_P, temperature=TEMPERATURE,
                                                    repetition_penalty=REPETITION_PENALTY, suppress_eos=suppress_eos, **pkw)
            code_list = [codes[b, : int(ncodes[b]) - 1] for b in range(B)]          # codes[:, :-1]  (:828)
        else:
            code_list = [np.asarray(c) for c in st.forced]
        # vqvae/model_24k.py:833-834: the stop token came first -> the reference decodes a ZERO latent of 16 frames (64 mel frames);
        # code -1 is that zero vector in dtts_vq_decode
        out_codes = code_list
        code_list = [c if len(c) else np.full(self.EMPTY_CODE_FRAMES, -1, np.int64) for c in code_list]
        mel = self.rt.vq_decode(code_list, refer, rl, g_vq=g_vq)
        lens_t = [4 * len(c) for c in code_list]
        wav = self.rt.vocoder(mel, seed, sample_ids, lens=lens_t, noise_scale=noise_scale)
        if not return_alignment:
            return wav
        return wav, self._alignment_of(st.texts, out_codes, refer, rl, pkw.get("cond"), **(align_options or {}))

    def _alignment_of(self, texts, code_list, refer, rl, cond, layers=None, head_weights=None, space_id=None, plan=None):
        """one teacher-forced pass with the attention read-out over (texts, code_list), the path kernel, then the host bookkeeping of
        gpt/alignment.py -> a list of per-row dictionaries (describe).  Waits for its own results (the path comes to the host).
        plan: the FramePlan stage B ran under (duration.py) - every time then follows its frame -> code map."""
        from ..gpt.alignment import describe
        rows = [np.asarray(c, np.int32).reshape(-1) for c in code_list]
        spc, sr = self.cfg["gpt"]["mel_length_compression"], self.cfg["data"]["sampling_rate"]
        if max(len(c) for c in rows) == 0:          # nothing was spoken in any row: no pass to run, every path is empty
            return [describe([], 0, t, None, spc, sr, space_id) for t in texts]
        attn, mass = self.rt.gpt_text_alignment(refer, rl, texts, rows, layers=layers, head_weights=head_weights, cond=cond)
        path = self.rt.op_monotone_path(torch.log(attn.clamp_min(1e-12)), [len(c) for c in rows], [len(t) + 2 for t in texts])
        path, mass = path.cpu().numpy(), mass.cpu().numpy()
        bounds = [None if plan is None else plan.code_bounds(b) for b in range(len(rows))]
        return [describe(path[b], len(rows[b]), texts[b], mass[b], spc, sr, space_id, frame_bounds=bounds[b]) for b in range(len(rows))]

    def align(self, text, text_length, codes, code_lengths=None, refer=None, refer_lengths=None, *, speaker=None, layers=None,
              head_weights=None, space_id=None):
        """When did the model speak what: the alignment of mel codes (infer's, encode()'s, anyone's) to the text, from the GPT's
        text-audio attention.  text [B, Lt] / text_length [B] as in infer (every row counts: there is no `batch` switch); codes [B, n]
        with code_lengths [B], or a list of B one-dimensional rows, WITHOUT a stop token; refer / refer_lengths or speaker= under
        infer's rules (both or neither: ValueError before any launch).  Returns one dictionary per row (gpt/alignment.py describe):
          path        int32 [n]: the text column of every code; columns are those of [255, text ..., 0], so column 1 + k is text id k
          spans/times per column (first, last) code and (start, end) seconds, None for a column without a code;
          token_spans / token_times the same per text id; words (with space_id, the tokenizer's [SPACE] id) the ids between spaces merged
          stats       coverage, skipped (text ids without a code), longest_stay, mean_text_mass - a decode that skipped or repeated
                      text shows here.
        Code j covers samples [1024 j, 1024 (j + 1)) (gpt.mel_length_compression at data.sampling_rate).  One teacher-forced pass with
        one more kernel per selected layer, then the path kernel.  layers / head_weights [len(layers), 16]: which maps count (default:
        the uniform mean over all 10 x 16 - which heads carry the alignment of a trained checkpoint is unknown here, and alignment
        quality is unmeasured)."""
        text = torch.as_tensor(text)
        B = text.shape[0]
        st = normalize_request(text, text_length, refer, refer_lengths, 0, None, None, batch=True, speaker=speaker,
                               dims=None if speaker is None else model_dims(self.cfg))
        if isinstance(codes, (list, tuple)):
            rows = [np.asarray(torch.as_tensor(c).cpu().numpy(), np.int32).reshape(-1) for c in codes]
        else:
            c = torch.as_tensor(codes).cpu().numpy().astype(np.int32)
            cl = [c.shape[1]] * c.shape[0] if code_lengths is None else [int(v) for v in torch.as_tensor(code_lengths).reshape(-1).tolist()]
            rows = [c[b, : cl[b]] for b in range(c.shape[0])]
        if len(rows) != B:
            raise ValueError(f"align: {len(rows)} code rows for {B} texts")
        if st.voice is not None:
            refer, cond = None, st.voice.for_batch(B).gpt
        else:
            refer, cond = st.refer.to(self.device, torch.float32).contiguous(), None
        return self._alignment_of(st.texts, rows, refer, st.rl, cond, layers, head_weights, space_id)

    def encode(self, y, y_lengths=None):
        """vqvae/model_24k.py:877-880 -> (codes [B, T/4] int64, x_vq [B,768,T/4])"""
        y = torch.as_tensor(y).to(self.device, torch.float32).contiguous()
        lens = None if y_lengths is None else [int(v) for v in torch.as_tensor(y_lengths).reshape(-1).tolist()]
        codes, xvq = self.rt.vq_encode(y, lens)
        return codes.long(), xvq

    def forward_gpt(self, y, y_lengths, data):
        """vqvae/model_24k.py:697-704, the GPT stage's validation loss: codes of data['raw_mel'] (encode), then UnifiedVoice.forward's
        loss mode on (data['mel'], data['spec_length'], data['text'], data['text_length'], codes, data['raw_wav_length']) ->
        loss_text * train.text_weight + loss_mel * train.mel_weight, a 0-d fp32 CUDA tensor.  No mel logits are materialised.
        Needs gpt.text_head in the checkpoint.  y / y_lengths are unused, as in the reference."""
        code, _ = self.encode(data["raw_mel"], data["raw_spec_length"])
        mel = torch.as_tensor(data["mel"]).to(self.device, torch.float32).contiguous()
        loss_text, loss_mel, _ = self.gpt(mel, data["spec_length"], data["text"], data["text_length"], code, data["raw_wav_length"],
                                          return_logits=False)
        return loss_text * self.text_loss_weight + loss_mel * self.mel_loss_weight

    def forward_diff(self, y, y_lengths, data, *, t=None, noise=None, seed=0):
        """vqvae/model_24k.py:667-696, the diffusion stage's validation loss -> a 0-d fp32 CUDA tensor.  eval() semantics, no gradients
        (unconditioned_percentage and layer_drop are training branches).  x_start = normalize_torch_mel(data['raw_mel']); codes of
        data['raw_mel'] (encode); GPT latents of (raw_mel, raw_spec_length, text, text_length, codes, raw_wav_length) with
        return_latent=True, clip_inputs=False; conditioning_latent = get_conditioning(y); diffuser.training_losses on the 200-step
        schedule; the mean of the rows' losses, added in row order.  y_lengths is unused, as in the reference.

        t [B] (integers in [0, 200), checked on the host) and noise [B,128,T] default to host-drawn timesteps (draw_timesteps(seed, B))
        and Philox noise keyed by (seed, row): neither can equal torch's RNG, so a caller who wants the reference's numbers passes
        both.  The reference's GPT forward here is a rectangle without an attention mask while this one is ragged (text_length,
        raw_wav_length): the two agree when every row has the full text width and a full-length raw_wav_length."""
        raw_mel = torch.as_tensor(data["raw_mel"]).to(self.device, torch.float32).contiguous()
        B = raw_mel.shape[0]
        ts = draw_timesteps(seed, B, self.desired_diffusion_steps) if t is None else check_timesteps(t, B, self.diffuser.num_timesteps)
        if self.rt.get_option("trunk_fp16"):
            raise NotImplementedError("forward_diff runs the three-product trunk only: switch the fp16 trunk mode off for this call "
                                      "(diffusion.enable_fp16 = False)")
        if noise is not None:
            noise = torch.as_tensor(noise).to(self.device, torch.float32).contiguous()
        code, _ = self.encode(raw_mel, data["raw_spec_length"])
        aligned = self.gpt(raw_mel, data["raw_spec_length"], data["text"], data["text_length"], code, data["raw_wav_length"],
                           return_latent=True, clip_inputs=False)
        cond = self.diffusion.get_conditioning(torch.as_tensor(y).to(self.device, torch.float32))
        sched = self.rt.diff_schedule(self.diffuser.timestep_map)
        x_start, _, noise = self.rt.diff_q_sample(sched, raw_mel, ts, noise=noise, seed=seed, normalize=True)
        losses = self.diffuser.training_losses(self.diffusion, x_start, ts, noise=noise,
                                               model_kwargs={"aligned_conditioning": aligned, "conditioning_latent": cond})["loss"]
        total = losses[0]
        for b in range(1, B):                                      # .mean() over the rows in a fixed order
            total = total + losses[b]
        return total / B

    def diffusion_bpd(self, y, y_lengths, data, *, noise=None, seed=0, rows_per_pass=0):
        """The diffusion decoder's variational bound in bits per dimension on one validation batch: forward_diff's preparation
        (x_start = normalize_torch_mel(data['raw_mel']), encode, the GPT latents with return_latent=True, clip_inputs=False,
        conditioning_latent = get_conditioning(y)), then diffuser.calc_bpd_loop (vqvae/utils/diffusion.py:1114-1169) on the 200-step
        schedule -> its dict: total_bpd, prior_bpd [B]; vb, xstart_mse, mse [B, 200] (column j = timestep 199 - j), fp32 CUDA.
        noise [200, B, 128, T] indexed by timestep, or None: Philox noise keyed by (seed, row, timestep).  y_lengths is unused, as in
        forward_diff.  The unguided model's likelihood: self.diffuser is built with conditioning_free=False."""
        raw_mel = torch.as_tensor(data["raw_mel"]).to(self.device, torch.float32).contiguous()
        if self.rt.get_option("trunk_fp16"):
            raise NotImplementedError("diffusion_bpd runs the three-product trunk only: switch the fp16 trunk mode off for this call "
                                      "(diffusion.enable_fp16 = False)")
        if noise is not None:
            noise = torch.as_tensor(noise).to(self.device, torch.float32).contiguous()
        code, _ = self.encode(raw_mel, data["raw_spec_length"])
        aligned = self.gpt(raw_mel, data["raw_spec_length"], data["text"], data["text_length"], code, data["raw_wav_length"],
                           return_latent=True, clip_inputs=False)
        cond = self.diffusion.get_conditioning(torch.as_tensor(y).to(self.device, torch.float32))
        sched = self.rt.diff_schedule(self.diffuser.timestep_map)
        # forward_diff's normalisation kernel (the x_t it also forms, at t = 0 with raw_mel standing in for the noise, is dropped)
        x_start, _, _ = self.rt.diff_q_sample(sched, raw_mel, [0] * raw_mel.shape[0], noise=raw_mel, normalize=True)
        return self.diffuser.calc_bpd_loop(self.diffusion, x_start, noise=noise, seed=seed, rows_per_pass=rows_per_pass,
                                           model_kwargs={"aligned_conditioning": aligned, "conditioning_latent": cond})

    def sampling_diffuser(self, diffusion_steps=None):
        """the guided DDIM diffuser of `diffusion_steps` (None: 50) steps - the schedule and guidance infer(sampler="ddim") samples on"""
        key, _, _ = sampling_args(diffusion_steps, "ddim")
        d = SpacedDiffusion(key, betas=get_named_beta_schedule("linear", TRAINED_DIFFUSION_STEPS), conditioning_free=True,
                            conditioning_free_k=COND_FREE_K, sampler="ddim")
        d.rt = self.rt
        return d

    def get_conditioning_latents(self, refer, refer_lengths=None, *, clip_lengths=None):
        """The speaker of a prompt as a Voice (voice.py): the outputs of gpt.conditioning_encoder, diffusion.contextual_embedder and
        vq_ref_enc, computed once and handed to infer / infer_gpt / infer_stream / invert_mel / resynthesize as speaker=.
        refer [S,128,T] (one clip per speaker; refer_lengths [S]) or [S,n,128,T] (n clips per speaker, pooled as the reference's two
        get_conditioning pool them); clip_lengths [S,n] gives every clip its own valid length (an extension, as lengths are elsewhere)."""
        checked = check_clips(refer, refer_lengths, clip_lengths)      # (ValueError before any device work)
        return make_voice(self.rt, refer, *checked)

    def _code_embedding(self, codes, text, text_length, refer, refer_lengths, speaker=None):
        """infer's conditioning of the diffusion (vqvae/model_24k.py:796-803) for given codes [B, n] -> code embedding [B,768,4n]"""
        check_speaker(speaker, refer, refer_lengths, codes.shape[0], None if speaker is None else model_dims(self.cfg))
        n = codes.shape[-1]
        wav_len = torch.tensor([n * 1024] * codes.shape[0])                   # codes.shape[-1] * mel_length_compression (:798)
        if speaker is not None:
            voice = speaker.for_batch(codes.shape[0])
            latent = self.gpt(None, None, text, text_length, codes, wav_len, return_latent=True, clip_inputs=False, cond_latents=voice.gpt)
            return self.diffusion.timestep_independent(latent, voice.diffusion, 4 * n)
        refer = torch.as_tensor(refer).to(self.device, torch.float32).contiguous()
        latent = self.gpt(refer, refer_lengths, text, text_length, codes, wav_len, return_latent=True, clip_inputs=False)
        cond = self.diffusion.get_conditioning(refer)
        return self.diffusion.timestep_independent(latent, cond, 4 * n)

    def invert_mel(self, mel, mel_lengths, text, text_length, refer=None, refer_lengths=None, *, diffusion_steps=None, depth=None,
                   speaker=None):
        """DDIM inversion of an existing mel under (text, refer): the noise-level-`depth` x that the guided DDIM sampler of
        `diffusion_steps` renders back from.  mel: a raw log-mel [B,128,T], T % 4 == 0 (ValueError otherwise).  forward_diff's
        preparation - normalize_torch_mel, encode, the GPT latents of (refer, text, codes) with return_latent=True, clip_inputs=False
        and the wav length (T / 4) * 1024 as in infer, get_conditioning(refer), timestep_independent - then
        ddim_reverse_sample_loop on sampling_diffuser(diffusion_steps) to `depth` (None: all steps).
        -> dict(x [B,128,T], depth, diffusion_steps, codes [B, T/4], emb [B,768,T]); feed it to resynthesize.

        The round trip is NOT the identity: guidance and the clamp of pred_xstart are not invertible.  On the test weights the
        reference's own inversion + DDIM (eta = 0, 10 steps) misses its input by 0.88 max-abs (normalised mel) from depth 5 and by
        1.37 from depth 9.  Audio under a trained checkpoint is unmeasured.  speaker: a Voice in the place of (refer, refer_lengths)."""
        check_speaker(speaker, refer, refer_lengths, torch.as_tensor(mel).shape[0], None if speaker is None else model_dims(self.cfg))
        mel = torch.as_tensor(mel).to(self.device, torch.float32).contiguous()
        if mel.dim() != 3 or mel.shape[-1] % 4 != 0:
            raise ValueError(f"mel must be [B,128,T] with T a multiple of 4 (the codes' hop), not shape {tuple(mel.shape)}")
        d = self.sampling_diffuser(diffusion_steps)
        depth, _ = d.invert_depth(depth)
        codes, _ = self.encode(mel, mel_lengths)
        emb = self._code_embedding(codes, text, text_length, refer, refer_lengths, speaker)
        x = d.ddim_reverse_sample_loop(self.diffusion, normalize_torch_mel(mel), {"precomputed_aligned_embeddings": emb}, depth=depth)
        return dict(x=x, depth=depth, diffusion_steps=d.num_timesteps, codes=codes, emb=emb)

    def resynthesize(self, inv, text, text_length, *, refer=None, refer_lengths=None, eta=0.0, vocode=True, seed=0, sample_ids=None,
                     noise_scale=NOISE_SCALE, speaker=None):
        """Render an inversion (invert_mel's dict) again: ddim_sample_loop from t_start = inv['depth'] on the same diffuser (a full loop
        with noise = x when depth == diffusion_steps), de-normalised -> mel [B,128,T] (vocode=False) or (wav, mel) through
        infer_flowvae.  refer given: the code embedding is rebuilt from inv['codes'] under THAT prompt (its GPT latents and
        get_conditioning), so the mel is rendered in another voice; else inv['emb'] is reused and text / text_length are not read.
        eta > 0 draws Philox noise keyed by (seed, sample_ids).  Not the identity, and unmeasured on a trained checkpoint: see
        invert_mel.  speaker: a Voice in the place of refer (both: ValueError)."""
        if speaker is not None:
            check_speaker(speaker, refer, refer_lengths, inv["codes"].shape[0], model_dims(self.cfg))
        d = self.sampling_diffuser(inv["diffusion_steps"])
        depth, t_start = d.invert_depth(inv["depth"])
        emb = inv["emb"] if refer is None and speaker is None else self._code_embedding(inv["codes"], text, text_length, refer, refer_lengths,
                                                                                        speaker)
        x = inv["x"]
        norm = d.ddim_sample_loop(self.diffusion, tuple(x.shape), noise=x, model_kwargs={"precomputed_aligned_embeddings": emb}, eta=eta,
                                  seed=seed, sample_ids=sample_ids, t_start=t_start)
        mel = denormalize_torch_mel(norm)
        if not vocode:
            return mel
        B, T = mel.shape[0], mel.shape[-1]
        return self.infer_flowvae(mel, [T] * B, None, noise_scale, batch=True, seed=seed, sample_ids=sample_ids), mel

    def inpaint_mel(self, mel, mel_lengths, text, text_length, refer=None, refer_lengths=None, *, spans=None, keep=None, codes=None,
                    diffusion_steps=None, sampler="ddim", eta=0.0, resample=1, t_start=None, seed=0, sample_ids=None, vocode=True,
                    noise_scale=NOISE_SCALE, speaker=None):
        """Render a stretch of an existing utterance again and leave the rest untouched (RePaint, Lugmayr et al. 2022, on the diffusion
        decoder).  mel: a raw log-mel [B,128,T], T % 4 == 0.  Exactly one of
          spans  per row a list of inclusive code spans (first, last) - what align / return_alignment hand out under "spans",
                 "token_spans" and each word's "span" (None entries are skipped); frames 4 first .. 4 last + 3 are regenerated
          keep   a bool frame mask [B,T] (or [T] for all rows), False where the mel is to be regenerated.
        codes [B, T/4]: what the result is to speak (None: encode(mel), the same content in a fresh rendering; another length:
        splice_codes).  The code embedding is _code_embedding(codes, text, ...) over the WHOLE sequence, known =
        normalize_torch_mel(mel), and the sampling loop of `diffusion_steps` (sampler "ddim" with eta, or "p") runs with known= / keep=
        / resample= (SpacedDiffusion.p_sample_loop): after every step the kept frames are overwritten with the known mel noised to
        that level, so the new frames are generated in the context of the old ones at every noise level; resample = U in [1, 32]
        repeats every step U times so that the seam harmonises (U times the cost).  t_start = s starts from q_sample(known, s) (Philox
        stage 5, keyed by seed / sample_ids) in the place of pure noise and keeps the span's coarse shape.
        -> mel' [B,128,T] (vocode=False) or (wav, mel') through infer_flowvae, as resynthesize.  The kept frames of mel' are the
        caller's mel BITS (torch.where on the caller's tensor, no normalise / de-normalise round trip); the values of mel inside the
        regenerated frames are read only by encode (codes=None) and by q_sample (t_start).

        ValueError before any launch: T % 4 != 0; both or neither of spans / keep; a mask of another shape or dtype; a span outside
        [0, T/4), reversed or overlapping; every frame kept (nothing to do); resample not an int in [1, 32]; sampler "dpmsolver++" (a
        multistep history does not survive the overwrite); eta < 0; codes of another length; t_start outside the schedule.  Nothing
        kept with t_start=None is allowed: it is the plain sampling loop under these codes.  speaker: a Voice in the place of (refer,
        refer_lengths).  Audio and seam quality under a trained checkpoint are unmeasured."""
        shape = tuple(torch.as_tensor(mel).shape)
        key, _, eta = sampling_args(diffusion_steps, sampler, eta)
        kmask = check_inpaint_args(shape, spans, keep, codes, resample, sampler, eta, t_start, len(key) if isinstance(key, list) else key)
        check_speaker(speaker, refer, refer_lengths, shape[0], None if speaker is None else model_dims(self.cfg))
        mel = torch.as_tensor(mel).to(self.device, torch.float32).contiguous()
        B, _, T = shape
        if codes is None:
            codes, _ = self.encode(mel, mel_lengths)
        else:
            codes = torch.as_tensor(codes).to(self.device).long()
        emb = self._code_embedding(codes, text, text_length, refer, refer_lengths, speaker)
        d = SpacedDiffusion(key, betas=get_named_beta_schedule("linear", TRAINED_DIFFUSION_STEPS), conditioning_free=True,
                            conditioning_free_k=COND_FREE_K, sampler=sampler)
        d.rt = self.rt
        known = normalize_torch_mel(mel).contiguous()
        ids = list(range(B)) if sample_ids is None else list(sample_ids)
        noise = None
        if t_start is not None:
            noise = d.q_sample(known, [int(t_start)] * B, seed=seed, sample_ids=ids)[0]
        kdev = kmask.to(self.device)
        args = dict(noise=noise, model_kwargs={"precomputed_aligned_embeddings": emb}, seed=seed, sample_ids=ids, t_start=t_start,
                    known=known, keep=kdev, resample=int(resample))
        if sampler == "ddim":
            args["eta"] = eta
        norm = (d.ddim_sample_loop if sampler == "ddim" else d.p_sample_loop)(self.diffusion, (B, 128, T), **args)
        out = torch.where(kdev[:, None, :], mel, denormalize_torch_mel(norm))
        if not vocode:
            return out
        return self.infer_flowvae(out, [T] * B, None, noise_scale, batch=True, seed=seed, sample_ids=sample_ids), out

    def forward_vq(self, y, y_lengths, data=None):
        """vqvae/model_24k.py:654-666, the VQ stage's validation loss -> a 0-d fp32 CUDA tensor: L1(vq_dec(quantizer(vq_enc(y)) +
        vq_ref_enc(y * mask, mask)), y), the mean over the whole [B,128,T] rectangle.  In eval mode the reference quantizer's commit
        loss is the constant 0 (vqvae/modules/core_vq.py:311-319), so the reconstruction loss is the whole of it."""
        y = torch.as_tensor(y)
        if y.shape[-1] % 4 != 0:
            raise ValueError(f"forward_vq needs a frame count divisible by 4 (the reference asserts it), not {y.shape[-1]}")
        y = y.to(self.device, torch.float32).contiguous()
        yl = [int(v) for v in torch.as_tensor(y_lengths).reshape(-1).tolist()]
        codes, _ = self.rt.vq_encode(y)                            # vq_enc sees the whole rectangle (:659)
        codes = codes.cpu().numpy()
        recon = self.rt.vq_decode([codes[b] for b in range(y.shape[0])], y, yl)      # vq_ref_enc(y * mask, mask): lengths y_lengths
        return self.rt.l1_mean(recon, y)

    def forward_flowvae(self, y, y_lengths, data, *, noise=None, ids_slice=None, seed=0, sample_ids=None):
        """vqvae/model_24k.py:706-737, the flow-VAE stage forward in eval mode, no gradients -> the reference's 8-tuple
        (o [B,1,seg*hop], 0, 0, 0, ids_slice int64 [B], y_mask [B,1,T], (z, z_p, m_p, logs_p, m_q, logs_q) [B,192,T] each, quantized
        [B,192,T] = enc_p's first output), CUDA tensors.  seg = train.segment_size // data.hop_length (40); data['spec'] is the linear
        spectrogram [B, filter_length // 2 + 1, T].  One device call (dtts_flowvae_forward): ref_enc, enc_p, enc_q, the forward flow,
        the segment gather and the generator.  Needs enc_q in the checkpoint.  A ragged batch is read as the reference reads its padded
        rectangle (ref_enc's spectral / temporal layers and in_proj see the padded frames before the mask applies), not row by row
        as the inference entries do.

        ValueError (before any launch) when T % 4 != 0 (the reference asserts it) or a row is shorter than seg (the reference would
        slice garbage there).  noise [B,192,T] is enc_q's eps (None: Philox stage 6 keyed (seed, sample_ids[b])); ids_slice [B] the
        segment starts (None: drawn on the host from `seed`, draw_segment_starts).  Neither draw can equal torch's RNG, so a caller
        who wants the reference's numbers passes both noise and ids_slice.  loss_mel and the discriminator losses of the reference's
        training loop are not part of this call."""
        y = torch.as_tensor(y)
        seg = self.cfg["train"]["segment_size"] // self.cfg["data"]["hop_length"]
        yl, ids = check_flowvae_args(y.shape, y_lengths, seg, ids_slice)
        if ids is None:
            ids = draw_segment_starts(seed, yl, seg)
        y = y.to(self.device, torch.float32).contiguous()
        spec = torch.as_tensor(data["spec"]).to(self.device, torch.float32).contiguous()
        if noise is not None:
            noise = torch.as_tensor(noise).to(self.device, torch.float32).contiguous()
        r = self.rt.flowvae_forward(y, spec, yl, ids, seg, noise=noise, seed=seed, sample_ids=sample_ids)
        ticket = self.rt.vocoder_ticket()
        if self.rt.vocoder_check_active():                         # the WaveNets' and the generator's split-precision planes
            torch.cuda.current_stream(self.device).synchronize()
            self.rt.vocoder_check(ticket)
        T = y.shape[-1]
        y_mask = (torch.arange(T, device=self.device)[None, :] < torch.as_tensor(yl, device=self.device)[:, None]).unsqueeze(1).to(torch.float32)
        return (r["o"], 0, 0, 0, torch.as_tensor(ids, dtype=torch.int64, device=self.device), y_mask,
                (r["z"], r["z_p"], r["m_p"], r["logs_p"], r["m_q"], r["logs_q"]), r["quantized"])

    def flowvae_stage_losses(self, y, y_lengths, data, disc, *, noise=None, ids_slice=None, seed=0, sample_ids=None):
        """Everything train.py:259-322 logs for target == 'flowvae', in one device call (dtts_flowvae_stage_losses), forward values only:
        forward_flowvae (same arguments, same bits), y = slice(data['wav'], ids_slice * hop, segment_size), y_mel =
        slice(spec_to_mel(data['spec']), ids_slice, segment_size // hop), y_hat_mel = mel_spectrogram(o), loss_mel = 45 L1, `disc`
        (a MultiPeriodDiscriminator bound to THIS model: MultiPeriodDiscriminator(state, model=self)) on (y, o) and the three GAN losses.
        -> dict: loss_gen, loss_fm, loss_mel, loss_kl, loss_disc, loss_gen_all (= loss_gen + loss_fm + loss_mel + loss_kl; this stage
        contributes zeros for the others) as 0-d fp32 CUDA tensors, losses_disc_r / losses_disc_g / losses_gen (lists of 6 such
        scalars) and `outputs`, forward_flowvae's tuple.  data['wav'] [B,1,>= T hop] is the waveform the spectrograms were made of
        (train.py's data['wav'])."""
        if getattr(disc, "rt", None) is not self.rt:
            raise ValueError("flowvae_stage_losses: disc must be a MultiPeriodDiscriminator bound to this model (MultiPeriodDiscriminator(state, model=model))")
        y = torch.as_tensor(y)
        seg = self.cfg["train"]["segment_size"] // self.cfg["data"]["hop_length"]
        yl, ids = check_flowvae_args(y.shape, y_lengths, seg, ids_slice)
        if ids is None:
            ids = draw_segment_starts(seed, yl, seg)
        y = y.to(self.device, torch.float32).contiguous()
        spec = torch.as_tensor(data["spec"]).to(self.device, torch.float32).contiguous()
        wav = torch.as_tensor(data["wav"])
        if wav.dim() != 3 or wav.shape[0] != y.shape[0] or wav.shape[1] != 1:
            raise ValueError(f"flowvae_stage_losses: data['wav'] must be [B, 1, samples], not {list(wav.shape)}")
        wav = wav.to(self.device, torch.float32).contiguous()
        if noise is not None:
            noise = torch.as_tensor(noise).to(self.device, torch.float32).contiguous()
        r = self.rt.flowvae_stage_losses(y, spec, yl, ids, seg, wav, noise=noise, seed=seed, sample_ids=sample_ids)
        ticket = self.rt.vocoder_ticket()
        if self.rt.vocoder_check_active():
            torch.cuda.current_stream(self.device).synchronize()
            self.rt.vocoder_check(ticket)
        T = y.shape[-1]
        y_mask = (torch.arange(T, device=self.device)[None, :] < torch.as_tensor(yl, device=self.device)[:, None]).unsqueeze(1).to(torch.float32)
        L, o = r["losses"], _lib_slots
        out = {k: L[i] for k, i in (("loss_gen", o.DISC_LOSS_GEN), ("loss_fm", o.DISC_LOSS_FM), ("loss_mel", o.DISC_LOSS_MEL),
                                    ("loss_kl", o.DISC_LOSS_KL), ("loss_disc", o.DISC_LOSS_DISC), ("loss_gen_all", o.DISC_LOSS_GEN_ALL))}
        for k, i in (("losses_disc_r", o.DISC_LOSSES_R), ("losses_disc_g", o.DISC_LOSSES_G), ("losses_gen", o.DISC_LOSSES_GEN)):
            out[k] = [L[i + d] for d in range(o.DISC_COUNT)]
        out["outputs"] = (r["o"], 0, 0, 0, torch.as_tensor(ids, dtype=torch.int64, device=self.device), y_mask,
                          (r["z"], r["z_p"], r["m_p"], r["logs_p"], r["m_q"], r["logs_q"]), r["quantized"])
        return out

    def forward_all(self, y, y_lengths, data, *, noise=None, ids_slice=None, seed=0, sample_ids=None, t=None, diff_noise=None):
        """vqvae/model_24k.py:749-772: forward_flowvae's tuple with l_diff, loss_gpt and vq_loss from forward_diff (t, diff_noise, seed),
        forward_gpt and forward_vq, each called as it would be alone"""
        o, _, _, _, ids, y_mask, latents, quantized = self.forward_flowvae(y, y_lengths, data, noise=noise, ids_slice=ids_slice, seed=seed,
                                                                           sample_ids=sample_ids)
        l_diff = self.forward_diff(y, y_lengths, data, t=t, noise=diff_noise, seed=seed)
        loss_gpt = self.forward_gpt(y, y_lengths, data)
        vq_loss = self.forward_vq(y, y_lengths, data)
        return o, l_diff, loss_gpt, vq_loss, ids, y_mask, latents, quantized

    def kl_loss(self, z_p, logs_q, m_p, logs_p, z_mask):
        """vqvae/modules/losses.py:43-58 -> a 0-d fp32 CUDA tensor: sum((logs_p - logs_q - 1/2 + 1/2 (z_p - m_p)^2 exp(-2 logs_p)) * z_mask)
        / sum(z_mask) on the device (dtts_kl_loss; two calls give the same bits).  z_mask [B,1,T] must be a sequence mask (ones up to
        each row's length, then zeros), which is what forward_flowvae returns: it is read back to the host as lengths."""
        ts = [torch.as_tensor(a).to(self.device, torch.float32).contiguous() for a in (z_p, logs_q, m_p, logs_p)]
        B, _, T = ts[0].shape
        m = torch.as_tensor(z_mask).to(self.device).reshape(B, T) != 0
        lens = m.sum(1)
        if not torch.equal(m, torch.arange(T, device=self.device)[None, :] < lens[:, None]):
            raise ValueError("kl_loss: z_mask must be a sequence mask (ones up to each row's length, then zeros)")
        return self.rt.kl_loss(*ts, [int(v) for v in lens.tolist()])

    def forward(self, y, y_lengths, data):
        """vqvae/model_24k.py:740-751: the stage loss cfg['train']['target'] names - 'vqvae' -> forward_vq, 'gpt' -> forward_gpt,
        'diff' -> forward_diff.  'flowvae' and the default (all stages) are NOT dispatched: forward_flowvae / forward_all exist and are
        called by name, but this dispatch and its NotImplementedError naming enc_q are pinned as they were."""
        name = FORWARD_TARGETS.get(self.target)
        if name is None:
            raise NotImplementedError(f"forward for train.target = {self.target!r} needs enc_q (the posterior encoder) and a forward-direction "
                                      "flow, which are not implemented on the device; targets 'vqvae', 'gpt' and 'diff' are")
        return getattr(self, name)(y, y_lengths, data)

    __call__ = forward

    def infer_vqvae(self, y, noise_scale=NOISE_SCALE, *, seed=0, sample_ids=None):
        """vqvae/model_24k.py:864-876: mel -> codes -> quantised latent + vq_ref_enc -> vq_dec -> (recon, wav); first row only"""
        y = torch.as_tensor(y)[:1].to(self.device, torch.float32).contiguous()
        assert y.shape[-1] % 4 == 0
        codes, _ = self.rt.vq_encode(y)
        recon = self.rt.vq_decode([codes[0].cpu().numpy()], y, [y.shape[-1]])
        sample_ids = [0] if sample_ids is None else list(sample_ids)
        return recon, self.rt.vocoder(recon, seed, sample_ids, lens=[y.shape[-1]], noise_scale=noise_scale)

    def infer_flowvae(self, y, y_lengths, data=None, noise_scale=NOISE_SCALE, *, batch=False, seed=0, sample_ids=None):
        """vqvae/model_24k.py:848-863"""
        y = torch.as_tensor(y)
        yl = [int(v) for v in torch.as_tensor(y_lengths).reshape(-1).tolist()]
        if not batch:
            y, yl = y[:1], yl[:1]
        assert y.shape[-1] % 4 == 0
        y = y.to(self.device, torch.float32).contiguous()
        sample_ids = list(range(y.shape[0])) if sample_ids is None else list(sample_ids)
        return self.rt.vocoder(y, seed, sample_ids, lens=yl, noise_scale=noise_scale)
