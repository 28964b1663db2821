"""Sampler object mirroring the subset of the reference's SpacedDiffusion that inference and evaluation use
(vqvae/utils/diffusion.py:179-228 + 1172-1272; p_sample_loop :654-742, ddim_sample_loop :819-899, k_diffusion_sample_loop :487-581,
sample_loop :640-652; q_sample :243-260, training_losses :930-1012; calc_bpd_loop :1114-1169, _vb_terms_bpd :903-928, _prior_bpd
:1098-1112; p_mean_variance :284-386, p_sample :445-485, ddim_sample :744-783, ddim_reverse_sample :785-817 and the progressive
loops).  The arithmetic lives in libdetail_hip.so (dtts_diff_sample_ex, dtts_diff_sample_from, dtts_diff_invert, dtts_diff_step,
dtts_diff_q_sample, dtts_diff_training_losses, dtts_diff_calc_bpd); this class carries the schedule constants and the call surface."""
from __future__ import annotations

import numpy as np

SAMPLERS = {"p": 0, "ddim": 1, "dpmsolver++": 2}


def space_timesteps(num_timesteps, section_counts):
    """vqvae/utils/diffusion.py:1223-1272: an int, a list of ints, or the string forms "25", "10,15" and "ddim25"."""
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            desired_count = int(section_counts[len("ddim"):])
            for i in range(1, num_timesteps):
                if len(range(0, num_timesteps, i)) == desired_count:
                    return set(range(0, num_timesteps, i))
            raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")
        section_counts = [int(x) for x in section_counts.split(",")]
    if isinstance(section_counts, int):
        section_counts = [section_counts]
    size_per, extra = num_timesteps // len(section_counts), num_timesteps % len(section_counts)
    start, out = 0, []
    for i, count in enumerate(section_counts):
        size = size_per + (1 if i < extra else 0)
        if size < count:
            raise ValueError(f"cannot divide section of {size} steps into {count}")
        stride = 1 if count <= 1 else (size - 1) / (count - 1)
        cur = 0.0
        for _ in range(count):
            out.append(start + round(cur))
            cur += stride
        start += size
    return set(out)


def check_timesteps(t, batch, num_timesteps):
    """Host-side check of training_losses' / q_sample's `t`, before any launch -> list of `batch` ints in [0, num_timesteps)."""
    a = np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t)
    if a.shape != (batch,):
        raise ValueError(f"t must hold one timestep per batch row (shape ({batch},)), not shape {tuple(a.shape)}")
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.all(a == np.floor(a))):
        raise ValueError("t must hold integer timesteps")
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= num_timesteps:
        raise ValueError(f"t must lie in [0, {num_timesteps}), not {a.tolist()}")
    return [int(v) for v in a]


def check_keep(keep, B, T):
    """a frame mask of an inpainting call: bool [B,T], or [T] for all rows -> bool [B,T] (ValueError otherwise; host only)"""
    import torch
    k = torch.as_tensor(keep)
    if k.dtype != torch.bool:
        raise ValueError(f"keep must be a bool mask, not {k.dtype}")
    if k.dim() == 1 and k.shape[0] == T:
        k = k.unsqueeze(0).expand(B, T)
    if tuple(k.shape) != (B, T):
        raise ValueError(f"keep must be [{B}, {T}] or [{T}], not {tuple(k.shape)}")
    return k.contiguous()


def get_named_beta_schedule(name, n):
    if name != "linear":
        raise NotImplementedError(name)
    scale = 1000 / n
    return np.linspace(scale * 0.0001, scale * 0.02, n, dtype=np.float64)


class SpacedDiffusion:
    def __init__(self, use_timesteps, betas, conditioning_free=True, conditioning_free_k=2.0, rescale_timesteps=False, sampler="ddim",
                 model_mean_type="epsilon", model_var_type="learned_range", loss_type="mse", ramp_conditioning_free=True):
        if model_mean_type != "epsilon" or model_var_type != "learned_range" or not ramp_conditioning_free:
            raise NotImplementedError("the device sampler implements the inference model's epsilon / learned_range / ramped-guidance form")
        self.use_timesteps = set(use_timesteps)
        self.original_num_steps = len(betas)
        ac = np.cumprod(1.0 - np.asarray(betas, np.float64))
        last, nb, self.timestep_map = 1.0, [], []
        for i, a in enumerate(ac):
            if i in self.use_timesteps:
                nb.append(1 - a / last)
                last = a
                self.timestep_map.append(i)
        self.sampler = sampler
        self.rescale_timesteps = rescale_timesteps
        self.conditioning_free = conditioning_free
        self.conditioning_free_k = conditioning_free_k
        # GaussianDiffusion.__init__ on the spaced betas (vqvae/utils/diffusion.py:201-228), float64
        betas = np.array(nb, dtype=np.float64)
        self.betas = betas
        self.num_timesteps = int(betas.shape[0])
        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        # a 1-step schedule has no posterior_variance[1] (the reference raises here); its only step adds no noise
        pv = self.posterior_variance
        with np.errstate(divide="ignore"):
            self.posterior_log_variance_clipped = np.log(np.append(pv[1 if len(pv) > 1 else 0], pv[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)
        self.rt = None                # the Runtime q_sample runs on (SynthesizerTrn binds its diffusers; training_losses takes the model's)

    # ---------------------------------------------------------------------------------------------------- evaluation losses
    def q_sample(self, x_start, t, noise=None, *, seed=0, sample_ids=None):
        """vqvae/utils/diffusion.py:243-260 on the device: x_t = sqrt_alphas_cumprod[t] x_start + sqrt_one_minus_alphas_cumprod[t] noise.
        x_start [B,128,T] fp32 CUDA, t [B] integers in [0, num_timesteps) (checked on the host).  noise None: drawn from the Philox
        spec on its own stage (5), keyed by (seed, sample_ids[b]) - never torch's RNG; (x_t, noise) is returned then, else x_t."""
        if self.rt is None:
            raise RuntimeError("q_sample needs a Runtime: set `diffuser.rt` (SynthesizerTrn does for its own diffusers)")
        ts = check_timesteps(t, x_start.shape[0], self.num_timesteps)
        _, x_t, z = self.rt.diff_q_sample(self.rt.diff_schedule(self.timestep_map), x_start.float().contiguous(), ts, noise=noise, seed=seed,
                                          sample_ids=sample_ids)
        return x_t if noise is not None else (x_t, z)

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None, *, seed=0, sample_ids=None):
        """vqvae/utils/diffusion.py:930-1012 for the model's epsilon / learned_range / mse configuration, eval() semantics, no gradients:
        -> dict(loss, mse, vb: fp32 CUDA [B]; x_start_predicted [B,128,T]).  model: a detail_tts_amd DiffusionTts.  t [B]: integers in
        [0, num_timesteps), one per row, checked on the host before any launch; row b's trunk forward runs at model timestep
        timestep_map[t[b]] (dtts_diff_training_losses on this diffuser's schedule, built once and cached).  model_kwargs carries
        precomputed_aligned_embeddings, or aligned_conditioning + conditioning_latent as forward_diff passes them.  noise None: drawn
        as in q_sample.  The losses are means over every row's whole [128, T] rectangle (mean_flat).  The loss path runs the default
        three-product trunk: with the model's fp16 mode on (option trunk_fp16) the call is refused."""
        B, _, T = x_start.shape
        ts = check_timesteps(t, B, self.num_timesteps)
        kw = dict(model_kwargs or {})
        emb = kw.get("precomputed_aligned_embeddings")
        if emb is None and (kw.get("aligned_conditioning") is None or kw.get("conditioning_latent") is None):
            raise ValueError("model_kwargs needs precomputed_aligned_embeddings, or aligned_conditioning and conditioning_latent")
        rt = model.rt
        if rt.get_option("trunk_fp16"):
            raise NotImplementedError("training_losses runs the three-product trunk only: switch the fp16 trunk mode off for this call "
                                      "(diffusion.enable_fp16 = False)")
        if emb is None:
            emb = model.timestep_independent(kw["aligned_conditioning"], kw["conditioning_latent"], T)
        terms, pred = rt.diff_training_losses(rt.diff_schedule(self.timestep_map), x_start.float().contiguous(), ts, emb, noise=noise,
                                              seed=seed, sample_ids=sample_ids)
        return {"loss": terms[:, 2].contiguous(), "mse": terms[:, 0].contiguous(), "vb": terms[:, 1].contiguous(), "x_start_predicted": pred}

    # ---------------------------------------------------------------------------------------------------- bits per dimension
    def _bpd_conditioning(self, who, model, T, clip_denoised, model_kwargs):
        """what calc_bpd_loop and _vb_terms_bpd refuse, before any launch -> (runtime, code embedding [B,768,T]).  These entries evaluate
        the model once per (row, timestep) and run no sampling loop, so they do not pass through _check."""
        if clip_denoised is not True:
            raise ValueError(f"{who}: clip_denoised must be True (the reference's p_mean_variance asserts it)")
        if self.conditioning_free:
            raise NotImplementedError(f"{who} on a conditioning_free=True diffuser: the bound of a guided (cond / uncond mixed) mean is not "
                                      "a likelihood of any model and is not implemented; use a conditioning_free=False diffuser "
                                      "(SynthesizerTrn.diffuser)")
        kw = dict(model_kwargs or {})
        emb = kw.get("precomputed_aligned_embeddings")
        if emb is None and (kw.get("aligned_conditioning") is None or kw.get("conditioning_latent") is None):
            raise ValueError("model_kwargs needs precomputed_aligned_embeddings, or aligned_conditioning and conditioning_latent")
        rt = model.rt
        if rt.get_option("trunk_fp16"):
            raise NotImplementedError(f"{who} runs the three-product trunk only: switch the fp16 trunk mode off for this call "
                                      "(diffusion.enable_fp16 = False)")
        if emb is None:
            emb = model.timestep_independent(kw["aligned_conditioning"], kw["conditioning_latent"], T)
        return rt, emb

    def _prior_bpd(self, x_start):
        """vqvae/utils/diffusion.py:1098-1112 on the device -> fp32 CUDA [B]: the mean over [128, T] of normal_kl(sqrt_alphas_cumprod[S-1]
        x_start, log_one_minus_alphas_cumprod[S-1], 0, 0) / ln 2.  Runs on `diffuser.rt`, as q_sample does."""
        if self.rt is None:
            raise RuntimeError("_prior_bpd needs a Runtime: set `diffuser.rt` (SynthesizerTrn does for its own diffusers)")
        return self.rt.diff_prior_bpd(self.rt.diff_schedule(self.timestep_map), x_start.float().contiguous())

    def _vb_terms_bpd(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None):
        """vqvae/utils/diffusion.py:903-928 -> dict(output: fp32 CUDA [B] in bits, the decoder NLL where t == 0 and the KL elsewhere;
        pred_xstart [B,128,T], clamped to [-1, 1]).  t [B]: integers in [0, num_timesteps), checked on the host; row b's forward runs at
        timestep_map[t[b]] (dtts_diff_forward_rows), then dtts_diff_bpd_terms.  Refusals as in calc_bpd_loop."""
        B, _, T = x_start.shape
        ts = check_timesteps(t, B, self.num_timesteps)
        rt, emb = self._bpd_conditioning("_vb_terms_bpd", model, T, clip_denoised, model_kwargs)
        sched = rt.diff_schedule(self.timestep_map)
        x_start, x_t = x_start.float().contiguous(), x_t.float().contiguous()
        out = rt.diff_forward_rows(x_t, ts, emb, sched=sched)
        # (the ε MSE the kernel also forms needs the noise, which this entry does not have: x_t stands in and that column is dropped)
        terms, pred = rt.diff_bpd_terms(sched, out, x_start, x_t, x_t, ts, want_pred=True)
        return {"output": terms[:, 0].contiguous(), "pred_xstart": pred}

    def calc_bpd_loop(self, model, x_start, clip_denoised=True, model_kwargs=None, *, noise=None, seed=0, sample_ids=None, rows_per_pass=0):
        """vqvae/utils/diffusion.py:1114-1169, the whole variational bound in bits per dimension, eval() semantics, no gradients ->
        dict(total_bpd [B], prior_bpd [B], vb / xstart_mse / mse [B, num_timesteps]; fp32 CUDA).  Column j of the three tables is
        timestep num_timesteps - 1 - j, as the reference stacks them.  model: a detail_tts_amd DiffusionTts; model_kwargs as in
        training_losses.  One device call (dtts_diff_calc_bpd): the (row, timestep) pairs run rows_per_pass at a time (0: the library's
        choice) as rows of the per-row trunk forward; the results are the same bits for every rows_per_pass.

        noise None: every (row, timestep) draws from the Philox spec on its own stage (7), keyed by (seed, sample_ids[b], t) - never
        torch's RNG, and independent of the batch.  noise [num_timesteps, B, 128, T]: noise[t] is used AT TIMESTEP t; the reference
        draws with randn_like in loop order (t = num_timesteps - 1 first), so a caller who wants its numbers stores its k-th draw at
        noise[num_timesteps - 1 - k].

        Refused before any launch: clip_denoised=False (ValueError: the reference asserts it), a conditioning_free=True diffuser
        (NotImplementedError: a guided bound is not a likelihood), the fp16 trunk mode (NotImplementedError), missing conditioning
        (ValueError)."""
        B, _, T = x_start.shape
        rt, emb = self._bpd_conditioning("calc_bpd_loop", model, T, clip_denoised, model_kwargs)
        if noise is not None:
            noise = noise.float().contiguous()
        return rt.diff_calc_bpd(rt.diff_schedule(self.timestep_map), x_start.float().contiguous(), emb, noise=noise, seed=seed,
                                sample_ids=sample_ids, rows_per_pass=rows_per_pass)

    # ---------------------------------------------------------------------------------------------------- sampling loops
    def _check(self, sampler):
        if sampler == "dpm++2m":
            raise NotImplementedError("sampler 'dpm++2m' is not implemented on the device (in k-diffusion the key names Karras-sigma "
                                      "sample_dpmpp_2m): the reference's own DPM-Solver++(2M) path (vqvae/utils/diffusion.py:487-581) "
                                      "is sampler='dpmsolver++'")
        if sampler not in SAMPLERS:
            raise ValueError(f"sampler must be 'p', 'ddim' or 'dpmsolver++', not {sampler!r}")
        if not self.conditioning_free:
            raise NotImplementedError("conditioning_free=False sampling (one unguided forward per step) is not implemented on the device")
        if self.rescale_timesteps and sampler != "dpmsolver++":
            raise NotImplementedError("rescale_timesteps=True (float timesteps) is not implemented on the device")

    # ---------------------------------------------------------------------------------------------------- single steps, inversion
    def _step_args(self, who, model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, sampler="ddim"):
        """what the single-step entries refuse, on the host before any launch -> (runtime, schedule id, step index, x, code embedding)"""
        self._check(sampler)
        if clip_denoised is not True:
            raise ValueError(f"{who}: clip_denoised must be True (the reference's p_mean_variance asserts it)")
        if denoised_fn is not None:
            raise ValueError(f"{who}: denoised_fn must be None (the reference's p_mean_variance asserts it)")
        if cond_fn is not None:
            raise ValueError(f"{who}: cond_fn (condition_mean / condition_score) is not implemented on the device")
        ts = check_timesteps(t, x.shape[0], self.num_timesteps)
        if len(set(ts)) != 1:
            raise ValueError(f"{who}: every row of a call must sit at the same t (the reference's guidance ramp reads t[0]), not {ts}")
        emb = (model_kwargs or {}).get("precomputed_aligned_embeddings")
        if emb is None:
            raise ValueError("precomputed_aligned_embeddings is required (as in do_spectrogram_diffusion)")
        rt = model.rt
        return rt, rt.diff_schedule(self.timestep_map), ts[0], x.float().contiguous(), emb

    def p_mean_variance(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, *, lens=None):
        """vqvae/utils/diffusion.py:284-386 on the device (dtts_diff_mean_variance) -> dict(mean, variance, log_variance, pred_xstart),
        each [B,128,T]: both model forwards at timestep_map[t], the guided eps with t's ramp value, pred_xstart clamped to [-1, 1], the
        posterior mean of it and the learned-range variance.  t [B]: one integer step for all rows.  Refusals: see ddim_reverse_sample."""
        rt, sched, i, x, emb = self._step_args("p_mean_variance", model, x, t, clip_denoised, denoised_fn, None, model_kwargs)
        mean, var, logvar, x0 = rt.diff_mean_variance(x, emb, i, sched, lens=lens)
        return {"mean": mean, "variance": var, "log_variance": logvar, "pred_xstart": x0}

    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, *, noise=None, seed=0,
                 sample_ids=None, lens=None):
        """vqvae/utils/diffusion.py:445-485 (dtts_diff_step, sampler p) -> dict(sample, pred_xstart).  The noise of a step t != 0 is the
        Philox draw the loops make at that step, keyed by (seed, sample_ids[b], t), unless `noise` [B,128,T] is given."""
        rt, sched, i, x, emb = self._step_args("p_sample", model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, "p")
        sample_ids = list(range(x.shape[0])) if sample_ids is None else sample_ids
        xs, x0 = rt.diff_step(x, emb, i, seed, sample_ids, sched=sched, sampler=0, lens=lens, noise=noise, return_x0=True)
        return {"sample": xs, "pred_xstart": x0}

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0, *, noise=None,
                    seed=0, sample_ids=None, lens=None):
        """vqvae/utils/diffusion.py:744-783 (dtts_diff_step, sampler ddim) -> dict(sample, pred_xstart); noise as in p_sample, drawn
        only when eta > 0 and t != 0."""
        if eta < 0:
            raise ValueError("eta must be >= 0")
        rt, sched, i, x, emb = self._step_args("ddim_sample", model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs)
        sample_ids = list(range(x.shape[0])) if sample_ids is None else sample_ids
        xs, x0 = rt.diff_step(x, emb, i, seed, sample_ids, sched=sched, sampler=1, eta=float(eta), lens=lens, noise=noise, return_x0=True)
        return {"sample": xs, "pred_xstart": x0}

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, eta=0.0, *, lens=None):
        """vqvae/utils/diffusion.py:785-817 on the device (dtts_diff_reverse_step): one step of the deterministic DDIM ODE upwards, from x
        at the level of step t to the level of step t + 1 -> dict(sample, pred_xstart).  At t = num_timesteps - 1 alphas_cumprod_next
        is 0 and the sample is the re-derived eps alone.

        Refused on the host before any launch (ValueError): eta != 0; clip_denoised other than True or a denoised_fn (the reference
        asserts both); rows at different t (the reference's guidance ramp reads t[0]); t out of [0, num_timesteps).  A
        conditioning_free=False or rescale_timesteps=True diffuser is refused as by the sampling loops."""
        if eta != 0.0:
            raise ValueError("Reverse ODE only for deterministic path")
        rt, sched, i, x, emb = self._step_args("ddim_reverse_sample", model, x, t, clip_denoised, denoised_fn, None, model_kwargs)
        xs, x0 = rt.diff_reverse_step(x, emb, i, sched, lens=lens, return_x0=True)
        return {"sample": xs, "pred_xstart": x0}

    def invert_depth(self, depth):
        """the depth of an inversion, checked: None is num_timesteps.  Inverting to depth d yields x at the level of step index d, which
        ddim_sample_loop(noise=x, t_start=d) consumes for d <= num_timesteps - 1; depth num_timesteps ends at alphas_cumprod_next = 0,
        yields pure eps' and can only feed a full loop as `noise` -> (depth, t_start or None for the full loop)"""
        d = self.num_timesteps if depth is None else depth
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 1 <= d <= self.num_timesteps:
            raise ValueError(f"depth must be an integer in [1, {self.num_timesteps}], not {depth!r}")
        return int(d), (int(d) if d < self.num_timesteps else None)

    def ddim_reverse_sample_loop(self, model, x_start, model_kwargs=None, *, depth=None, lens=None, return_trajectory=False):
        """DDIM inversion: ddim_reverse_sample iterated for t = 0 .. depth - 1 in ONE device call (dtts_diff_invert), the fast path.  The
        reference has the step (vqvae/utils/diffusion.py:785-817) and no loop of its own; this is that step fed its own output, and
        equals calling ddim_reverse_sample depth times bit for bit.  -> x at the level of step index `depth` [B,128,T]; with
        return_trajectory a dict(sample, trajectory [depth,B,128,T] = x after each step, pred_xstart [depth,B,128,T]).

        depth (default num_timesteps) and t_start pair up as follows: depth d <= num_timesteps - 1 is consumed by
        ddim_sample_loop(noise=x, t_start=d); depth num_timesteps ends at alphas_cumprod_next = 0, is pure eps' and can only feed a
        full loop as `noise` (invert_depth).  Inversion followed by DDIM at eta = 0 is NOT the identity: the guidance and the clamp of
        pred_xstart are not invertible (the reference's own round trip on the test weights misses x_start by 0.88 max-abs from depth 5
        of 10 and by 1.37 from depth 9)."""
        self._check("ddim")
        d, _ = self.invert_depth(depth)
        emb = (model_kwargs or {}).get("precomputed_aligned_embeddings")
        if emb is None:
            raise ValueError("precomputed_aligned_embeddings is required (as in do_spectrogram_diffusion)")
        rt = model.rt
        r = rt.diff_invert(x_start.float().contiguous(), emb, d, rt.diff_schedule(self.timestep_map), lens=lens,
                           return_trajectory=return_trajectory)
        return {"sample": r[0], "trajectory": r[1], "pred_xstart": r[2]} if return_trajectory else r

    def _progressive(self, step, model, shape, noise, seed, sample_ids, kw):
        B = shape[0]
        sample_ids = list(range(B)) if sample_ids is None else sample_ids
        if noise is None:
            raise ValueError("the progressive generators need `noise` (x_T): the loop calls draw it on the device")
        img = noise
        for i in range(self.num_timesteps - 1, -1, -1):
            out = step(model, img, np.full(B, i, np.int64), seed=seed, sample_ids=sample_ids, **kw)
            yield out
            img = out["sample"]

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                                  device=None, progress=False, *, seed=0, sample_ids=None, lens=None):
        """vqvae/utils/diffusion.py:700-742: a generator over p_sample's dicts, t = num_timesteps - 1 .. 0.  A host loop, one device
        call per step with the code-path terms evaluated inside every step: p_sample_loop is the fast path.  `noise` (x_T) is required."""
        return self._progressive(self.p_sample, model, shape, noise, seed, sample_ids,
                                 dict(clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn, model_kwargs=model_kwargs, lens=lens))

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                                     device=None, progress=False, eta=0.0, *, seed=0, sample_ids=None, lens=None):
        """vqvae/utils/diffusion.py:853-901: a generator over ddim_sample's dicts.  A host loop, one device call per step:
        ddim_sample_loop is the fast path.  `noise` (x_T) is required."""
        return self._progressive(self.ddim_sample, model, shape, noise, seed, sample_ids,
                                 dict(clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn, model_kwargs=model_kwargs, eta=eta,
                                      lens=lens))

    def _loop_from(self, sampler, model, shape, noise, model_kwargs, seed, sample_ids, lens, eta, t_start, denorm=False):
        """a sampling loop entered at step t_start: `noise` is x at that level and steps t_start .. 0 run (dtts_diff_sample_from)"""
        self._check(sampler)
        if sampler == "dpmsolver++":
            raise ValueError("t_start is not available with dpmsolver++ (a multistep solver has no state below its first step)")
        if eta < 0:
            raise ValueError("eta must be >= 0")
        if isinstance(t_start, bool) or not isinstance(t_start, (int, np.integer)) or not 0 <= t_start < self.num_timesteps:
            raise ValueError(f"t_start must be an integer in [0, {self.num_timesteps}), not {t_start!r}")
        if noise is None:
            raise ValueError("t_start needs `noise`: x at the level of step t_start")
        emb = (model_kwargs or {}).get("precomputed_aligned_embeddings")
        if emb is None:
            raise ValueError("precomputed_aligned_embeddings is required (as in do_spectrogram_diffusion)")
        sample_ids = list(range(shape[0])) if sample_ids is None else sample_ids
        rt = model.rt
        return rt.diff_sample_from(noise.float().contiguous(), emb, int(t_start), seed, sample_ids, sched=rt.diff_schedule(self.timestep_map),
                                   sampler=SAMPLERS[sampler], eta=eta, lens=lens, denorm=denorm)

    def _loop(self, sampler, model, shape, noise, model_kwargs, seed, sample_ids, lens, eta, denorm=False):
        self._check(sampler)
        if eta < 0:
            raise ValueError("eta must be >= 0")
        if sampler == "dpmsolver++":
            if self.num_timesteps < 2:
                raise ValueError("dpmsolver++ needs >= 2 steps (the reference asserts steps >= order)")
            if self.conditioning_free_k != 2.0:
                raise NotImplementedError("the device's DPM-Solver++ guidance scale is the model's cond_free_k = 2.0")
        emb = (model_kwargs or {}).get("precomputed_aligned_embeddings")
        if emb is None:
            raise ValueError("precomputed_aligned_embeddings is required (as in do_spectrogram_diffusion)")
        B = shape[0]
        sample_ids = list(range(B)) if sample_ids is None else sample_ids
        rt = model.rt
        if sampler == "dpmsolver++":
            sched = rt.diff_schedule_dpm(self.num_timesteps)
        else:
            sched = rt.diff_schedule(self.timestep_map)
        return rt.diff_sample_ex(emb, seed, sample_ids, sched=sched, sampler=SAMPLERS[sampler], eta=eta, lens=lens, x_init=noise,
                                 denorm=denorm)

    def _inpaint_args(self, known, keep, resample, shape):
        """known= / keep= / resample= of the sampling loops, checked on the host -> None (none given: today's path) or
        (known, keep [B,T] bool, U).  ValueError: one of known / keep without the other, resample without them, a mask of another
        shape or dtype, resample not an int in [1, 32]."""
        if known is None and keep is None:
            if resample != 1:
                raise ValueError("resample repeats the steps of an inpainting call: it needs known= and keep=")
            return None
        if self.sampler == "dpmsolver++":
            raise ValueError("inpainting is not available on a dpmsolver++ diffuser (a multistep history does not survive the overwrite)")
        if known is None or keep is None:
            raise ValueError("inpainting needs both known= (the normalised mel) and keep= (the frame mask), or neither")
        if isinstance(resample, bool) or not isinstance(resample, (int, np.integer)) or not 1 <= resample <= 32:
            raise ValueError(f"resample must be an integer in [1, 32], not {resample!r}")
        B, _, T = shape
        if tuple(known.shape) != tuple(shape):
            raise ValueError(f"known must be {tuple(shape)}, not {tuple(known.shape)}")
        return known, check_keep(keep, B, T), int(resample)

    def _inpaint_loop(self, sampler, model, shape, noise, model_kwargs, seed, sample_ids, lens, eta, t_start, inp, step_noise=None,
                      known_noise=None, renoise=None, return_trajectory=False):
        """a sampling loop with the kept frames overwritten after every step (dtts_diff_inpaint); `noise` is x_T, or x at t_start"""
        self._check(sampler)
        if sampler == "dpmsolver++":
            raise ValueError("inpainting is not available with dpmsolver++ (a multistep history does not survive the overwrite)")
        if eta < 0:
            raise ValueError("eta must be >= 0")
        if t_start is not None:
            if isinstance(t_start, bool) or not isinstance(t_start, (int, np.integer)) or not 0 <= t_start < self.num_timesteps:
                raise ValueError(f"t_start must be an integer in [0, {self.num_timesteps}), not {t_start!r}")
            if noise is None:
                raise ValueError("t_start needs `noise`: x at the level of step t_start")
        emb = (model_kwargs or {}).get("precomputed_aligned_embeddings")
        if emb is None:
            raise ValueError("precomputed_aligned_embeddings is required (as in do_spectrogram_diffusion)")
        known, keep, U = inp
        sample_ids = list(range(shape[0])) if sample_ids is None else sample_ids
        rt = model.rt
        return rt.diff_inpaint(known.float().contiguous(), keep, emb, seed, sample_ids, sched=rt.diff_schedule(self.timestep_map),
                               sampler=SAMPLERS[sampler], eta=eta, resample=U, first_step=None if t_start is None else int(t_start),
                               x_init=None if noise is None else noise.float().contiguous(), lens=lens, step_noise=step_noise,
                               known_noise=known_noise, renoise=renoise, return_trajectory=return_trajectory)

    def p_sample_loop(self, model, shape, noise=None, model_kwargs=None, progress=False, seed=0, sample_ids=None, lens=None, t_start=None,
                      known=None, keep=None, resample=1, step_noise=None, known_noise=None, renoise=None, return_trajectory=False,
                      **_):
        """model: a detail_tts_amd DiffusionTts; returns x_0 (normalised mel) [B,128,T] of THIS diffuser's schedule.  t_start = s: `noise`
        (required then) is x at the level of step s and steps s .. 0 run, with the Philox noise the whole loop draws at those steps;
        t_start = num_timesteps - 1 is the whole loop from x_T = noise.  None: the whole loop.

        Inpainting (RePaint): known [B,128,T] (a normalised mel) and keep (bool [B,T], or [T] for all rows) - both or neither - hold
        the frames with keep set to `known`: after every step they are overwritten with known noised to the level just reached, so the
        other frames are generated in their context at every noise level; resample = U runs every step above 0 U times with one
        forward step in between.  The kept frames of the result are known's bits (a select); known is never read elsewhere.  Nothing
        kept with U = 1 is the plain loop bit for bit.  step_noise / known_noise / renoise [t * U + 1, B,128,T] (t = t_start or
        num_timesteps - 1) replace the three Philox streams, and return_trajectory=True returns (x_0, x after every evaluation, the
        same leading axis) - both for parity tests, and only on the inpainting path."""
        inp = self._inpaint_args(known, keep, resample, shape)
        if inp is not None:
            return self._inpaint_loop("p", model, shape, noise, model_kwargs, seed, sample_ids, lens, 0.0, t_start, inp, step_noise,
                                      known_noise, renoise, return_trajectory)
        if t_start is not None:
            return self._loop_from("p", model, shape, noise, model_kwargs, seed, sample_ids, lens, 0.0, t_start)
        return self._loop("p", model, shape, noise, model_kwargs, seed, sample_ids, lens, 0.0)

    def ddim_sample_loop(self, model, shape, noise=None, model_kwargs=None, progress=False, eta=0.0, seed=0, sample_ids=None, lens=None,
                         t_start=None, known=None, keep=None, resample=1, step_noise=None, known_noise=None, renoise=None,
                         return_trajectory=False, **_):
        """vqvae/utils/diffusion.py:819-851 (ddim_sample :744-783 per step, Philox noise when eta > 0).  t_start = s: `noise` (required
        then) is x at the level of step s and steps s .. 0 run - what ddim_reverse_sample_loop(depth=s) yields, for s <= num_timesteps
        - 1; an inversion to depth num_timesteps is pure eps' and feeds the whole loop (t_start None) as `noise`.
        known / keep / resample: inpainting, as in p_sample_loop."""
        inp = self._inpaint_args(known, keep, resample, shape)
        if inp is not None:
            return self._inpaint_loop("ddim", model, shape, noise, model_kwargs, seed, sample_ids, lens, float(eta), t_start, inp,
                                      step_noise, known_noise, renoise, return_trajectory)
        if t_start is not None:
            return self._loop_from("ddim", model, shape, noise, model_kwargs, seed, sample_ids, lens, float(eta), t_start)
        return self._loop("ddim", model, shape, noise, model_kwargs, seed, sample_ids, lens, float(eta))

    def k_diffusion_sample_loop(self, k_sampler, pbar, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                device=None, model_kwargs=None, progress=False, seed=0, sample_ids=None, lens=None, t_start=None,
                                known=None, keep=None, resample=1, **_):
        """vqvae/utils/diffusion.py:487-581: DPM-Solver++(2M) over num_timesteps steps (vqvae/utils/dpm_solver.py, time_uniform,
        multistep, order 2) with constant guidance cond_free_k; as in the reference, `k_sampler` is ignored.  x_T = `noise` (None: the
        Philox STAGE_DIFF_INIT draw); no noise after it, no clamp.  `pbar` (may be None) is advanced by the num_timesteps model
        evaluations once the loop is enqueued."""
        if t_start is not None:
            raise ValueError("t_start is not available with dpmsolver++ (a multistep solver has no state below its first step)")
        if known is not None or keep is not None or resample != 1:
            raise ValueError("inpainting is not available with dpmsolver++ (a multistep history does not survive the overwrite)")
        if not isinstance(model_kwargs, dict):
            raise ValueError("model_kwargs must be a dict (the reference asserts it)")
        x = self._loop("dpmsolver++", model, shape, noise, model_kwargs, seed, sample_ids, lens, 0.0)
        if pbar is not None:
            pbar.update(self.num_timesteps)
        return x

    def sample_loop(self, *args, **kwargs):
        """vqvae/utils/diffusion.py:640-652: dispatch on self.sampler ("dpmsolver++": k_diffusion_sample_loop)"""
        self._check(self.sampler)
        if self.sampler == "dpmsolver++":
            if kwargs.get("known") is not None or kwargs.get("keep") is not None or kwargs.get("resample", 1) != 1:
                raise ValueError("inpainting is not available with dpmsolver++ (a multistep history does not survive the overwrite)")
            return self.k_diffusion_sample_loop(None, None, *args, **kwargs)
        if self.sampler == "ddim":
            return self.ddim_sample_loop(*args, **kwargs)
        return self.p_sample_loop(*args, **kwargs)
