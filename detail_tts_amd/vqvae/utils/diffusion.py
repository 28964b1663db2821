"""Sampler object mirroring the subset of the reference's SpacedDiffusion that inference and evaluation use
(vqvae/utils/diffusion.py:179-228 + 1172-1272; p_sample_loop :654-742, ddim_sample_loop :819-899, k_diffusion_sample_loop :487-581,
sample_loop :640-652; q_sample :243-260, training_losses :930-1012; calc_bpd_loop :1114-1169, _vb_terms_bpd :903-928, _prior_bpd
:1098-1112).  The arithmetic lives in libdetail_hip.so (dtts_diff_sample_ex, dtts_diff_q_sample, dtts_diff_training_losses,
dtts_diff_calc_bpd); this class carries the schedule constants and the call surface."""
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

    def p_sample_loop(self, model, shape, noise=None, model_kwargs=None, progress=False, seed=0, sample_ids=None, lens=None, **_):
        """model: a detail_tts_amd DiffusionTts; returns x_0 (normalised mel) [B,128,T] of THIS diffuser's schedule."""
        return self._loop("p", model, shape, noise, model_kwargs, seed, sample_ids, lens, 0.0)

    def ddim_sample_loop(self, model, shape, noise=None, model_kwargs=None, progress=False, eta=0.0, seed=0, sample_ids=None, lens=None,
                         **_):
        """vqvae/utils/diffusion.py:819-851 (ddim_sample :744-783 per step, Philox noise when eta > 0)"""
        return self._loop("ddim", model, shape, noise, model_kwargs, seed, sample_ids, lens, float(eta))

    def k_diffusion_sample_loop(self, k_sampler, pbar, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                device=None, model_kwargs=None, progress=False, seed=0, sample_ids=None, lens=None, **_):
        """vqvae/utils/diffusion.py:487-581: DPM-Solver++(2M) over num_timesteps steps (vqvae/utils/dpm_solver.py, time_uniform,
        multistep, order 2) with constant guidance cond_free_k; as in the reference, `k_sampler` is ignored.  x_T = `noise` (None: the
        Philox STAGE_DIFF_INIT draw); no noise after it, no clamp.  `pbar` (may be None) is advanced by the num_timesteps model
        evaluations once the loop is enqueued."""
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
            return self.k_diffusion_sample_loop(None, None, *args, **kwargs)
        if self.sampler == "ddim":
            return self.ddim_sample_loop(*args, **kwargs)
        return self.p_sample_loop(*args, **kwargs)
