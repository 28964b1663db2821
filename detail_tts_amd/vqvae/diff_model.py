"""DiffusionTts mirror (reference: vqvae/diff_model.py:133-322) — the device work is libdetail_hip.so."""
from __future__ import annotations

import torch


class DiffusionTts:
    def __init__(self, rt, cfg):
        self.rt = rt
        self.model_channels = cfg["model_channels"]
        self.in_channels = cfg["in_channels"]
        self.out_channels = cfg["out_channels"]
        self.num_heads = cfg["num_heads"]
        if cfg.get("use_fp16", False):                          # vqvae/diff_model.py:157: the constructor stores use_fp16
            self.enable_fp16 = True

    @property
    def enable_fp16(self):
        """The reference's half-precision switch (vqvae/diff_model.py:157, 299-309: layers[1:] under autocast), settable as on its
        module.  Here: option "trunk_fp16" - those layers' convs and attention products as one fp16 product, fp32 accumulation."""
        return bool(self.rt.get_option("trunk_fp16"))

    @enable_fp16.setter
    def enable_fp16(self, on):
        self.rt.set_option("trunk_fp16", 1 if on else 0)

    def get_conditioning(self, conditioning_input, lengths=None):
        """vqvae/diff_model.py:221-229: mel [B,128,T] -> [B,1536]; n clips per speaker [B,n,128,T] (lengths [B,n]: every clip's valid
        length, an extension) -> the mean over the n embedder outputs concatenated along time, as the reference takes it: the B n clips
        run as one batch, then the pool weighted by each clip's embedder length (csrc/voice.hip, voice.embedder_length)."""
        if conditioning_input.dim() != 4:
            return self.rt.diff_conditioning(conditioning_input.float().contiguous(), lengths)
        import numpy as np
        from ..voice import check_clips, embedder_length
        S, n, T, lens = check_clips(conditioning_input, None, lengths)
        d = self.rt.diff_conditioning(conditioning_input.float().reshape(S * n, -1, T).contiguous(), lens)
        if n == 1:
            return d
        return self.rt.voice_pool(d.view(S, n, -1), np.asarray([embedder_length(l) for l in lens], np.float32).reshape(S, n))

    def timestep_independent(self, aligned_conditioning, conditioning_latent, expected_seq_len, return_code_pred=False, lengths=None,
                             *, frames=None, durations=None):
        """vqvae/diff_model.py:231-260 (latent branch): [B,n,768] -> [B,768,expected_seq_len].  expected_seq_len = 4 n is the
        inference path's x4 launch.  Any other positive multiple of 4 (the vocoder's granule) with lengths=None is the reference's
        F.interpolate(size=expected_seq_len, mode='nearest') of every row, torch's float32 index rule bit for bit (duration.py).  A
        ragged batch (lengths: the rows' code counts, an extension) at other rates says so per row: frames= (one frame count per row,
        expected_seq_len >= their largest) and optionally durations= (Runtime.diff_timestep_independent)."""
        if return_code_pred:
            raise NotImplementedError("return_code_pred is a training-only branch")
        if aligned_conditioning.dtype != torch.float32:
            raise NotImplementedError("token (code_converter) conditioning is not on the inference path")
        B, n = aligned_conditioning.shape[0], aligned_conditioning.shape[1]
        T = int(expected_seq_len)
        if frames is None:
            if durations is not None:
                raise ValueError("durations= needs frames= (the rows' frame counts)")
            if T != 4 * n:
                if lengths is not None:
                    raise ValueError("expected_seq_len must be 4 * n for a ragged batch (lengths=): give the rows' frame counts with "
                                     "the keyword frames= (one per row, each a multiple of 4) instead")
                if T < 4 or T % 4:
                    raise ValueError(f"expected_seq_len must be a positive multiple of 4, but is {expected_seq_len}")
                frames = [T] * B
        elif T % 4 or T < max(int(f) for f in frames):
            raise ValueError(f"expected_seq_len = {expected_seq_len} must be a multiple of 4 that holds every row of frames= {list(frames)}")
        lat_cm = aligned_conditioning.permute(0, 2, 1).contiguous()
        if frames is None:
            return self.rt.diff_timestep_independent(lat_cm, conditioning_latent.contiguous(), lengths)
        out = self.rt.diff_timestep_independent(lat_cm, conditioning_latent.contiguous(), lengths, frames=frames, durations=durations)
        if out.shape[-1] < T:                                       # every row shorter than expected_seq_len: zero columns behind them
            out = torch.nn.functional.pad(out, (0, T - out.shape[-1]))
        return out

    def forward(self, x, timesteps, aligned_conditioning=None, conditioning_latent=None, precomputed_aligned_embeddings=None,
                conditioning_free=False, return_code_pred=False, lengths=None):
        """vqvae/diff_model.py:262-322.  `timesteps` are model-side timesteps in [0, 4000): integers as _WrappedModel passes them
        (vqvae/utils/diffusion.py:1282-1287; those of the default 50-step schedule use its bind-time tables), or fractional fp32 times
        as k_diffusion_sample_loop passes them (t * 1000, :534-535; timestep_embedding takes `timesteps.float()`, :20-38).  Integer
        timesteps may differ between rows (conditional branch only, not with the fp16 trunk mode); fractional ones may not."""
        if precomputed_aligned_embeddings is None and not conditioning_free:
            precomputed_aligned_embeddings = self.timestep_independent(aligned_conditioning, conditioning_latent, x.shape[-1])
        tl = torch.as_tensor(timesteps).reshape(-1).float().tolist()
        for t in tl:
            if not 0 <= t < 4000:
                raise ValueError(f"timestep {t} is outside the trained range [0, 4000)")
        emb = None if conditioning_free else precomputed_aligned_embeddings
        if len(set(tl)) != 1:
            # rows at different timesteps (training_losses draws one t per row): the conditional branch alone, every row at its own
            # column of a one-off schedule of the distinct values (dtts_diff_forward_rows)
            if any(t != int(t) for t in tl):
                raise ValueError("batch rows at different FRACTIONAL timesteps are not implemented (integer timesteps may differ)")
            if conditioning_free:
                raise ValueError("conditioning_free=True needs all batch rows at one timestep (as in p_sample_loop)")
            if len(tl) != x.shape[0]:
                raise ValueError(f"{len(tl)} timesteps for {x.shape[0]} batch rows")
            distinct = sorted(set(int(t) for t in tl))
            cols = [distinct.index(int(t)) for t in tl]
            return self.rt.diff_forward_rows(x.float().contiguous(), cols, emb, sched=self.rt.diff_schedule(distinct), lens=lengths)
        t = tl[0]
        if t == int(t):
            return self.rt.diff_forward_t(x.float().contiguous(), int(t), emb, cond_free=conditioning_free, lens=lengths)
        return self.rt.diff_forward_tf(x.float().contiguous(), t, emb, cond_free=conditioning_free, lens=lengths)

    __call__ = forward
