"""A speaker as a value: the latents the three prompt encoders make of the prompt mel, computed once.

    gpt        [S, 768]   gpt.conditioning_encoder          (UnifiedVoice.get_conditioning, gpt/model.py:419-427)
    diffusion  [S, 1536]  diffusion.contextual_embedder     (DiffusionTts.get_conditioning, vqvae/diff_model.py:221-229)
    vq         [S, 768]   vq_ref_enc (infer_gpt only); None when the model binds no VQ weights

There is no stage-C member: infer_flowvae runs ref_enc on the GENERATED mel, not on the prompt.

A speaker may be made of n clips (refer [S, n, 128, T]), as in the reference's two get_conditioning: the S n clips run through each encoder
as one ragged batch of S n rows, then one pool launch per member (csrc/voice.hip) - the plain mean for gpt and vq, the mean weighted by
each clip's embedder length ((l - 1) // 2 + 1 - 1) // 2 + 1 for diffusion, which is the reference's mean over the concatenation.  n = 1 is
not pooled: the member IS the encoder's output, so a request that hands the voice back in computes what the `refer` form computes, bit
for bit.  How a pooled or blended voice SOUNDS under a trained checkpoint is unmeasured.

The checks here are host code (no device, no library): every refusal is a ValueError before any launch."""
from __future__ import annotations

import numpy as np
import torch

MEMBERS = ("gpt", "diffusion", "vq")


def model_dims(cfg):
    """the member widths of a model of this config"""
    return dict(gpt=int(cfg["gpt"]["model_dim"]), diffusion=2 * int(cfg["diffusion"]["model_channels"]),
                vq=4 * int(cfg["vaegan"]["inter_channels"]))


def embedder_length(l):
    """frames the contextual embedder's two stride-2 convs (k 3, pad 1) leave of l mel frames: Model::diff_conditioning's l2"""
    return ((int(l) - 1) // 2 + 1 - 1) // 2 + 1


def check_weights(weights, S, n):
    """pool / blend weights -> float32 [S, n]: finite, >= 0, every speaker's sum > 0 (and finite in float32)"""
    w = np.asarray(weights, np.float64)
    if w.shape != (S, n):
        raise ValueError(f"weights have to be [{S}, {n}], but are {w.shape}")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights have to be finite and >= 0")
    w32 = np.ascontiguousarray(w, np.float32)
    with np.errstate(over="ignore"):
        s = w32.sum(1, dtype=np.float32)
    if not (np.isfinite(w32).all() and np.isfinite(s).all() and (s > 0).all()):
        raise ValueError("weights need a sum > 0 (and finite in float32)")
    return w32


def check_clips(refer, refer_lengths=None, clip_lengths=None):
    """get_conditioning_latents' arguments -> (S, n, T, lens): refer [S,128,T] (n = 1) or [S,n,128,T]; lens = the S n clips' valid
    lengths in batch order, each in 1 .. T, from refer_lengths [S] (3-D input) or clip_lengths [S,n] (either form; default T)"""
    shape = tuple(refer.shape)
    if len(shape) == 3:
        S, n, T = shape[0], 1, shape[2]
    elif len(shape) == 4:
        S, n, T = shape[0], shape[1], shape[3]
        if refer_lengths is not None:
            raise ValueError("refer [S,n,128,T]: give clip_lengths [S,n], not refer_lengths")
    else:
        raise ValueError(f"refer has to be [S,128,T] or [S,n,128,T], but is {shape}")
    if min(shape) < 1:
        raise ValueError(f"refer has an empty dimension: {shape}")
    if refer_lengths is not None and clip_lengths is not None:
        raise ValueError("give refer_lengths or clip_lengths, not both")
    given = refer_lengths if refer_lengths is not None else clip_lengths
    if given is None:
        return S, n, T, [T] * (S * n)
    lens = np.asarray(torch.as_tensor(given).cpu().numpy())
    want = (S,) if refer_lengths is not None else (S, n)
    if lens.shape != want and not (n == 1 and lens.shape == (S,)):
        raise ValueError(f"{'refer_lengths' if refer_lengths is not None else 'clip_lengths'} have to be {list(want)}, but are {list(lens.shape)}")
    if lens.dtype.kind not in "iu":
        raise ValueError("clip lengths have to be integers")
    lens = [int(v) for v in lens.reshape(-1)]
    if min(lens) < 1 or max(lens) > T:
        raise ValueError(f"clip lengths have to be in 1 .. T = {T}, but are {lens}")
    return S, n, T, lens


class Voice:
    """S speakers' latents (device tensors, fp32); see the module text.  dims: the member widths it was made with."""

    def __init__(self, gpt, diffusion, vq=None, rt=None):
        self.rt = rt        # the Runtime that made it (None: a voice put together by hand); blend launches its pool on it
        for name, t in (("gpt", gpt), ("diffusion", diffusion), ("vq", vq)):
            if t is None and name == "vq":
                continue
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32 or t.shape[0] != gpt.shape[0] or t.shape[0] < 1:
                raise ValueError(f"Voice.{name} has to be a float32 tensor [S, width] with the S of the other members")
        self.gpt, self.diffusion, self.vq = gpt.contiguous(), diffusion.contiguous(), None if vq is None else vq.contiguous()

    @property
    def S(self):
        return int(self.gpt.shape[0])

    @property
    def dims(self):
        return dict(gpt=int(self.gpt.shape[1]), diffusion=int(self.diffusion.shape[1]), vq=None if self.vq is None else int(self.vq.shape[1]))

    def members(self):
        return [(k, getattr(self, k)) for k in MEMBERS if getattr(self, k) is not None]

    def check_dims(self, dims):
        """ValueError naming the first member whose width is not the model's (dims: model_dims(cfg))"""
        for k, t in self.members():
            if int(t.shape[1]) != int(dims[k]):
                raise ValueError(f"Voice.{k} is {int(t.shape[1])} wide, the model's is {int(dims[k])}: a voice of another model")

    def rows(self, idx):
        """the speakers idx (an int, a slice or a list of ints) as a Voice"""
        if isinstance(idx, (int, np.integer)):
            idx = [int(idx)]
        if not isinstance(idx, slice):
            idx = [int(i) for i in idx]
            if not idx or min(idx) < -self.S or max(idx) >= self.S:
                raise ValueError(f"Voice.rows: speakers {idx} of a voice of {self.S}")
            idx = torch.as_tensor(idx, device=self.gpt.device)
        return Voice(*[None if t is None else t[idx].contiguous() for t in (self.gpt, self.diffusion, self.vq)], rt=self.rt)

    def for_batch(self, B):
        """the voice of a request of B rows: S = 1 serves every row, else S has to be B (checked by check_speaker before any launch)"""
        if self.S == B:
            return self
        if self.S != 1:
            raise ValueError(f"a Voice of {self.S} speakers cannot serve {B} rows (S has to be 1 or B)")
        return Voice(*[None if t is None else t.expand(B, -1).contiguous() for t in (self.gpt, self.diffusion, self.vq)], rt=self.rt)

    def save(self, path):
        """one .npz: the members' vectors and their widths (vq_dim 0 = no vq member)"""
        d = self.dims
        arrays = {k: t.detach().cpu().numpy() for k, t in self.members()}
        with open(path, "wb") as f:         # (a file object: numpy appends no suffix of its own)
            np.savez(f, gpt_dim=np.int64(d["gpt"]), diffusion_dim=np.int64(d["diffusion"]), vq_dim=np.int64(d["vq"] or 0), **arrays)

    @classmethod
    def load(cls, path, model=None, *, dims=None, device=None):
        """the Voice save() wrote, on the model's device; a member whose width is not the model's is refused by name"""
        if model is not None:
            dims = model_dims(model.cfg) if dims is None else dims
            device = model.device if device is None else device
        with np.load(path) as z:
            stored = dict(gpt=int(z["gpt_dim"]), diffusion=int(z["diffusion_dim"]), vq=int(z["vq_dim"]))
            arr = {k: np.ascontiguousarray(z[k], np.float32) for k in MEMBERS if k in z.files}
        for k in ("gpt", "diffusion"):
            if k not in arr:
                raise ValueError(f"{path}: no `{k}` member")
        for k, a in arr.items():
            if a.ndim != 2 or a.shape[1] != stored[k]:
                raise ValueError(f"{path}: `{k}` is {a.shape}, the file says width {stored[k]}")
            if dims is not None and a.shape[1] != int(dims[k]):
                raise ValueError(f"{path}: Voice.{k} is {a.shape[1]} wide, the model's is {int(dims[k])}: a voice of another model")
        t = {k: torch.from_numpy(a) if device is None else torch.from_numpy(a).to(device) for k, a in arr.items()}
        return cls(t["gpt"], t["diffusion"], t.get("vq"), rt=getattr(model, "rt", None) if model is not None else None)

    @staticmethod
    def cat(voices):
        """voices of the same members and widths joined along S, in order: the inverse of rows() (cat([v.rows(i) for i in ...]) holds
        the bits of v's rows).  A copy per member (torch.cat), no kernel of the library."""
        voices = list(voices)
        if not voices:
            raise ValueError("Voice.cat: no voices")
        for v in voices:
            if not isinstance(v, Voice):
                raise ValueError(f"Voice.cat: a {type(v).__name__} among the voices")
            if v.dims != voices[0].dims:
                raise ValueError(f"Voice.cat: voices of different members or widths ({v.dims} against {voices[0].dims})")
            if v.gpt.device != voices[0].gpt.device:
                raise ValueError("Voice.cat: voices on different devices")
        if len(voices) == 1:
            return voices[0]
        out = {k: torch.cat([getattr(v, k) for v in voices], 0).contiguous() for k, _ in voices[0].members()}
        return Voice(out["gpt"], out["diffusion"], out.get("vq"), rt=voices[0].rt)

    @staticmethod
    def blend(voices, weights, *, rt=None):
        """the convex combination sum_i w_i voice_i / sum_i w_i, member by member, on the pool kernel (weights >= 0, finite, sum > 0;
        they are normalised by their sum).  Voices of one S and one set of members; rt: the Runtime that launches (default: the one
        that made the first voice)."""
        voices = list(voices)
        if not voices:
            raise ValueError("Voice.blend: no voices")
        w = check_weights(np.asarray(weights, np.float64).reshape(1, -1), 1, len(voices))
        S, dims = voices[0].S, voices[0].dims
        for v in voices[1:]:
            if v.S != S or v.dims != dims:
                raise ValueError(f"Voice.blend: voices of different shapes ({v.S} x {v.dims} against {S} x {dims})")
        rt = voices[0].rt if rt is None else rt
        if rt is None:
            raise ValueError("Voice.blend: these voices were put together by hand - pass rt= (a model's .rt), which launches the pool")
        ws = np.repeat(w, S, 0)
        out = {k: rt.voice_pool(torch.stack([getattr(v, k) for v in voices], 1).contiguous(), ws) for k, _ in voices[0].members()}
        return Voice(out["gpt"], out["diffusion"], out.get("vq"), rt=rt)


def check_speaker(speaker, refer, refer_lengths, B, dims=None):
    """a synthesis entry's (speaker, refer, refer_lengths): exactly one of speaker / refer, refer_lengths only with refer, S in {1, B},
    the model's widths.  ValueError before any launch."""
    if speaker is not None and (refer is not None or refer_lengths is not None):
        raise ValueError("`speaker` and `refer` / `refer_lengths` are both given: a request names its speaker once")
    if speaker is None and refer is None:
        raise ValueError("neither `speaker` nor `refer` is given")
    if speaker is None:
        return
    if not isinstance(speaker, Voice):
        raise ValueError(f"`speaker` has to be a Voice (model.get_conditioning_latents), not {type(speaker).__name__}")
    if speaker.S not in (1, int(B)):
        raise ValueError(f"`speaker` holds {speaker.S} speakers for {B} rows: S has to be 1 (one voice, many texts) or B")
    if dims is not None:
        speaker.check_dims(dims)


def make_voice(rt, refer, S, n, T, lens):
    """SynthesizerTrn.get_conditioning_latents behind check_clips: refer [S,128,T] or [S,n,128,T] -> Voice.  Three encoder passes over
    the S n clips as one ragged batch (the launches every request made so far), then for n > 1 one pool launch per member."""
    x = torch.as_tensor(refer).to(rt.device, torch.float32).reshape(S * n, -1, T).contiguous()
    g = rt.mel_style("gpt.conditioning_encoder", x, lens)
    d = rt.diff_conditioning(x, lens)
    q = rt.mel_style("vq_ref_enc", x, lens) if rt.has_tensor("vq_ref_enc.") else None
    if n > 1:
        g = rt.voice_pool(g.view(S, n, -1))
        d = rt.voice_pool(d.view(S, n, -1), np.asarray([embedder_length(l) for l in lens], np.float32).reshape(S, n))
        q = None if q is None else rt.voice_pool(q.view(S, n, -1))
    return Voice(g, d, q, rt=rt)
