"""feature_loss / discriminator_loss / generator_loss / kl_loss mirrors (reference: vqvae/modules/losses.py), forward values on the device.

Every mean of one call is taken by one fixed-order reduction (dtts_disc_losses: per-block fp32 partials, then fp64 in index order; two
calls give the same bits) and the sums over the lists are taken in list order in fp32, as the reference's `loss += ...` does.  The
tensors are CUDA fp32 on one device; a (real, generated) pair must have one shape.  The handle comes from `rt=` or, by default, from
the Runtime that last bound a discriminator on the tensors' device (the entries of this stage run only on such a handle)."""
from __future__ import annotations

import torch

from ... import _lib
from ...runtime import DttsError, Runtime

def _rt(rt, t):
    if rt is not None:
        return rt.rt if hasattr(rt, "rt") else rt
    ref = Runtime.last_bound_disc.get(str(torch.device(t.device.type, t.device.index or 0)))
    found = ref() if ref is not None else None
    if found is None:
        raise DttsError("discriminators.0.convs.0.weight is not bound on this device: the loss functions run on the handle a "
                        "MultiPeriodDiscriminator is bound to (or pass rt=)")
    return found


def _dense(t):
    """t's elements fill one gap-free block of memory (any permutation of a contiguous tensor)"""
    n = 1
    for size, stride in sorted(zip(t.shape, t.stride()), key=lambda p: p[1]):
        if size == 1:
            continue
        if stride != n:
            return False
        n *= size
    return True


def _pair(r, g):
    """a pair whose mean |r - g| may be taken over the storage: both dense with one set of strides; anything else is copied"""
    if r.shape != g.shape:
        raise ValueError(f"feature_loss: a real map {list(r.shape)} and its generated map {list(g.shape)} must have one shape")
    r, g = _cuda(r), _cuda(g)
    if r.stride() == g.stride() and _dense(r):
        return r, g
    return r.contiguous(), g.contiguous()


def _cuda(t):
    t = torch.as_tensor(t)
    if not t.is_cuda:
        raise DttsError("the loss functions run on the device: CUDA tensors only (there is no CPU path)")
    return t.detach().float()


def _score(t):
    t = _cuda(t)
    return t if _dense(t) else t.contiguous()


def feature_loss(fmap_r, fmap_g, *, rt=None):
    """2 * sum over every map of mean |r - g| (vqvae/modules/losses.py:4-12) -> 0-d fp32 CUDA tensor; one launch covers all maps"""
    pairs = [_pair(rl, gl) for dr, dg in zip(fmap_r, fmap_g) for rl, gl in zip(dr, dg)]
    out = _rt(rt, pairs[0][0]).disc_losses([p[0] for p in pairs], [p[1] for p in pairs])
    return out[_lib.DISC_LOSS_FM]


def discriminator_loss(disc_real_outputs, disc_generated_outputs, *, rt=None):
    """(sum of mean (1 - dr)^2 + mean dg^2, r_losses, g_losses) (vqvae/modules/losses.py:15-28): a 0-d fp32 CUDA tensor and two lists
    of Python floats (the reference's .item(): one read-back for both lists)"""
    dr, dg = [_score(t) for t in disc_real_outputs], [_score(t) for t in disc_generated_outputs]
    out = _rt(rt, dg[0]).disc_losses(scores_r=dr, scores_g=dg)
    n = len(dg)
    host = out[_lib.DISC_LOSSES_R:_lib.DISC_LOSSES_G + _lib.DISC_COUNT].tolist()
    return out[_lib.DISC_LOSS_DISC], host[:n], host[_lib.DISC_COUNT:_lib.DISC_COUNT + n]


def generator_loss(disc_outputs, *, rt=None):
    """(sum of mean (1 - dg)^2, gen_losses) (vqvae/modules/losses.py:31-40): 0-d fp32 CUDA tensors, as the reference returns them"""
    dg = [_score(t) for t in disc_outputs]
    out = _rt(rt, dg[0]).disc_losses(scores_g=dg)
    return out[_lib.DISC_LOSS_GEN], [out[_lib.DISC_LOSSES_GEN + k] for k in range(len(dg))]


def kl_loss(z_p, logs_q, m_p, logs_p, z_mask, *, rt=None):
    """vqvae/modules/losses.py:43-58 through the existing kernel (dtts_kl_loss); z_mask [B,1,T] must be a sequence mask"""
    ts = [_cuda(a).contiguous() for a in (z_p, logs_q, m_p, logs_p)]
    B, _, T = ts[0].shape
    m = torch.as_tensor(z_mask).to(ts[0].device).reshape(B, T) != 0
    lens = m.sum(1)
    if not torch.equal(m, torch.arange(T, device=m.device)[None, :] < lens[:, None]):
        raise ValueError("kl_loss: z_mask must be a sequence mask (ones up to each row's length, then zeros)")
    return _rt(rt, ts[0]).kl_loss(*ts, [int(v) for v in lens.tolist()])
