"""Torch restatement of the per-pixel minimum-reprojection appearance term with identity auto-masking (test infrastructure;
imports ssim_ref and nothing from the product).

The reference has none of this, so this file IS the definition the HIP kernels (csrc/minreproj_loss.hip) are tested
against: plain tensor code, any dtype, gradients by autograd.  For a target ``x`` [B,C,H,W], ``V`` warped references and --
auto-masking -- the ``V`` unwarped ones (all used as ``in_scale * value``), the candidates y_k are the warped references
first, then the unwarped ones in the same order:

  e_k(p)  = mean over channels of alpha * dssim(x, y_k)(p) + (1 - alpha) * |x(p) - y_k(p)|      (ssim_ref.dssim)
  usable  : a warped candidate where ssim_ref.valid_mask is 1 (not exactly zero in all channels), an identity candidate
            everywhere; no gradient
  k*(p)   = the lowest index among the usable candidates that attain min_k e_k(p); 255 when none is usable
  loss    = mean over B*H*W of e_k*(p)(p), pixels without a usable candidate adding 0

The selection is piecewise constant: autograd sends each pixel's gradient through the selected candidate only.
"""
import torch

import ssim_ref

NONE = 255


def candidate_errors(x, warped, identity=(), alpha=0.85, c1=1e-4, c2=9e-4, in_scale=1.0):
    """(e [K,B,H,W], usable [K,B,H,W] bool) of the candidates ``list(warped) + list(identity)``."""
    x = in_scale * x
    e, usable = [], []
    for k, y in enumerate(list(warped) + list(identity)):
        y = in_scale * y
        e.append((alpha * ssim_ref.dssim(x, y, c1, c2) + (1 - alpha) * (x - y).abs()).mean(1))
        usable.append(ssim_ref.valid_mask(y.detach())[:, 0] > 0 if k < len(warped) else torch.ones_like(e[-1], dtype=torch.bool))
    return torch.stack(e), torch.stack(usable)


def select_lowest(e, usable):
    """uint8 [B,H,W]: the lowest usable index attaining the minimum of e over dim 0, NONE where nothing is usable."""
    masked = torch.where(usable, e.detach(), torch.full_like(e, float("inf")))
    best = masked.min(0).values
    select = torch.full(best.shape, NONE, dtype=torch.uint8, device=e.device)
    for k in reversed(range(e.shape[0])):
        select = torch.where(usable[k] & (masked[k] == best), torch.full_like(select, k), select)
    return select


def minreproj_loss(x, warped, identity=(), alpha=0.85, c1=1e-4, c2=9e-4, in_scale=1.0):
    """(loss, select): 0-dim loss and the uint8 [B,H,W] selection map (255 = no usable candidate)."""
    e, usable = candidate_errors(x, warped, identity, alpha, c1, c2, in_scale)
    select = select_lowest(e, usable)
    none = select == NONE
    picked = e.gather(0, select.masked_fill(none, 0).long().unsqueeze(0))[0]
    return torch.where(none, torch.zeros_like(picked), picked).mean(), select
