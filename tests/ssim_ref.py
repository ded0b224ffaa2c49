"""Torch restatement of the SSIM + L1 appearance term (test infrastructure; imports nothing from the product).

The reference has no SSIM, so this file IS the definition the HIP kernels (csrc/ssim_loss.hip) are tested against:
plain tensor code, any dtype, gradients by autograd.  For target ``x`` and warped reference ``y`` [B,C,H,W]
(both already multiplied by ``in_scale``):

  3x3 window, uniform weights 1/9, reflection border (index -1 -> 1, H -> H-2; same for W);
  variances in the centred form mean((x - mu_x)^2) (the E[x^2] - mu^2 form loses ~10x more to cancellation in fp32);
  SSIM  = ((2 mu_x mu_y + c1)(2 s_xy + c2)) / ((mu_x^2 + mu_y^2 + c1)(s_x^2 + s_y^2 + c2));
  dssim = clamp((1 - SSIM) / 2, 0, 1);
  term  = alpha * dssim + (1 - alpha) * |x - y|;
  valid = 1 - prod_c [y_c == 0] (the reference's exact-zero mask, oracle/losses.py::_valid_mask), no gradient;
  loss  = mean over B*C*H*W of term * valid * m   (m: optional [B,1,H,W] explainability mask; masked pixels stay in
          the denominator).
"""
import torch
import torch.nn.functional as F


def windows(t):
    """[B,C,H,W] -> [B,C,H,W,9]: the 3x3 neighbourhood of every pixel under a reflection border."""
    p = F.pad(t, (1, 1, 1, 1), mode="reflect")
    return p.unfold(2, 3, 1).unfold(3, 3, 1).reshape(*t.shape, 9)


def dssim(x, y, c1=1e-4, c2=9e-4):
    wx, wy = windows(x), windows(y)
    mx, my = wx.mean(-1), wy.mean(-1)
    dx, dy = wx - mx.unsqueeze(-1), wy - my.unsqueeze(-1)
    vx, vy, cxy = (dx * dx).mean(-1), (dy * dy).mean(-1), (dx * dy).mean(-1)
    ssim = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return ((1 - ssim) / 2).clamp(0, 1)


def valid_mask(y):
    return 1 - (y == 0).prod(1, keepdim=True).type_as(y)


def ssim_l1_loss(x, y, mask=None, alpha=0.85, c1=1e-4, c2=9e-4, in_scale=1.0):
    """mask: None or [B,1,H,W] (one view of the explainability mask)."""
    x, y = in_scale * x, in_scale * y
    term = alpha * dssim(x, y, c1, c2) + (1 - alpha) * (x - y).abs()
    term = term * valid_mask(y.detach())
    if mask is not None:
        term = term * mask.expand_as(term)
    return term.mean()
