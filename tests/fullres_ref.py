"""Torch restatement of the full-resolution multi-scale sampling step (test infrastructure; imports nothing from the product).

The reference has no such mode, so this file IS the definition the HIP kernels (csrc/upsample.hip) are tested against:
plain tensor code, any dtype, gradients by autograd.  A coarse map [B,C,h,w] is brought to ``out_hw`` = (H, W) by

  upsample(x, out_hw)              = F.interpolate(x, out_hw, mode='bilinear', align_corners=False)
  upsample_depth(disp, out_hw, eps) = 1 / (upsample(disp, out_hw) + eps)

i.e. source coordinate (dst + 0.5) * h / H - 0.5 clamped at 0, the upper tap clamped to the last row / column.  A map that
already has the size ``out_hw`` passes through ``upsample`` unchanged (the weights are exactly 1 and 0).
"""
import torch.nn.functional as F


def upsample(x, out_hw):
    """[B,C,h,w] -> [B,C,H,W], bilinear, align_corners=False."""
    return F.interpolate(x, tuple(int(v) for v in out_hw), mode="bilinear", align_corners=False)


def upsample_depth(disp, out_hw, eps=0.0):
    """Depth at ``out_hw`` from a coarse disparity: the reciprocal is taken AFTER upsampling, at the fine resolution."""
    return 1.0 / (upsample(disp, out_hw) + eps)
