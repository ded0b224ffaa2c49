"""Torch restatement of the edge-aware smoothness of the mean-normalised disparity (test infrastructure; imports nothing from
the product).

The reference has no such term -- its smoothness is second-order on depth (loss_functions.py:23-41) or the Caffe graph's
un-normalised edge-aware one -- so this file IS the definition the HIP kernels (csrc/norm_smooth.hip) are tested against and
parity is unpinned: plain tensor code, any dtype, gradients by autograd.  With disp [B,1,H,W] and I = in_scale * img [B,C,H,W]:

  m_b  = mean over (H,W) of disp_b                       n = disp / (m_b + eps)
  wx   = exp(-mean_c |I[..., :, :-1] - I[..., :, 1:]|)   wy = exp(-mean_c |I[..., :-1, :] - I[..., 1:, :]|)
  loss = mean(wx * |n[..., :, :-1] - n[..., :, 1:]|) + mean(wy * |n[..., :-1, :] - n[..., 1:, :]|)

the two means running over B*H*(W-1) and B*(H-1)*W elements.  Only disp is meant to receive a gradient (the image is a
constant of the term); d|v|/dv at v = 0 is 0, torch's convention.
"""
import torch
import torch.nn.functional as F


def normalized_smooth_loss(disp, img, in_scale=1.0, eps=1e-7):
    """One scale: disp [B,1,H,W], img [B,C,H,W] -> 0-dim loss."""
    I = (in_scale * img).detach()
    n = disp / (disp.mean(dim=(2, 3), keepdim=True) + eps)
    wx = torch.exp(-(I[..., :, :-1] - I[..., :, 1:]).abs().mean(dim=1, keepdim=True))
    wy = torch.exp(-(I[..., :-1, :] - I[..., 1:, :]).abs().mean(dim=1, keepdim=True))
    return (wx * (n[..., :, :-1] - n[..., :, 1:]).abs()).mean() + (wy * (n[..., :-1, :] - n[..., 1:, :]).abs()).mean()


def multiscale_normalized_smooth_loss(disps, img, scale_factor=2.0, in_scale=1.0, eps=1e-7, weight=1.0):
    """sum_i weight / scale_factor^i * loss(disp_i, area_downsample(img, size of disp_i)); F.interpolate(mode='area') is the
    pyramid of loss_functions_sfm.py:18-19, and a map at the image's own size takes the image as it is."""
    total, w = 0, float(weight)
    for d in disps:
        hw = tuple(d.shape[2:])
        img_s = img if tuple(img.shape[2:]) == hw else F.interpolate(img, hw, mode="area")
        total = total + w * normalized_smooth_loss(d, img_s, in_scale, eps)
        w /= scale_factor
    return total
