"""Drop-in for the reference's ``pytorch_version/loss_functions.py`` (single-scale API of
``unsupervise.py``) on MI355X: each loss is a fused HIP kernel pair (forward / backward)."""
import torch

from dvf import lib as _L
from dvf.ops import PhotoLossFn, SmoothLossFn
from inverse_warp import inverse_warp, check_sizes  # noqa: F401  (re-exported like the reference's copy)


def photometric_reconstruction_loss(img_R2, img_R1, img_L2, depth, T_2to1, T_R2L, intrinsics, intrinsics_inv,
                                    rotation_mode='euler', padding_mode='zeros', align_corners=False, img_scale=1.0,
                                    ssim_weight=0.0, ssim_c1=1e-4, ssim_c2=9e-4):
    """Temporal (img_R1 warped with T_2to1) + stereo (img_L2 warped with T_R2L) masked L1 against img_R2
    (reference loss_functions.py:7-20).  Works for images (C=3) and 32-channel feature maps alike; grads
    flow to depth, both poses and any image/feature input that requires them.
    ``img_scale`` (extension, default 1): the three images are used as img_scale * img inside the kernel -- the
    reference's call site passes 0.004 * img (unsupervise.py:101); this gives the same bits without the three
    scaled copies.
    ``ssim_weight`` (extension, default 0 = the reference's L1): a value a > 0 replaces |diff| by
    a * DSSIM + (1 - a) * |diff| (monodepth2 form; ``ssim_c1`` / ``ssim_c2`` must fit the range of img_scale * img).  The
    reference has no SSIM: parity unpinned.  Composition of one inverse warp per view and dvf.ops.SsimL1LossFn."""
    assert(intrinsics_inv.size() == intrinsics.size())
    flags = _L.geom_flags(rotation_mode, padding_mode, align_corners)
    if ssim_weight > 0:
        from dvf.ops import InverseWarpFn, SsimL1LossFn
        cfg = (float(img_scale), float(ssim_weight), float(ssim_c1), float(ssim_c2), None)
        loss = 0
        for src, T in ((img_R1, T_2to1), (img_L2, T_R2L)):
            warped = InverseWarpFn.apply(src, depth, T, intrinsics, intrinsics_inv, flags)
            loss = loss + SsimL1LossFn.apply(img_R2, warped, None, cfg)
        return loss
    pose = torch.stack((T_2to1, T_R2L), dim=0)                 # [V=2, B, 6]
    if img_scale != 1.0:
        flags = (flags, float(img_scale))
    return PhotoLossFn.apply(img_R2, depth, pose, intrinsics, intrinsics_inv, None, flags, img_R1, img_L2)


def smooth_loss(pred_map, scale_factor=1):
    """Second-order smoothness of one map or a list of maps (reference loss_functions.py:23-41)."""
    if type(pred_map) not in [tuple, list]:
        pred_map = [pred_map]
    return SmoothLossFn.apply(float(scale_factor), *pred_map)
