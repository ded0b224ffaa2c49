"""Drop-in for the reference's ``pytorch_version/loss_functions.py`` (single-scale API of
``unsupervise.py``) on MI355X: each loss is a fused HIP kernel pair (forward / backward)."""
from dvf import lib as _L
from dvf.appearance import appearance_term
from dvf.ops import NormSmoothLossFn, SmoothLossFn, as_list
from inverse_warp import inverse_warp, check_sizes  # noqa: F401  (re-exported like the reference's copy)


def photometric_reconstruction_loss(img_R2, img_R1, img_L2, depth, T_2to1, T_R2L, intrinsics, intrinsics_inv,
                                    rotation_mode='euler', padding_mode='zeros', align_corners=False, img_scale=1.0,
                                    ssim_weight=0.0, ssim_c1=1e-4, ssim_c2=9e-4, min_reprojection=False, auto_mask=False,
                                    selection_counts=None):
    """Temporal (img_R1 warped with T_2to1) + stereo (img_L2 warped with T_R2L) masked L1 against img_R2
    (reference loss_functions.py:7-20).  Works for images (C=3) and 32-channel feature maps alike; grads
    flow to depth, both poses and any image/feature input that requires them.
    ``img_scale`` (extension, default 1): the three images are used as img_scale * img inside the kernel -- the
    reference's call site passes 0.004 * img (unsupervise.py:101); this gives the same bits without the three
    scaled copies.
    ``ssim_weight`` (extension, default 0 = the reference's L1): a value a > 0 replaces |diff| by
    a * DSSIM + (1 - a) * |diff| (monodepth2 form; ``ssim_c1`` / ``ssim_c2`` must fit the range of img_scale * img).  The
    reference has no SSIM: parity unpinned.  Composition of one inverse warp per view and dvf.ops.SsimL1LossFn.
    ``min_reprojection`` (extension, default off): the per-pixel MINIMUM over the two views of a * DSSIM + (1 - a) * L1
    (a = ``ssim_weight``, 0 allowed) instead of their sum; with ``auto_mask`` the unwarped img_R1 / img_L2 compete too
    (tests/minreproj_ref.py; dvf.ops.MinReprojLossFn).  ``selection_counts``: a list that receives the int32 [K+1] tensor of
    pixels won by each candidate (temporal, stereo, then the two identities; last entry: no usable candidate)."""
    assert(intrinsics_inv.size() == intrinsics.size())
    if auto_mask and not min_reprojection:
        raise ValueError("auto_mask needs min_reprojection=True")
    return appearance_term(None, img_R2, (img_R1, img_L2), depth, (T_2to1, T_R2L), intrinsics, intrinsics_inv,
                           _L.geom_flags(rotation_mode, padding_mode, align_corners), img_scale, None, ssim_weight, ssim_c1,
                           ssim_c2, min_reprojection, auto_mask, selection_counts)


def smooth_loss(pred_map, scale_factor=1):
    """Second-order smoothness of one map or a list of maps (reference loss_functions.py:23-41)."""
    return SmoothLossFn.apply(float(scale_factor), *as_list(pred_map))


def normalized_smooth_loss(disp, img, img_scale=1.0, eps=1e-7):
    """Edge-aware first-order smoothness of the mean-normalised disparity, single scale (extension, monodepth2 form; the
    reference has no such term: parity unpinned, tests/normsmooth_ref.py is the definition): with n = disp / (mean over the
    image of disp + eps) and I = img_scale * img, mean(exp(-mean_c |dx I|) |dx n|) + mean(exp(-mean_c |dy I|) |dy n|).
    disp [B,1,H,W], img [B,C,H,W]; only disp receives a gradient.  monodepth2 weighs the term with 1e-3."""
    return NormSmoothLossFn.apply((1.0, float(img_scale), float(eps)), disp, img)
