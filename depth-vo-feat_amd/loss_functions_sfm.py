"""Drop-in for the reference's ``pytorch_version/loss_functions_sfm.py`` (multi-scale API of ``train.py``)."""
import torch

from dvf import lib as _L
from dvf.appearance import appearance_term
from dvf.conv import area_downsample, reciprocal
from dvf.ops import ExplainabilityLossFn, NormSmoothLossFn, SmoothLossFn, UpsampleIntFn, as_list


def photometric_reconstruction_loss(tgt_img, ref_imgs, intrinsics, intrinsics_inv, depth, explainability_mask, pose,
                                    rotation_mode='euler', padding_mode='zeros', align_corners=False,
                                    check_nan=False, ssim_weight=0.0, ssim_c1=1e-4, ssim_c2=9e-4, min_reprojection=False,
                                    auto_mask=False, selection_counts=None):
    """Sum over scales and reference views of the masked, explainability-weighted L1 between the target and
    the inverse-warped references (reference loss_functions_sfm.py:9-46).  One fused kernel per scale handles
    all views.  The reference's per-view NaN assert (:34) forces a device sync per view per scale; here it is
    opt-in (``check_nan=True``) and done once on the summed loss.
    ``ssim_weight`` (extension, default 0 = the reference's L1): a value a > 0 replaces |diff| by
    a * DSSIM + (1 - a) * |diff| (monodepth2 form: 3x3 reflected windows, ``ssim_c1`` / ``ssim_c2`` for images in [-1, 1]).
    The reference has no SSIM, so parity of this term is unpinned.  It is a composition, not the fused kernel: per scale and
    view one inverse warp materialises the warped image, then dvf.ops.SsimL1LossFn.
    ``min_reprojection`` (extension, default off): the appearance term a * DSSIM + (1 - a) * L1 (a = ``ssim_weight``, 0
    allowed) is reduced per pixel by the MINIMUM over the views instead of their sum, and with ``auto_mask`` the unwarped
    references compete as well, so a pixel that does not move between frames is won by an identity candidate and pulls on
    no depth (definition: tests/minreproj_ref.py; dvf.ops.MinReprojLossFn, one call per scale over all views).  The
    explainability mask is not part of this mode: every mask must be None.  ``selection_counts``: a list that receives, per
    scale, the int32 [K+1] tensor of pixels won by each candidate (the last entry: no usable candidate).
    Full-resolution multi-scale sampling (extension, monodepth2 form) needs no keyword here: ``downscale`` comes from each
    depth map's own size and ``area_downsample`` returns its input when the sizes agree, so a list of depths (and masks)
    that ``full_resolution`` brought to the input resolution runs every mode above at that resolution for every scale."""
    if auto_mask and not min_reprojection:
        raise ValueError("auto_mask needs min_reprojection=True")
    explainability_mask, depth = as_list(explainability_mask), as_list(depth)
    assert(pose.size(1) == len(ref_imgs))
    if min_reprojection and any(m is not None for m in explainability_mask):
        raise ValueError("min_reprojection does not take an explainability mask: pass None for every scale")
    flags = _L.geom_flags(rotation_mode, padding_mode, align_corners)
    pose_vb6 = pose.transpose(0, 1).contiguous()                        # [V, B, 6]
    loss = 0
    for d, mask in zip(depth, explainability_mask):
        assert(mask is None or d.size()[2:] == mask.size()[2:])
        b, _, h, w = d.size()
        downscale = tgt_img.size(2) / h
        tgt_s = area_downsample(tgt_img, (h, w))                         # :18
        refs_s = [area_downsample(r, (h, w)) for r in ref_imgs]          # :19
        k_s = torch.cat((intrinsics[:, 0:2] / downscale, intrinsics[:, 2:]), dim=1)               # :20
        kinv_s = torch.cat((intrinsics_inv[:, :, 0:2] * downscale, intrinsics_inv[:, :, 2:]), dim=2)   # :21
        loss = appearance_term(loss, tgt_s, refs_s, d, (pose[:, v] for v in range(len(refs_s))), k_s, kinv_s, flags,
                               1.0, mask, ssim_weight, ssim_c1, ssim_c2, min_reprojection, auto_mask, selection_counts,
                               pose_vb6=pose_vb6)
    if check_nan:
        assert((loss == loss).item() == 1)
    return loss


def full_resolution(maps, out_hw, recip_eps=None):
    """The maps of a coarse-to-fine list brought to ``out_hw`` = (H, W) for full-resolution multi-scale sampling (extension;
    definition tests/fullres_ref.py): every [B,C,h,w] map with H / h = W / w in {1, 2, 4, 8} is upsampled bilinearly
    (align_corners=False) by dvf.ops.UpsampleIntFn; with ``recip_eps`` a float the result is 1 / (upsampled + recip_eps),
    disparity -> depth, fused into the same pass.  A map already at (H, W) is returned as it is (through ``reciprocal``
    with ``recip_eps``).  Gradients reach the coarse maps.  Any other size ratio raises ValueError.  Returns a list."""
    H, W = int(out_hw[0]), int(out_hw[1])
    maps = as_list(maps)
    factors = []
    for m in maps:                       # every size is checked before the first kernel runs
        h, w = m.shape[2:]
        f = H // h if h > 0 else 0
        if m.dim() != 4 or f not in (1, 2, 4, 8) or (f * h, f * w) != (H, W):
            raise ValueError(f"full_resolution: a map of size {tuple(m.shape)} does not reach {(H, W)} by a factor of 1, 2, 4 "
                             f"or 8 in both axes")
        factors.append(f)
    out = []
    for m, f in zip(maps, factors):
        if f == 1:
            out.append(m if recip_eps is None else reciprocal(m, recip_eps))
        else:
            out.append(UpsampleIntFn.apply(m, f, None if recip_eps is None else float(recip_eps)))
    return out


def explainability_loss(mask):
    """sum_s BCE(mask_s, 1)  (reference loss_functions_sfm.py:49-56)."""
    return ExplainabilityLossFn.apply(*as_list(mask))


def smooth_loss(pred_map, scale_factor):
    """Second-order smoothness over a list of maps, weight divided by ``scale_factor`` per scale (:59-77)."""
    return SmoothLossFn.apply(float(scale_factor), *as_list(pred_map))


def normalized_smooth_loss(disparities, tgt_img, scale_factor=2.0, img_scale=1.0, eps=1e-7):
    """Edge-aware first-order smoothness of the mean-normalised DISPARITY, weight divided by ``scale_factor`` per scale
    (extension, monodepth2 form; the reference has no such term: parity unpinned, tests/normsmooth_ref.py is the definition).
    Per scale: n = disp / (mean over the image of disp + eps); mean(exp(-mean_c |dx I|) |dx n|) + mean(exp(-mean_c |dy I|) |dy n|)
    with I = img_scale * tgt_img brought to the scale's size by ``area_downsample`` (a map at the image's own size takes the
    image as it is).  Only the disparities receive a gradient.  dvf.ops.NormSmoothLossFn: one forward pass and one backward
    launch per scale.  monodepth2 weighs the term with 1e-3."""
    pairs = []
    for d in as_list(disparities):
        pairs += [d, area_downsample(tgt_img, tuple(d.shape[2:]))]
    return NormSmoothLossFn.apply((float(scale_factor), float(img_scale), float(eps)), *pairs)


@torch.no_grad()
def compute_errors(gt, pred, crop=True):
    """Evaluation-only depth metrics, same contract as the reference helper (loss_functions_sfm.py:80-116):
    per sample, valid = 0 < gt < 80 (inside the Garg/Eigen crop when ``crop``), prediction clamped to
    [1e-3, 80] and median-scaled to the ground truth; returns batch means of
    [abs_diff, abs_rel, sq_rel, a1, a2, a3].  Plain tensor code, not on the training hot path."""
    n, h, w = gt.shape
    region = torch.ones(h, w, dtype=torch.bool, device=gt.device)
    if crop:
        region[:] = False
        region[int(0.40810811 * h):int(0.99189189 * h), int(0.03594771 * w):int(0.96405229 * w)] = True
    totals = torch.zeros(6, dtype=torch.float64)
    for g_i, p_i in zip(gt, pred):
        keep = (g_i > 0) & (g_i < 80) & region
        g, p = g_i[keep], p_i[keep].clamp(1e-3, 80)
        p = p * (g.median() / p.median())
        ratio = torch.maximum(g / p, p / g)
        err = (g - p).abs()
        row = [err.mean(), (err / g).mean(), (err * err / g).mean()] + [(ratio < 1.25 ** e).float().mean() for e in (1, 2, 3)]
        totals += torch.stack([r.double().cpu() for r in row])
    return (totals / n).tolist()


@torch.no_grad()
def compute_errors_device(gt, pred, crop=True):
    """``compute_errors`` on the device: the same six batch means [abs_diff, abs_rel, sq_rel, a1, a2, a3] from one
    ``dvf.metrics.depth_metrics`` call (a few launches for the whole batch, exact lower median, no boolean gather, no sort)
    and ONE host transfer, the ``.tolist()`` below.  Like the reference it divides by the batch size: an image without a
    valid pixel contributes zeros here, where ``compute_errors`` fails on the median of an empty tensor."""
    from dvf.metrics import depth_metrics
    rows = depth_metrics(gt, pred, crop=crop)
    return (rows[:, [0, 1, 2, 5, 6, 7]].double().sum(0) / gt.shape[0]).tolist()
