"""The photometric appearance term: warp V references into the target and compare.  Every loss file and step body reaches
PhotoLossFn / SsimL1LossFn / MinReprojLossFn (and InverseWarpFn, as a loss) through ``appearance_term`` and nowhere else."""
import torch

from .ops import InverseWarpFn, MinReprojLossFn, PhotoLossFn, SsimL1LossFn


def appearance_term(loss, tgt, refs, depth, poses, K, Kinv, flags, img_scale=1.0, mask=None, ssim_weight=0.0, ssim_c1=1e-4,
                    ssim_c2=9e-4, min_reprojection=False, auto_mask=False, selection_counts=None, pose_vb6=None):
    """``loss`` + the appearance term of one scale.  tgt [B,C,H,W]; V references; depth [B,H,W] or [B,1,H,W]; ``poses``: an
    iterable of V [B,6] vectors; K, Kinv [B,3,3]; ``flags``: dvf.lib's geometry bits; images enter as img_scale * x; mask [B,V,H,W].
      min_reprojection   V inverse warps + ONE MinReprojLossFn (the unwarped references compete under ``auto_mask``), whose
                         int32 [K+1] counts are appended to ``selection_counts`` if that is a list
      ssim_weight > 0    per view one inverse warp + SsimL1LossFn on the view's slice of the mask
      otherwise          ONE fused PhotoLossFn over [V,B,6] poses: ``pose_vb6`` if given (``poses`` is not touched), else stacked
    fp32 addition is not associative, so ``loss`` is the caller's running sum: the per-view terms join it one by one in view
    order (autograd runs the latest node first: also the order in which the views' depth gradients are summed) and a [B,1,H,W]
    depth is sliced anew for every warp.  None: no sum yet -- a single term is returned as it is, the per-view sum starts at 0."""
    poses = iter(poses)

    def plane():
        return depth[:, 0] if depth.dim() == 4 else depth

    def warp(ref):          # (the depth slice is made before the pose is taken: the order these nodes always had)
        return InverseWarpFn.apply(ref, plane(), next(poses), K, Kinv, flags)

    if min_reprojection:
        cfg = (float(img_scale), float(ssim_weight), float(ssim_c1), float(ssim_c2), bool(auto_mask))
        term, _, counts = MinReprojLossFn.apply(tgt, cfg, len(refs), *[warp(ref) for ref in refs], *(refs if auto_mask else ()))
        if selection_counts is not None:
            selection_counts.append(counts)
    elif ssim_weight > 0:
        loss = 0 if loss is None else loss
        for v, ref in enumerate(refs):
            cfg = (float(img_scale), float(ssim_weight), float(ssim_c1), float(ssim_c2), v if mask is not None else None)
            loss = loss + SsimL1LossFn.apply(tgt, warp(ref), mask, cfg)
        return loss
    else:
        if pose_vb6 is None:
            pose_vb6 = torch.stack(tuple(poses), dim=0)
        term = PhotoLossFn.apply(tgt, plane(), pose_vb6, K, Kinv, mask, (flags, float(img_scale)), *refs)
    return term if loss is None else loss + term
