"""The training-step bodies of the reference's entry scripts, on the HIP path.

  unsupervise_losses  unsupervise.py:83-111   img recon + 10*smooth (+ 0.1*feature recon), single scale
  train_sfm_losses    train.py:179-203        4-scale photometric with masks + w3*smooth + stereo-pose MSE
Each returns (total_loss, dict of detached per-term losses); the caller does zero_grad / backward / step.
No ``.item()`` here: the reference's 5 host syncs per step (train.py:205-209) are left to the logger."""

import torch

import loss_functions as LF
import loss_functions_sfm as LS
from dvf import lib as L
from dvf.appearance import appearance_term
from dvf.conv import reciprocal


POSE_STREAM = True       # the pose network runs on the auxiliary stream beside the depth network


def _side_by_side(aux_fn, main_fn):
    """Run two independent sub-networks concurrently: ``aux_fn`` (the small pose network) on a second stream, ``main_fn``
    (the depth network) on the current one.  The deep layers of either network launch fewer blocks than the GPU has
    CUs, so the two fill each other's gaps; autograd runs each backward on its forward stream, so the backward passes
    overlap too.  FlatAdam.step() joins the auxiliary stream (dvf/lib.py AUX_STREAMS).  ``POSE_STREAM = False`` (module
    attribute; tools set it, nothing on the product path reads the environment) puts both networks on one stream."""
    if L.SERIALIZE or not POSE_STREAM:
        # same HOST order as below (depth network first): the order in which gradient buckets become ready -- and with it
        # the order of the all-reduce calls -- must not depend on this switch (bench.py times rank 0 serialised while the
        # other ranks run the overlapped schedule: mismatched collective orders would hang RCCL)
        m_out = main_fn()
        return aux_fn(), m_out
    cur = torch.cuda.current_stream()
    aux = L.aux_stream(cur.device)
    aux.wait_stream(cur)
    # Host order: the depth network first, the pose network LAST.  Autograd runs ready nodes latest-created first, so the
    # pose network's whole backward pass is enqueued (on its own stream) before the depth network's and overlaps it from
    # the start; the other order leaves it -- and its weight gradients, Adam and repack -- as a serial tail of the step.
    m_out = main_fn()
    with torch.cuda.stream(aux):
        a_out = aux_fn()
    cur.wait_stream(aux)

    def _mark(t):
        if torch.is_tensor(t):
            t.record_stream(cur)          # produced on aux, consumed by the losses on the current stream
        elif isinstance(t, (list, tuple)):
            for x in t:
                _mark(x)
    _mark(a_out)
    return a_out, m_out


def _pose_only(pose_net, frames):
    """pose_net(frames) for a body that discards the explainability masks: a PoseExpNet is told not to compute them (its
    decoder is a third of the network's forward time and no gradient reaches it); any other module is called as it is."""
    from PoseExpNet_sfm import _PoseExpBase
    if isinstance(getattr(pose_net, "module", pose_net), _PoseExpBase):
        return pose_net(frames, need_masks=False)
    return pose_net(frames)


def _identity_share(counts, n_views):
    """Share of the pixels won by an identity candidate, from the selection counts of MinReprojLossFn (a handful of
    integers: no image-sized kernel)."""
    return counts[n_views:2 * n_views].sum() / counts.sum()


def _feature_maps(feat_extractor, L2, R2, R1, frozen=False):
    """One extractor pass over the three frames (unsupervise.py:104-107); ``frozen``: no graph, no weight gradients."""
    with torch.set_grad_enabled(torch.is_grad_enabled() and not frozen):
        feat = feat_extractor(torch.cat((L2, R2, R1), dim=0))
    b = R2.size(0)
    return feat[:b], feat[b:2 * b], feat[2 * b:]


def _smoothness(normalized, disparities, depths, img, scale_factor=1.0, img_scale=1.0):
    """Second-order smoothness of the depths, or ``normalized``: edge-aware first-order, of the mean-normalised disparities."""
    if normalized:
        return LS.normalized_smooth_loss(disparities, img, scale_factor, img_scale)
    return LS.smooth_loss(depths, scale_factor)


def unsupervise_losses(depth_net, pose_net, batch, feat_extractor=None, img_scale=0.004, smooth_weight=10.0,
                       feat_weight=0.1, depth_eps=1e-4, ssim_weight=0.0, ssim_c1=1e-4, ssim_c2=9e-4, min_reprojection=False,
                       auto_mask=False, normalized_smoothness=False):
    """unsupervise.py:83-111.  ssim_weight > 0 (extension): the image term becomes a * DSSIM + (1 - a) * L1; the feature
    term stays L1.  min_reprojection / auto_mask (extension): the image term takes the per-pixel minimum over the two
    views, with the unwarped references competing under auto_mask; terms["automask"] is then the share of pixels won by
    an identity candidate.  normalized_smoothness (extension, monodepth2 form): terms["smooth"] is the edge-aware first-order
    smoothness of the mean-normalised DISPARITY against img_scale * R2 (LF.normalized_smooth_loss) instead of the second-order
    smoothness of depth, under the same smooth_weight (monodepth2 uses 1e-3).  Off: nothing changes."""
    counts = []
    R2, R1, L2 = batch["img_R2"], batch["img_R1"], batch["img_L2"]
    # unsupervise.py:92,95 (cat(R2, R1) done virtually) and :94 (intended: finest disparity)
    (_, T_2to1), disps = _side_by_side(lambda: _pose_only(pose_net, (R2, R1)), lambda: depth_net(R2))
    inv_depth = disps[0]
    depth = reciprocal(inv_depth, depth_eps).squeeze(1)            # :99
    img_loss = LF.photometric_reconstruction_loss(R2, R1, L2, depth, T_2to1, batch["T_R2L"], batch["K"], batch["Kinv"],
                                                  img_scale=img_scale,   # :101 (0.004 * img applied inside the kernel)
                                                  ssim_weight=ssim_weight, ssim_c1=ssim_c1, ssim_c2=ssim_c2,
                                                  min_reprojection=min_reprojection, auto_mask=auto_mask,
                                                  selection_counts=counts)
    smooth = _smoothness(normalized_smoothness, inv_depth, depth.unsqueeze(1), R2, img_scale=img_scale)    # :102
    terms = {"img": img_loss.detach(), "smooth": smooth.detach()}
    if auto_mask:
        terms["automask"] = _identity_share(counts[0], 2)
    loss = img_loss + smooth_weight * smooth
    if feat_extractor is not None:
        f_L2, f_R2, f_R1 = _feature_maps(feat_extractor, L2, R2, R1)                               # :104-107
        feat_loss = LF.photometric_reconstruction_loss(f_R2, f_R1, f_L2, depth, T_2to1, batch["T_R2L"], batch["K"],
                                                       batch["Kinv"])                              # :109
        loss = img_loss + feat_weight * feat_loss + smooth_weight * smooth                          # :111
        terms["feat"] = feat_loss.detach()
    terms["total"] = loss.detach()
    return loss, terms


def depth_only_losses(depth_net, batch, img_scale=0.004, smooth_weight=10.0, depth_eps=1e-4):
    """BASELINE.json configs[0] (cfg 1): DispNetS alone with the stereo photometric loss (one view: the left image warped
    into the right one with the fixed baseline pose) + 10 * smooth -- unsupervise.py:94-102 without the pose network."""
    R2, L2 = batch["img_R2"], batch["img_L2"]
    depth = reciprocal(depth_net(R2)[0], depth_eps)                # [B,1,H,W]
    photo = appearance_term(None, R2, (L2,), depth.squeeze(1), (batch["T_R2L"],), batch["K"], batch["Kinv"], 0, img_scale,
                            pose_vb6=batch["T_R2L"].unsqueeze(0).contiguous())
    smooth = LF.smooth_loss(depth)
    loss = photo + smooth_weight * smooth
    return loss, {"img": photo.detach(), "smooth": smooth.detach(), "total": loss.detach()}


def train_sfm_losses(disp_net, pose_exp_net, batch, w1=1.0, w2=0.0, w3=0.1, smooth_factor=2.0,
                     rotation_mode="euler", padding_mode="zeros", feat_extractor=None, feat_weight=0.1,
                     ssim_weight=0.0, ssim_c1=1e-4, ssim_c2=9e-4, min_reprojection=False, auto_mask=False,
                     full_res_multiscale=False, normalized_smoothness=False):
    """train.py:179-203.  ssim_weight > 0 (extension): the 4-scale photometric term becomes a * DSSIM + (1 - a) * L1.
    min_reprojection / auto_mask (extension): the image term takes the per-pixel minimum over the views (the unwarped
    references competing under auto_mask) and no explainability mask, so w2 must be 0; terms["automask"] is the share of
    finest-scale pixels won by an identity candidate.  feat_extractor: BASELINE.json configs[3] (cfg 4) adds the feature-reconstruction term of
    unsupervise.py:104-111 (single scale, finest depth, the network's two poses) to the 4-scale body.
    full_res_multiscale (extension, monodepth2 form): every scale's disparity (and explainability mask) is upsampled
    bilinearly to the input resolution, turned into depth there (one fused pass, LS.full_resolution) and the photometric term
    of every scale warps the full-resolution references against the full-resolution target; gradients reach the coarse
    disparities and masks.  Smoothness, the explainability regulariser, the stereo-pose MSE and the feature term stay on the
    native-scale maps; terms["automask"] is still the finest scale's share.  Off: nothing changes.
    normalized_smoothness (extension, monodepth2 form): terms["smooth"] is the edge-aware first-order smoothness of the
    mean-normalised DISPARITIES of every scale at its native resolution, also under full_res_multiscale, against the target
    image (LS.normalized_smooth_loss) instead of the second-order smoothness of the depths, under the same w3 and
    smooth_factor (monodepth2 uses w3 = 1e-3).  Off: nothing changes."""
    if min_reprojection and w2 > 0:
        raise ValueError("min_reprojection leaves the explainability mask out of the photometric term: w2 must be 0")
    tgt = batch["img_R2"]
    refs = [batch["img_R1"], batch["img_L2"]] + list(batch.get("extra_refs", []))[: pose_exp_net.nb_ref_imgs - 2]
    (masks, pose), disparities = _side_by_side(lambda: pose_exp_net(tgt, refs), lambda: disp_net(tgt))   # train.py:187,189
    depth = [reciprocal(d, 0.0) for d in disparities]              # :188
    counts = []
    photo_depth, photo_masks = depth, masks
    if full_res_multiscale:
        hw = tgt.shape[2:]
        photo_depth = LS.full_resolution(disparities, hw, recip_eps=0.0)
        if not min_reprojection:
            photo_masks = LS.full_resolution(masks, hw)
    l1 = LS.photometric_reconstruction_loss(tgt, refs, batch["K"], batch["Kinv"], photo_depth,
                                            [None] * len(depth) if min_reprojection else photo_masks, pose,
                                            rotation_mode, padding_mode, ssim_weight=ssim_weight, ssim_c1=ssim_c1,
                                            ssim_c2=ssim_c2, min_reprojection=min_reprojection, auto_mask=auto_mask,
                                            selection_counts=counts)                               # :191
    l3 = _smoothness(normalized_smoothness, disparities, depth, tgt, smooth_factor)                # :200
    l4 = torch.nn.functional.mse_loss(pose[:, 1], batch["T_R2L"])  # :201  (24 floats: left to torch)
    loss = w1 * l1 + w3 * l3 + l4
    terms = {"photo": l1.detach(), "smooth": l3.detach(), "lr": l4.detach()}
    if auto_mask:
        terms["automask"] = _identity_share(counts[0], len(refs))
    if w2 > 0:
        l2 = LS.explainability_loss(masks)                         # :195-196
        loss = loss + w2 * l2
        terms["exp"] = l2.detach()
    if feat_extractor is not None:
        f_L2, f_R2, f_R1 = _feature_maps(feat_extractor, refs[1], tgt, refs[0])
        lf = LF.photometric_reconstruction_loss(f_R2, f_R1, f_L2, depth[0].squeeze(1), pose[:, 0], pose[:, 1], batch["K"],
                                                batch["Kinv"], rotation_mode, padding_mode)
        loss = loss + feat_weight * lf
        terms["feat"] = lf.detach()
    terms["total"] = loss.detach()
    return loss, terms


def unsupervise_dvo_losses(depth_net, pose_net, batch, img_scale=0.004, smooth_weight=10.0, depth_eps=1e-4,
                           normalized_smoothness=False):
    """unsupervise_dvo.py:83-122 (the Caffe-style chain): T = (T_R2L, T_2to1) as se(3) vectors -> exponential map
    (t = R u) -> GeoTransform -> PinHole -> InverseWarping in PIXEL coordinates -> exact-zero-masked L1 for the
    stereo (L2 -> R2) and temporal (R1 -> R2) warps + 10 * smooth(depth).  All of it is the fused warp kernel with the
    DVF_POSE_SE3 | DVF_PIXEL_COORDS front end.  batch["T_R2L"] must be in the se(3) order (w, u), i.e. (0,0,0,Tx,0,0)
    as the reference dataset writes it (data/dataset_builder.py:155).  normalized_smoothness (extension): as in
    unsupervise_losses."""
    R2, R1, L2 = batch["img_R2"], batch["img_R1"], batch["img_L2"]
    (_, T_2to1), disps = _side_by_side(lambda: _pose_only(pose_net, (R2, R1)), lambda: depth_net(R2))
    inv_depth = disps[0]
    depth = reciprocal(inv_depth, depth_eps)                               # [B,1,H,W]
    photo = appearance_term(None, R2, (L2, R1), depth.squeeze(1), (batch["T_R2L"], T_2to1), batch["K"], batch["Kinv"],
                            L.POSE_SE3 | L.PIXEL_COORDS, img_scale)        # view 0 = left image, view 1 = R1
    smooth = _smoothness(normalized_smoothness, inv_depth, depth, R2, img_scale=img_scale)
    loss = photo + smooth_weight * smooth
    return loss, {"photo": photo.detach(), "smooth": smooth.detach(), "total": loss.detach()}


def paper_losses(depth_net, pose_net, batch, feat_extractor=None, img_scale=0.004, smooth_weight=10.0, feat_weight=0.1,
                 depth_eps=1e-4):
    """The loss of the reference's Caffe experiment ``depth_odometry_feature`` (train.prototxt:4355-4367, 4428-4446,
    4452-4661, 5571-5588): AbsLoss warp errors of the left and of the previous right image under the
    se(3) / pixel-coordinate chain (weight 1 each), edge-aware first-order smoothness of the inverse depth (weight 10)
    and, with ``feat_extractor`` (frozen: its parameters must not require gradients), 0.1 * AbsLoss on warped
    feature maps.  batch["T_R2L_se3"] is the stereo pose as the dataset holds it."""
    import loss_functions_caffe as LC
    R2, R1, L2 = batch["img_R2"], batch["img_R1"], batch["img_L2"]
    (_, T_2to1), disps = _side_by_side(lambda: _pose_only(pose_net, (R2, R1)), lambda: depth_net(R2))
    inv_depth = disps[0]
    depth = reciprocal(inv_depth, depth_eps)                               # depth = (inv_depth + 1e-4)^-1  (:4355-4367)
    poses = (batch["T_R2L_se3"], T_2to1)
    photo = LC.abs_warp_loss(R2, (L2, R1), depth, poses, batch["K"], batch["Kinv"], img_scale=img_scale)
    smooth = LC.edge_aware_smooth_loss(inv_depth, R2, img_scale=img_scale)
    loss = photo + smooth_weight * smooth
    terms = {"photo": photo.detach(), "smooth": smooth.detach()}
    if feat_extractor is not None:
        f_L2, f_R2, f_R1 = _feature_maps(feat_extractor, L2, R2, R1, frozen=True)
        lf = LC.abs_warp_loss(f_R2, (f_L2, f_R1), depth, poses, batch["K"], batch["Kinv"])
        loss = loss + feat_weight * lf
        terms["feat"] = lf.detach()
    terms["total"] = loss.detach()
    return loss, terms
