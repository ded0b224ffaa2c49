"""torch.autograd.Function wrappers over the C ABI: geometry + losses.

Each forward/backward is one (or two) kernel launches on torch's current stream; nothing here
synchronises with the host, so a whole training step can be captured in a HIP graph.
"""
import warnings

import torch

from . import conv as _conv
from . import lib as L
from .conv import _c

_WARNED_SRC_ATOMICS = False   # PhotoLossFn.backward: the deterministic-mode warning about source gradients has been given


def _grad_loss(gloss):
    """The gradient of a 0-dim loss as the [1] float32 tensor the backward kernels read."""
    return _c(gloss).reshape(1)


def as_list(x):
    """One map, or a tuple / list of maps (one per scale) as it is."""
    return x if type(x) in (tuple, list) else [x]


class InverseWarpFn(torch.autograd.Function):
    """inverse_warp.inverse_warp (reference pytorch_version/inverse_warp.py:160-193)."""

    @staticmethod
    def forward(ctx, img, depth, pose, K, Kinv, flags):
        img, depth, pose, K, Kinv = map(_c, (img, depth, pose, K, Kinv))
        B, C, H, W = img.shape
        out = torch.empty_like(img)
        L.check(L.lib().dvf_inverse_warp_fwd(L.dev(img, "img"), L.dev(depth, "depth"), L.dev(pose, "pose"),
                                             L.dev(K, "intrinsics"), L.dev(Kinv, "intrinsics_inv"), L.dev(out),
                                             B, C, H, W, flags, L.stream()), "dvf_inverse_warp_fwd")
        ctx.save_for_backward(img, depth, pose, K, Kinv)
        ctx.flags = flags
        return out

    @staticmethod
    def backward(ctx, gout):
        img, depth, pose, K, Kinv = ctx.saved_tensors
        B, C, H, W = img.shape
        need_img, need_depth, need_pose = ctx.needs_input_grad[:3]
        g_img = torch.zeros_like(img) if need_img else None
        g_depth = torch.empty_like(depth) if need_depth else None
        g_pose = torch.empty_like(pose) if need_pose else None
        lib = L.lib()
        # deterministic mode: the pose gradient's per-block partials go through a scratch and are added in block order
        ordered = _conv.DETERMINISTIC and need_pose
        bwd, what = (lib.dvf_inverse_warp_bwd_ordered, "dvf_inverse_warp_bwd_ordered") if ordered else \
            (lib.dvf_inverse_warp_bwd, "dvf_inverse_warp_bwd")
        ws_floats = lib.dvf_inverse_warp_ordered_ws_floats(B, H, W) if ordered else lib.dvf_pose_ws_floats(1, B)
        ws = torch.empty(int(ws_floats), device=img.device) if need_pose else None
        L.check(bwd(L.dev(img), L.dev(depth), L.dev(pose), L.dev(K), L.dev(Kinv), L.dev(_c(gout), "grad_out"), L.dev(g_img),
                    L.dev(g_depth), L.dev(g_pose), L.dev(ws), B, C, H, W, ctx.flags, L.stream()), what)
        return g_img, g_depth, g_pose, None, None, None


class PhotoLossFn(torch.autograd.Function):
    """Fused warp + exact-zero mask + (explainability mask) + L1 mean for all views of one scale.

    Inputs: tgt [B,C,H,W], depth [B,H,W], pose [V,B,6], K, Kinv [B,3,3], mask [B,V,H,W] or None,
    flags (int, or (int, in_scale): every image value is used as in_scale * x, the `0.004 * img` of
    unsupervise.py:101 without materialising scaled copies), then the V source tensors.
    Output: 0-dim loss (sum over views)."""

    @staticmethod
    def forward(ctx, tgt, depth, pose, K, Kinv, mask, flags, *srcs):
        flags, in_scale = flags if isinstance(flags, tuple) else (flags, 1.0)
        tgt, depth, pose, K, Kinv = map(_c, (tgt, depth, pose, K, Kinv))
        srcs = [_c(s) for s in srcs]
        mask = _c(mask) if mask is not None else None
        B, C, H, W = tgt.shape
        V = len(srcs)
        lib = L.lib()
        out = torch.empty(1 + V, device=tgt.device)
        partials = torch.empty(int(lib.dvf_photo_partials_floats(B, H, W, V)), device=tgt.device)
        # algorithmic bytes per target pixel: depth + C target + C*V sources (+ V masks)
        fwd_bytes = float(B * H * W) * (4 + 4 * C + 4 * C * V + (4 * V if mask is not None else 0))
        with L.timed("photo_fwd", 0.0, fwd_bytes):
            L.check(lib.dvf_photo_loss_fwd(L.dev(tgt, "tgt"), L.ptr_array(srcs, "srcs"), V, L.dev(depth, "depth"),
                                           L.dev(pose, "pose"), L.dev(K, "intrinsics"), L.dev(Kinv, "intrinsics_inv"),
                                           L.dev(mask, "mask"), L.dev(out), L.dev(out[1:]), L.dev(partials),
                                           B, C, H, W, in_scale, flags, L.stream()), "dvf_photo_loss_fwd")
        ctx.fwd_bytes = fwd_bytes
        ctx.save_for_backward(tgt, depth, pose, K, Kinv, mask, *srcs)
        ctx.flags, ctx.in_scale = flags, in_scale
        ctx.view_loss = out[1:]
        return out[0]

    @staticmethod
    def backward(ctx, gloss):
        tgt, depth, pose, K, Kinv, mask, *srcs = ctx.saved_tensors
        B, C, H, W = tgt.shape
        V = len(srcs)
        need = ctx.needs_input_grad
        lib = L.lib()
        g_tgt = torch.empty_like(tgt) if need[0] else None
        g_depth = torch.empty_like(depth) if need[1] else None
        g_pose = torch.empty_like(pose) if need[2] else None
        g_mask = torch.empty_like(mask) if (mask is not None and need[5]) else None
        g_srcs = [torch.zeros_like(s) if need[7 + i] else None for i, s in enumerate(srcs)]
        global _WARNED_SRC_ATOMICS
        if _conv.DETERMINISTIC and not _WARNED_SRC_ATOMICS and any(g is not None for g in g_srcs):
            _WARNED_SRC_ATOMICS = True
            warnings.warn("deterministic mode: the photometric backward sums the source-image gradients (the feature term's "
                          "feature maps) with float atomics, so the parameters trained through them are not bit-identical "
                          "from run to run", RuntimeWarning, stacklevel=2)
        ws = torch.empty(int(lib.dvf_photo_pose_ws_floats(B, H, W, V)), device=tgt.device) if need[2] else None
        gl = _grad_loss(gloss)
        # bwd = fwd (recompute) + grad depth + mask grads + grad target + RMW scatter into the source grads
        bwd_bytes = ctx.fwd_bytes + float(B * H * W) * (
            (4 if g_depth is not None else 0) + (4 * V if g_mask is not None else 0) +
            (4 * C if g_tgt is not None else 0) + 8 * C * sum(1 for g in g_srcs if g is not None))
        with L.timed("photo_bwd", 0.0, bwd_bytes):
            L.check(lib.dvf_photo_loss_bwd(L.dev(tgt), L.ptr_array(srcs), V, L.dev(depth), L.dev(pose), L.dev(K),
                                           L.dev(Kinv), L.dev(mask), L.dev(gl, "grad_loss"), L.dev(g_depth),
                                           L.dev(g_pose), L.dev(g_tgt), L.ptr_array(g_srcs), L.dev(g_mask), L.dev(ws),
                                           B, C, H, W, ctx.in_scale, ctx.flags, L.stream()), "dvf_photo_loss_bwd")
        return (g_tgt, g_depth, g_pose, None, None, g_mask, None, *g_srcs)


class SsimL1LossFn(torch.autograd.Function):
    """alpha * DSSIM + (1 - alpha) * L1 between a target and an already warped reference, exact-zero and explainability
    masked, mean over B*C*H*W (csrc/ssim_loss.hip; build-side extension, the reference has no SSIM).

    Inputs: tgt, warped [B,C,H,W]; mask None, [B,H,W] / [B,1,H,W], or [B,V,H,W] with a view index;
    cfg = (in_scale, alpha, c1, c2, view_index or None).  Output: 0-dim loss."""

    @staticmethod
    def forward(ctx, tgt, warped, mask, cfg):
        in_scale, alpha, c1, c2, view = cfg
        tgt, warped = _c(tgt), _c(warped)
        mask = _c(mask) if mask is not None else None
        B, C, H, W = tgt.shape
        if warped.shape != tgt.shape:
            raise ValueError(f"warped {tuple(warped.shape)} does not match target {tuple(tgt.shape)}")
        m_off, m_stride = 0, 0
        ctx.mask_shape = mask.shape if mask is not None else None
        if mask is not None:
            if mask.dim() == 3:
                mask = mask.unsqueeze(1)
            V = mask.shape[1]
            if tuple(mask.shape) != (B, V, H, W) or not 0 <= (view or 0) < V or (view is None and V != 1):
                raise ValueError(f"mask {tuple(mask.shape)} / view {view} does not match target {tuple(tgt.shape)}")
            m_off, m_stride = (view or 0) * H * W, V * H * W
        lib = L.lib()
        out = torch.empty(1, device=tgt.device)
        partials = torch.empty(int(lib.dvf_ssim_partials_floats(B, H, W)), device=tgt.device)
        fwd_bytes = float(B * H * W) * (8 * C + (4 if mask is not None else 0))
        m_ptr = L.dev(mask, "mask")
        with L.timed("ssim_fwd", 0.0, fwd_bytes):
            L.check(lib.dvf_ssim_loss_fwd(L.dev(tgt, "tgt"), L.dev(warped, "warped"), m_ptr + 4 * m_off if mask is not None else None,
                                          m_stride, L.dev(out), L.dev(partials), B, C, H, W, in_scale, alpha, c1, c2, 0,
                                          L.stream()), "dvf_ssim_loss_fwd")
        ctx.save_for_backward(tgt, warped, mask)
        ctx.cfg, ctx.m_off, ctx.m_stride, ctx.fwd_bytes = (in_scale, alpha, c1, c2), m_off, m_stride, fwd_bytes
        return out[0]

    @staticmethod
    def backward(ctx, gloss):
        tgt, warped, mask = ctx.saved_tensors
        B, C, H, W = tgt.shape
        need = ctx.needs_input_grad
        g_tgt = torch.empty_like(tgt) if need[0] else None
        g_warped = torch.empty_like(warped) if need[1] else None
        g_mask = None
        if mask is not None and need[2]:
            # the kernel writes the view it was given; the other views of a [B,V,H,W] mask get no gradient from this term
            g_mask = torch.empty_like(mask) if mask.shape[1] == 1 else torch.zeros_like(mask)
        in_scale, alpha, c1, c2 = ctx.cfg
        off = 4 * ctx.m_off
        bwd_bytes = ctx.fwd_bytes + float(B * H * W) * (4 * C * ((g_tgt is not None) + (g_warped is not None)) +
                                                        (4 if g_mask is not None else 0))
        with L.timed("ssim_bwd", 0.0, bwd_bytes):
            L.check(L.lib().dvf_ssim_loss_bwd(L.dev(tgt), L.dev(warped), L.dev(mask) + off if mask is not None else None,
                                              ctx.m_stride, L.dev(_grad_loss(gloss), "grad_loss"), L.dev(g_warped),
                                              L.dev(g_tgt), L.dev(g_mask) + off if g_mask is not None else None,
                                              B, C, H, W, in_scale, alpha, c1, c2, L.stream()), "dvf_ssim_loss_bwd")
        return g_tgt, g_warped, g_mask.reshape(ctx.mask_shape) if g_mask is not None else None, None


class MinReprojLossFn(torch.autograd.Function):
    """Per-pixel minimum over the reference views of alpha * DSSIM + (1 - alpha) * L1, with an optional identity-reprojection
    auto-mask (csrc/minreproj_loss.hip; build-side extension, monodepth2 form, nothing in the reference).

    ``apply(tgt, cfg, n_views, *cands)``: tgt [B,C,H,W]; cfg = (in_scale, alpha, c1, c2, auto_mask); cands = the n_views warped
    references (outputs of InverseWarpFn) and, with auto_mask, the n_views unwarped references in the same order.
    Returns (loss 0-dim, select uint8 [B,H,W] with 255 = no usable candidate, counts int32 [K+1], the last one "none");
    select and counts are not differentiable.  Gradients go to tgt and the warped candidates; an identity source must not
    require one."""

    @staticmethod
    def forward(ctx, tgt, cfg, n_views, *cands):
        in_scale, alpha, c1, c2, auto_mask = cfg
        V, K = int(n_views), len(cands)
        if not 1 <= V <= L.MAX_VIEWS:
            raise ValueError(f"n_views must be 1..{L.MAX_VIEWS}, got {V}")
        if K != (2 * V if auto_mask else V):
            raise ValueError(f"expected {2 * V if auto_mask else V} candidates for {V} views (auto_mask={bool(auto_mask)}), got {K}")
        for k, y in enumerate(cands):
            if y.shape != tgt.shape:
                raise ValueError(f"candidate {k} {tuple(y.shape)} does not match target {tuple(tgt.shape)}")
            if k >= V and ctx.needs_input_grad[3 + k]:
                raise ValueError(f"identity candidate {k} requires a gradient: the auto-mask sources are constants")
        tgt = _c(tgt)
        cands = [_c(y) for y in cands]
        B, C, H, W = tgt.shape
        lib = L.lib()
        dev = tgt.device
        out = torch.empty(1, device=dev)
        select = torch.empty((B, H, W), device=dev, dtype=torch.uint8)
        counts = torch.empty(K + 1, device=dev, dtype=torch.int32)
        partials = torch.empty(int(lib.dvf_minreproj_partials_floats(B, H, W, K)), device=dev)
        fwd_bytes = float(B * H * W) * (4 * C * (1 + K) + 1)         # target + K candidates read, selection written
        with L.timed("minreproj_fwd", 0.0, fwd_bytes):
            L.check(lib.dvf_minreproj_fwd(L.dev(tgt, "tgt"), L.ptr_array(cands, "cands"), V, int(bool(auto_mask)), L.dev(out),
                                          select.data_ptr(), counts.data_ptr(), L.dev(partials), B, C, H, W, in_scale, alpha,
                                          c1, c2, 0, L.stream()), "dvf_minreproj_fwd")
        ctx.save_for_backward(tgt, select, *cands)
        ctx.cfg, ctx.V, ctx.fwd_bytes = (in_scale, alpha, c1, c2, int(bool(auto_mask))), V, fwd_bytes
        ctx.mark_non_differentiable(select, counts)
        return out[0], select, counts

    @staticmethod
    def backward(ctx, gloss, _gselect, _gcounts):
        tgt, select, *cands = ctx.saved_tensors
        B, C, H, W = tgt.shape
        V = ctx.V
        need = ctx.needs_input_grad
        g_tgt = torch.empty_like(tgt) if need[0] else None
        g_warped = [torch.empty_like(cands[k]) if need[3 + k] else None for k in range(V)]
        in_scale, alpha, c1, c2, auto_mask = ctx.cfg
        n_grads = (g_tgt is not None) + sum(g is not None for g in g_warped)
        bwd_bytes = ctx.fwd_bytes + float(B * H * W) * 4 * C * n_grads
        with L.timed("minreproj_bwd", 0.0, bwd_bytes):
            L.check(L.lib().dvf_minreproj_bwd(L.dev(tgt), L.ptr_array(cands), V, auto_mask, select.data_ptr(),
                                              L.dev(_grad_loss(gloss), "grad_loss"), L.dev(g_tgt), L.ptr_array(g_warped),
                                              B, C, H, W, in_scale, alpha, c1, c2, L.stream()), "dvf_minreproj_bwd")
        return (g_tgt, None, None, *g_warped, *([None] * (len(cands) - V)))


class UpsampleIntFn(torch.autograd.Function):
    """Bilinear upsampling of x [B,C,H,W] by an integer ``factor`` (2, 4 or 8; F.interpolate(mode='bilinear',
    align_corners=False)), with ``recip_eps`` a float followed in the same pass by 1 / (. + recip_eps): a coarse disparity
    becomes a full-resolution depth and the upsampled disparity is never stored (csrc/upsample.hip; build-side extension,
    definition tests/fullres_ref.py).  ``recip_eps=None``: plain upsampling (explainability masks).  The backward is the
    exact transpose in gather form, bit-reproducible."""

    @staticmethod
    def forward(ctx, x, factor, recip_eps=None):
        x = _c(x)
        if x.dim() != 4:
            raise ValueError(f"expected a [B,C,H,W] map, got {tuple(x.shape)}")
        B, C, H, W = x.shape
        factor, recip = int(factor), recip_eps is not None
        out = torch.empty((B, C, factor * H, factor * W), device=x.device, dtype=torch.float32)
        with L.timed("upsample_int_fwd", 0.0, 4.0 * (x.numel() + out.numel())):
            L.check(L.lib().dvf_upsample_int_fwd(L.dev(x, "input"), L.dev(out), B * C, H, W, factor, int(recip),
                                                 float(recip_eps) if recip else 0.0, L.stream()), "dvf_upsample_int_fwd")
        if recip:
            ctx.save_for_backward(out)
        ctx.cfg = (B, C, H, W, factor, recip)
        return out

    @staticmethod
    def backward(ctx, gout):
        B, C, H, W, factor, recip = ctx.cfg
        out = ctx.saved_tensors[0] if recip else None
        gin = torch.empty((B, C, H, W), device=gout.device, dtype=torch.float32)
        with L.timed("upsample_int_bwd", 0.0, 4.0 * (gin.numel() + gout.numel() * (2 if recip else 1))):
            L.check(L.lib().dvf_upsample_int_bwd(L.dev(_c(gout), "grad_out"), L.dev(out), L.dev(gin), B * C, H, W, factor,
                                                 int(recip), L.stream()), "dvf_upsample_int_bwd")
        return gin, None, None


class SmoothLossFn(torch.autograd.Function):
    """smooth_loss over a list of maps (reference loss_functions.py:23-41, loss_functions_sfm.py:59-77):
    sum_s w_s * (mean|dx2| + mean|dxdy| + mean|dydx| + mean|dy2|), w_{s+1} = w_s / scale_factor."""

    @staticmethod
    def forward(ctx, scale_factor, *maps):
        maps = [_c(m) for m in maps]
        lib = L.lib()
        out = torch.empty(1, device=maps[0].device)
        weights, w = [], 1.0
        for i, m in enumerate(maps):
            B, C, H, W = m.shape
            partials = torch.empty(int(lib.dvf_smooth_partials_floats(B * C, H, W)), device=m.device)
            L.check(lib.dvf_smooth_loss_fwd(L.dev(m, "pred_map"), L.dev(out), L.dev(partials), B * C, H, W, w,
                                            1 if i > 0 else 0, L.stream()), "dvf_smooth_loss_fwd")
            weights.append(w)
            w /= scale_factor
        ctx.save_for_backward(*maps)
        ctx.weights = weights
        return out[0]

    @staticmethod
    def backward(ctx, gloss):
        maps = ctx.saved_tensors
        gl = _grad_loss(gloss)
        grads = []
        for i, (m, w) in enumerate(zip(maps, ctx.weights)):
            if not ctx.needs_input_grad[1 + i]:
                grads.append(None)
                continue
            B, C, H, W = m.shape
            g = torch.empty_like(m)
            L.check(L.lib().dvf_smooth_loss_bwd(L.dev(m), L.dev(gl, "grad_loss"), L.dev(g), B * C, H, W, w,
                                                L.stream()), "dvf_smooth_loss_bwd")
            grads.append(g)
        return (None, *grads)


class NormSmoothLossFn(torch.autograd.Function):
    """Edge-aware first-order smoothness of the mean-normalised disparity over a list of scales (csrc/norm_smooth.hip;
    build-side extension, monodepth2 form -- the reference has no such term, tests/normsmooth_ref.py is the definition):
    sum_s w_s * loss(disp_s, img_s), w_{s+1} = w_s / scale_factor, w_0 = 1.

    Inputs: cfg = (scale_factor, in_scale, eps), then the pairs disp_0, img_0, disp_1, img_1, ... with disp_s [B,1,H_s,W_s]
    and img_s [B,C,H_s,W_s].  Only the disparities receive a gradient.  Output: 0-dim loss."""

    @staticmethod
    def forward(ctx, cfg, *pairs):
        scale_factor, in_scale, eps = cfg
        if not pairs or len(pairs) % 2:
            raise ValueError("NormSmoothLossFn takes (disparity, image) pairs")
        disps, imgs = [_c(d) for d in pairs[0::2]], [_c(i) for i in pairs[1::2]]
        for d, i in zip(disps, imgs):
            if d.dim() != 4 or i.dim() != 4 or d.shape[1] != 1 or (d.shape[0],) + tuple(d.shape[2:]) != (i.shape[0],) + tuple(i.shape[2:]):
                raise ValueError(f"disparity {tuple(d.shape)} does not match image {tuple(i.shape)}")
        lib = L.lib()
        out = torch.empty(1, device=disps[0].device)
        weights, stats, w = [], [], 1.0
        for s, (d, i) in enumerate(zip(disps, imgs)):
            B, C, H, W = i.shape
            st = torch.empty(B, 2, device=d.device)
            partials = torch.empty(int(lib.dvf_norm_smooth_partials_floats(B, H, W)), device=d.device)
            with L.timed("normsmooth_fwd", 0.0, 4.0 * (1 + C) * B * H * W):
                L.check(lib.dvf_norm_smooth_fwd(L.dev(d, "disparity"), L.dev(i, "img"), L.dev(out), L.dev(st), L.dev(partials),
                                                B, C, H, W, in_scale, eps, w, 1 if s > 0 else 0, L.stream()),
                        "dvf_norm_smooth_fwd")
            weights.append(w)
            stats.append(st)
            w /= scale_factor
        ctx.save_for_backward(*disps, *imgs, *stats)
        ctx.cfg, ctx.weights = (in_scale, eps), weights
        return out[0]

    @staticmethod
    def backward(ctx, gloss):
        n = len(ctx.weights)
        saved = ctx.saved_tensors
        disps, imgs, stats = saved[:n], saved[n:2 * n], saved[2 * n:]
        in_scale, eps = ctx.cfg
        gl = _grad_loss(gloss)
        grads = []
        for s, (d, i, st, w) in enumerate(zip(disps, imgs, stats, ctx.weights)):
            if not ctx.needs_input_grad[1 + 2 * s]:
                grads += [None, None]
                continue
            B, C, H, W = i.shape
            g = torch.empty_like(d)
            with L.timed("normsmooth_bwd", 0.0, 4.0 * (2 + C) * B * H * W):
                L.check(L.lib().dvf_norm_smooth_bwd(L.dev(d), L.dev(i), L.dev(st), L.dev(gl, "grad_loss"), L.dev(g), B, C, H, W,
                                                    in_scale, eps, w, L.stream()), "dvf_norm_smooth_bwd")
            grads += [g, None]
        return (None, *grads)


class EdgeSmoothLossFn(torch.autograd.Function):
    """Edge-aware first-order smoothness of the inverse depth as the reference's Caffe graph defines it
    (experiments/depth_odometry_feature/train.prototxt:4452-4661): see csrc/paper_losses.hip."""

    @staticmethod
    def forward(ctx, inv_depth, img, in_scale, edge_k, weight):
        inv_depth, img = _c(inv_depth), _c(img)
        B, C, H, W = img.shape
        if tuple(inv_depth.shape) not in ((B, 1, H, W), (B, H, W)):
            raise ValueError(f"inv_depth {tuple(inv_depth.shape)} does not match image {tuple(img.shape)}")
        lib = L.lib()
        out = torch.empty(1, device=img.device)
        partials = torch.empty(int(lib.dvf_edge_smooth_partials_floats(B, H, W)), device=img.device)
        L.check(lib.dvf_edge_smooth_fwd(L.dev(inv_depth, "inv_depth"), L.dev(img, "img"), L.dev(out), L.dev(partials), B, C, H, W,
                                        in_scale, edge_k, weight, 0, L.stream()), "dvf_edge_smooth_fwd")
        ctx.save_for_backward(inv_depth, img)
        ctx.cfg = (in_scale, edge_k, weight)
        return out[0]

    @staticmethod
    def backward(ctx, gloss):
        inv_depth, img = ctx.saved_tensors
        B, C, H, W = img.shape
        g = torch.empty_like(inv_depth)
        in_scale, edge_k, weight = ctx.cfg
        L.check(L.lib().dvf_edge_smooth_bwd(L.dev(inv_depth), L.dev(img), L.dev(_grad_loss(gloss), "grad_loss"), L.dev(g),
                                            B, C, H, W, in_scale, edge_k, weight, L.stream()), "dvf_edge_smooth_bwd")
        return g, None, None, None, None


class ExplainabilityLossFn(torch.autograd.Function):
    """explainability_loss over a list of masks (reference loss_functions_sfm.py:49-56)."""

    @staticmethod
    def forward(ctx, *masks):
        masks = [_c(m) for m in masks]
        out = torch.empty(1, device=masks[0].device)
        partials = torch.empty(1024, device=masks[0].device)
        for i, m in enumerate(masks):
            L.check(L.lib().dvf_bce_ones_fwd(L.dev(m, "mask"), L.dev(out), L.dev(partials), m.numel(), 1 if i > 0 else 0,
                                             L.stream()), "dvf_bce_ones_fwd")
        ctx.save_for_backward(*masks)
        return out[0]

    @staticmethod
    def backward(ctx, gloss):
        gl = _grad_loss(gloss)
        grads = []
        for i, m in enumerate(ctx.saved_tensors):
            if not ctx.needs_input_grad[i]:
                grads.append(None)
                continue
            g = torch.empty_like(m)
            L.check(L.lib().dvf_bce_ones_bwd(L.dev(m), L.dev(gl, "grad_loss"), L.dev(g), m.numel(), L.stream()),
                    "dvf_bce_ones_bwd")
            grads.append(g)
        return tuple(grads)


class PoseVec2MatFn(torch.autograd.Function):
    """pose_vec2mat (reference inverse_warp.py:141-157): [n,6] -> [n,3,4]."""

    @staticmethod
    def forward(ctx, vec, flags):
        vec = _c(vec)
        n = vec.shape[0]
        out = torch.empty((n, 3, 4), device=vec.device, dtype=torch.float32)
        L.check(L.lib().dvf_pose_vec2mat_fwd(L.dev(vec, "vec"), L.dev(out), n, flags, L.stream()), "dvf_pose_vec2mat_fwd")
        ctx.save_for_backward(vec)
        ctx.flags = flags
        return out

    @staticmethod
    def backward(ctx, gmat):
        (vec,) = ctx.saved_tensors
        n = vec.shape[0]
        g = torch.empty_like(vec)
        ws = torch.empty(n * 12, device=vec.device)
        L.check(L.lib().dvf_pose_vec2mat_bwd(L.dev(vec), L.dev(_c(gmat), "grad_out"), L.dev(g), L.dev(ws), n, ctx.flags,
                                             L.stream()), "dvf_pose_vec2mat_bwd")
        return g, None


class Pixel2CamFn(torch.autograd.Function):
    """pixel2cam (reference inverse_warp.py:26-40)."""

    @staticmethod
    def forward(ctx, depth, Kinv):
        depth, Kinv = _c(depth), _c(Kinv)
        B, H, W = depth.shape
        cam = torch.empty((B, 3, H, W), device=depth.device, dtype=torch.float32)
        L.check(L.lib().dvf_pixel2cam_fwd(L.dev(depth, "depth"), L.dev(Kinv, "intrinsics_inv"), L.dev(cam), B, H, W,
                                          L.stream()), "dvf_pixel2cam_fwd")
        ctx.save_for_backward(Kinv)
        ctx.shape = (B, H, W)
        return cam

    @staticmethod
    def backward(ctx, gcam):
        (Kinv,) = ctx.saved_tensors
        B, H, W = ctx.shape
        g = torch.empty((B, H, W), device=gcam.device, dtype=torch.float32)
        L.check(L.lib().dvf_pixel2cam_bwd(L.dev(Kinv), L.dev(_c(gcam), "grad_out"), L.dev(g), B, H, W, L.stream()),
                "dvf_pixel2cam_bwd")
        return g, None


class Cam2PixelFn(torch.autograd.Function):
    """cam2pixel (reference inverse_warp.py:43-74): cam [B,3,H,W] -> normalised grid [B,H,W,2]."""

    @staticmethod
    def forward(ctx, cam, rot, tr, flags):
        cam = _c(cam)
        rot = _c(rot) if rot is not None else None
        tr = _c(tr).reshape(-1, 3) if tr is not None else None
        B, _, H, W = cam.shape
        grid = torch.empty((B, H, W, 2), device=cam.device, dtype=torch.float32)
        L.check(L.lib().dvf_cam2pixel_fwd(L.dev(cam, "cam_coords"), L.dev(rot, "proj_c2p_rot"), L.dev(tr, "proj_c2p_tr"),
                                          L.dev(grid), B, H, W, flags, L.stream()), "dvf_cam2pixel_fwd")
        ctx.save_for_backward(cam, rot, tr)
        ctx.flags = flags
        return grid

    @staticmethod
    def backward(ctx, ggrid):
        cam, rot, tr = ctx.saved_tensors
        B, _, H, W = cam.shape
        gcam = torch.empty_like(cam) if ctx.needs_input_grad[0] else None
        need_rt = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        ws = torch.empty((B, 12), device=cam.device) if need_rt else None
        L.check(L.lib().dvf_cam2pixel_bwd(L.dev(cam), L.dev(rot), L.dev(tr), L.dev(_c(ggrid), "grad_out"), L.dev(gcam),
                                          L.dev(ws), B, H, W, ctx.flags, L.stream()), "dvf_cam2pixel_bwd")
        g_rot = ws[:, 3:].reshape(B, 3, 3) if (rot is not None and ctx.needs_input_grad[1]) else None
        g_tr = ws[:, :3].reshape(B, 3, 1) if (tr is not None and ctx.needs_input_grad[2]) else None
        return gcam, g_rot, g_tr, None
