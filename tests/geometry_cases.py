"""Inputs for the stand-alone geometry helpers of inverse_warp.py -- PoseVec2MatFn, Pixel2CamFn, Cam2PixelFn of dvf/ops.py
(tests/test_geometry_cases.py, tests/test_gpu_geometry_helpers.py).

Shapes: (1,2,2) the smallest legal image; (3,5,130); (2,91,91) = 8281 pixels per image, which dvf_cam2pixel_bwd splits into
chunks = ceil(8281 / 8192) = 2 blocks per image of per = 4141 pixels, the last one short (4140).

Families.  "front": depths in [2, 22] and small poses, as test_gpu_losses.py::test_geometry_helpers_vs_oracle.  "behind":
the translation has t_z = -2 and a lateral shift, and the depths come from two bands of [0.5, 4]: [0.5, 1.5] lands behind
the camera (p_z in about [-1.6, -0.4]: Z = max(p_z, 1e-3) and its gradient cut act) and [2.5, 4] in front of it with p_z of
0.4 or more.  The gap is on purpose.  d(x/Z)/dZ = -x / Z^2, and p_z = r . cam + t_z cancels two numbers of size 2 in fp32, an
absolute error near 2e-7: at p_z = 0.01 that alone is 2e-5 of Z and 4e-5 of the gradient, on the pixel that sets the
tensor's maximum, so a band of depths around 2 would measure fp32's conditioning and not the kernel.  Of the pixels in front
a share leaves [-1, 1] (the perspective magnifies by depth / p_z, 1.25 to 6) and a share stays.

Absent operands.  cam2pixel computes p = rot @ cam + tr with rot = K R and tr = K t.  The same p reaches the kernel through
fewer operands when the work is folded into the points: rot = None takes cam' = rot @ cam, tr = None takes cam' = cam + R^T t,
both None take cam' = p itself (operands()).  Each combination is rounded to fp32 on its own, and the determinacy checks of
tests/test_geometry_cases.py run on those fp32 operands in fp64, per combination."""
import types

import torch

from oracle import geometry as og

SHAPES = ((1, 2, 2), (3, 5, 130), (2, 91, 91))
FAMILIES = ("front", "behind")
COMBOS = ("rot+tr", "no_rot", "no_tr", "neither")
CHUNK = 8192                                    # pixels per block of cam2pixel_bwd_kernel at most (csrc/warp_loss.hip)
# seeds for which no coordinate lies near a decision (tests/test_geometry_cases.py asserts it); default 0
SEEDS = {((1, 2, 2), "behind"): 5, ((2, 91, 91), "front"): 23, ((2, 91, 91), "behind"): 2}


def kitti_K(b, h, w):
    K = torch.tensor([[0.58 * w, 0, 0.5 * w], [0, 1.92 * h, 0.5 * h], [0, 0, 1.0]]).expand(b, 3, 3).contiguous()
    return K, torch.inverse(K[0]).expand(b, 3, 3).contiguous()


def make(shape, family, seed=None):
    """One case (fp32, CPU): depth [B,H,W], K, Kinv, vec [B,6] (Euler), cam [B,3,H,W] = the fp64 pixel2cam rounded, the
    fp64 projection (rot64 [B,3,3], tr64 [B,3,1], R64, t64) and upstream gradients gg [B,H,W,2], gc [B,3,H,W]."""
    b, h, w = shape
    seed = SEEDS.get((shape, family), 0) if seed is None else seed
    gen = torch.Generator().manual_seed(10000 * h + 10 * w + b + 1000003 * seed + (5 if family == "behind" else 0))
    K, Kinv = kitti_K(b, h, w)
    if family == "front":
        depth = torch.rand(b, h, w, generator=gen) * 20 + 2
        vec = torch.randn(b, 6, generator=gen) * 0.04
    else:
        near = torch.rand(b, h, w, generator=gen) < 0.4
        near.view(b, -1)[:, 0], near.view(b, -1)[:, -1] = True, False            # both bands in every image, also at 2x2
        u = torch.rand(b, h, w, generator=gen)
        depth = torch.where(near, 0.5 + u, 2.5 + 1.5 * u)
        vec = torch.randn(b, 6, generator=gen) * 0.01
        # lateral shift, another per image.  Behind the camera p_x = u d + f_x t_x - 2 c_x up to the rotation (p_z = d - 2):
        # at most 1.5 (W - 1) - 0.58 W 1.1 - W < -0.13 W, and p_y <= 1.5 (H - 1) - 1.92 H 0.4 - H < -0.26 H: the clamped
        # point of every behind-camera pixel leaves the image on the low side of both axes, by far
        vec[:, 0] = -1.2 + 0.05 * torch.arange(b)
        vec[:, 1] = -0.4
        vec[:, 2] = -2.0
    case = types.SimpleNamespace(shape=shape, family=family, depth=depth, K=K, Kinv=Kinv, vec=vec)
    case.cam = og.pixel2cam(depth.double(), Kinv.double()).float().contiguous()
    pose = og.pose_vec2mat(vec.double(), "euler")
    proj = K.double() @ pose
    case.R64, case.t64 = pose[:, :, :3], pose[:, :, 3:]
    case.rot64, case.tr64 = proj[:, :, :3], proj[:, :, 3:]
    case.gg = torch.randn(b, h, w, 2, generator=gen)
    case.gc = torch.randn(b, 3, h, w, generator=gen)
    return case


def operands(case, combo):
    """(cam [B,3,H,W], rot [B,3,3] or None, tr [B,3,1] or None), fp32, for one operand combination (module docstring)."""
    b, h, w = case.shape
    cam = case.cam.double().reshape(b, 3, -1)
    if combo == "rot+tr":
        cam_in, rot, tr = cam, case.rot64, case.tr64
    elif combo == "no_rot":
        cam_in, rot, tr = case.rot64 @ cam, None, case.tr64
    elif combo == "no_tr":
        cam_in, rot, tr = cam + case.R64.transpose(1, 2) @ case.t64, case.rot64, None
    else:
        cam_in, rot, tr = case.rot64 @ cam + case.tr64, None, None
    f = lambda x: None if x is None else x.float().contiguous()
    return f(cam_in.reshape(b, 3, h, w)), f(rot), f(tr)


def project(cam, rot, tr):
    """fp64 from the fp32 operands: p [B,3,H,W], and x_n, y_n [B,H,W] before the zeros overwrite (Z clamped at 1e-3)."""
    b, _, h, w = cam.shape
    p = cam.double().reshape(b, 3, -1)
    if rot is not None:
        p = rot.double() @ p
    if tr is not None:
        p = p + tr.double().reshape(b, 3, 1)
    p = p.reshape(b, 3, h, w)
    Z = p[:, 2].clamp(min=1e-3)
    return p, 2 * (p[:, 0] / Z) / (w - 1) - 1, 2 * (p[:, 1] / Z) / (h - 1) - 1


def census(cam, rot, tr):
    """Counts over the case's pixels: behind the camera (p_z < 1e-3), overwritten by the zeros padding (a coordinate outside
    [-1, 1]; the behind-camera pixels are among them), inside; and the margins: the smallest |p_z - 1e-3|, the smallest
    distance of a normalised coordinate from +-1, and for behind-camera pixels the smallest distance in PIXELS by which
    the clamped point p_x / 1e-3, p_y / 1e-3 misses the image [0, W-1] x [0, H-1] along an axis."""
    b, _, h, w = cam.shape
    p, xn, yn = project(cam, rot, tr)
    behind = p[:, 2] < 1e-3
    out = (xn.abs() > 1) | (yn.abs() > 1)
    n = types.SimpleNamespace(behind=int(behind.sum()), overwritten=int(out.sum()), inside=int((~out).sum()),
                              pixels=behind.numel())
    n.pz_margin = float((p[:, 2] - 1e-3).abs().min())
    n.edge_margin = float(torch.minimum((xn.abs() - 1).abs().min(), (yn.abs() - 1).abs().min()))
    n.behind_miss = float("inf")
    if n.behind:
        for q, size in ((p[:, 0][behind] / 1e-3, w), (p[:, 1][behind] / 1e-3, h)):
            n.behind_miss = min(n.behind_miss, float(torch.maximum(-q, q - (size - 1)).min()))
    n.min_front_pz = float(p[:, 2][~behind].min()) if n.behind < n.pixels else float("inf")
    return n


def _leaf(x, grad):
    return None if x is None else x.detach().double().clone().requires_grad_(grad)


def oracle_cam2pixel(cam, rot, tr, pad, gg, need_cam=True, need_rt=True):
    """oracle.geometry.cam2pixel in fp64 on the fp32 operands (an absent operand is the identity / zero, without a
    gradient): (grid, g_cam, g_rot, g_tr), None where not requested or absent."""
    b = cam.shape[0]
    c, r, t = _leaf(cam, need_cam), _leaf(rot, need_rt), _leaf(tr, need_rt)
    eye = torch.eye(3, dtype=torch.float64).expand(b, 3, 3)
    grid = og.cam2pixel(c, r if r is not None else eye, t if t is not None else torch.zeros(b, 3, 1, dtype=torch.float64), pad)
    if need_cam or (need_rt and (r is not None or t is not None)):
        (grid * gg.double()).sum().backward()
    return grid.detach(), c.grad, None if r is None else r.grad, None if t is None else t.grad


# ------------------------------------------------------------------------------------------------ pose vectors
N_POSE = 130                                    # three blocks of pose_vec2mat_kernel's 64 threads, the last of 2


def pose_vectors(mode, seed=0):
    """[N_POSE, 6] fp32.  euler / quat: (t, r) with rotations of 0.2 rad / quaternion parts of 0.2, row 0 all zeros.  se3:
    (w, u); rows 0-3 have w = 0 exactly (theta = 0: the first-order branch and the reference's constant generators), rows
    4-7 |w| = 1 +- 0.1, rows 8-11 |w| = 1e-3 (small but on the closed-form side of theta^2 < 1e-12), the rest |w| up to 0.5."""
    gen = torch.Generator().manual_seed(77 + seed + {"euler": 0, "quat": 1, "se3": 2}[mode])
    vec = torch.randn(N_POSE, 6, generator=gen) * 0.2
    if mode != "se3":
        vec[0] = 0.0
        return vec
    w = torch.randn(N_POSE, 3, generator=gen)
    w = w / w.norm(dim=1, keepdim=True)
    theta = torch.rand(N_POSE, generator=gen) * 0.5
    theta[:4] = 0.0
    theta[4:8] = 0.9 + 0.2 * torch.rand(4, generator=gen)
    theta[8:12] = 1e-3
    vec[:, :3] = w * theta[:, None]
    vec[:, 3:] = torch.randn(N_POSE, 3, generator=gen)
    return vec


def oracle_pose(vec, mode, gm):
    """fp64 [N,3,4] and the gradient of sum(out * gm): pose_vec2mat for euler / quat, se3_exp (with the reference's own
    backward) for se3."""
    v = vec.detach().double().clone().requires_grad_(True)
    out = og.se3_exp(v) if mode == "se3" else og.pose_vec2mat(v, mode)
    (out * gm.double()).sum().backward()
    return out.detach(), v.grad
