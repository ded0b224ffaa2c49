"""The stand-alone geometry helpers of inverse_warp.py (PoseVec2MatFn, Pixel2CamFn, Cam2PixelFn of dvf/ops.py; kernels in
csrc/warp_loss.hip) against the fp64 oracle on the fp32 operands of tests/geometry_cases.py, at the shapes and branches
test_gpu_losses.py::test_geometry_helpers_vs_oracle (2x24x40, everything in front of the camera, every operand present and
every gradient requested) leaves out: the smallest legal image, an image that cam2pixel_bwd_kernel splits into two chunks
with a short last one, points behind the camera (Z = max(p_z, 1e-3) and its gradient cut, zpass), rot == NULL, tr == NULL,
g_cam == NULL and ws == NULL, and the se(3) mode of pose_vec2mat at theta = 0, 1e-3 and 1.

Bounds, as that test: forward values 1e-6 and the pose_vec2mat / pixel2cam gradients 1e-5; the cam2pixel gradients
test_gpu_losses.TOL = 1e-4 (conftest.rel_err, relative to the tensor's maximum).  With border padding a point behind the
camera sits at p_x / 1e-3, a thousand times further out than any other, and sets that maximum, so the points in front of
the camera are compared once more among themselves, with the same bounds.  With zeros padding the overwritten coordinates
are the oracle's, element for element, and so are the exact zeros of the gradient.
Measured worst deviations over every case of this file: pose_vec2mat forward 2.3e-7 (quat), gradient 1.7e-7 (euler, quat) and
4.1e-6 (se3, bound 1e-5); pixel2cam 9.6e-8 and 7.9e-8; cam2pixel forward 5.1e-7 (2x91x91 behind the camera, zeros), g_cam
7.7e-7 (in front, border), g_rot 5.6e-7, g_tr 1.0e-6."""
import pytest
import torch

import geometry_cases as G
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD, GRAD, TOL = 1e-6, 1e-5, 1e-4
IDS = ["%dx%dx%d" % s for s in G.SHAPES]


def _dev(x, grad=False):
    return None if x is None else x.detach().clone().to(DEV).requires_grad_(grad)


@pytest.fixture(scope="module")
def cases():
    return {(s, f): G.make(s, f) for s in G.SHAPES for f in G.FAMILIES}


@pytest.mark.parametrize("mode", ["euler", "quat", "se3"])
def test_pose_vec2mat_modes(mode):
    """130 poses (three blocks of 64 threads, the last of 2).  se3: rows with theta = 0 exactly (first-order branch and the
    reference's constant generators in the backward), theta = 1e-3 and theta ~ 1, against oracle.geometry.se3_exp."""
    import inverse_warp as iw
    from dvf import lib as L
    from dvf.ops import PoseVec2MatFn
    vec = G.pose_vectors(mode)
    gm = torch.randn(G.N_POSE, 3, 4, generator=torch.Generator().manual_seed(3))
    ref, ref_grad = G.oracle_pose(vec, mode, gm)
    gv = _dev(vec, True)
    out = PoseVec2MatFn.apply(gv, L.POSE_SE3) if mode == "se3" else iw.pose_vec2mat(gv, mode)
    (out * gm.to(DEV)).sum().backward()
    e_out, e_grad = rel_err(out, ref), rel_err(gv.grad, ref_grad)
    rows = slice(0, 4) if mode == "se3" else slice(0, 1)
    e0_out, e0_grad = rel_err(out[rows], ref[rows]), rel_err(gv.grad[rows], ref_grad[rows])
    print(f"pose_vec2mat {mode}: forward {e_out:.3g}, gradient {e_grad:.3g}; zero-rotation rows {e0_out:.3g}, {e0_grad:.3g}")
    assert tuple(out.shape) == (G.N_POSE, 3, 4)
    assert e_out < FWD and e_grad < GRAD
    assert e0_out < FWD and e0_grad < GRAD


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_pixel2cam(cases, shape, family):
    import inverse_warp as iw
    case = cases[(shape, family)]
    rd = case.depth.double().requires_grad_(True)
    ref = G.og.pixel2cam(rd, case.Kinv.double())
    (ref * case.gc.double()).sum().backward()
    gd = _dev(case.depth, True)
    cam = iw.pixel2cam(gd, case.Kinv.to(DEV))
    (cam * case.gc.to(DEV)).sum().backward()
    e_out, e_grad = rel_err(cam, ref), rel_err(gd.grad, rd.grad)
    print(f"pixel2cam {shape} {family}: forward {e_out:.3g}, gradient {e_grad:.3g}")
    assert tuple(cam.shape) == (shape[0], 3) + shape[1:]
    assert e_out < FWD and e_grad < GRAD


def _cam2pixel(case, combo, pad, need_cam, need_rt):
    """Run Cam2PixelFn and the oracle on one operand combination and compare; returns the worst ratio error / bound."""
    import inverse_warp as iw
    cam, rot, tr = G.operands(case, combo)
    ref, r_cam, r_rot, r_tr = G.oracle_cam2pixel(cam, rot, tr, pad, case.gg, need_cam, need_rt)
    front = G.project(cam, rot, tr)[0][:, 2] >= 1e-3                       # [B,H,W]
    dc, dr, dt = _dev(cam, need_cam), _dev(rot, need_rt), _dev(tr, need_rt)
    grid = iw.cam2pixel(dc, dr, dt, pad)
    if grid.requires_grad:
        (grid * case.gg.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grid = grid.detach().cpu()
    tag = (case.shape, case.family, combo, pad, need_cam, need_rt)
    assert tuple(grid.shape) == tuple(ref.shape)
    if pad == "zeros":
        assert torch.equal(grid == 2, ref == 2), (tag, "overwritten coordinates differ")
    errs = {"grid": (rel_err(grid, ref), FWD), "grid, in front": (rel_err(grid[front], ref[front]), FWD)}
    if need_cam:
        g = dc.grad.cpu()
        errs["g_cam"] = (rel_err(g, r_cam), TOL)
        errs["g_cam, in front"] = (rel_err(g.permute(0, 2, 3, 1)[front], r_cam.permute(0, 2, 3, 1)[front]), TOL)
        assert bool((g[r_cam == 0] == 0).all()), (tag, "gradient where the oracle cuts it")
    else:
        assert dc.grad is None
    for name, d, r in (("g_rot", dr, r_rot), ("g_tr", dt, r_tr)):
        if d is None:
            continue
        if need_rt:
            assert d.grad is not None and d.grad.shape == d.shape, (tag, name)
            errs[name] = (rel_err(d.grad, r), TOL)
        else:
            assert d.grad is None
    print(tag, " ".join(f"{k} {e:.3g}" for k, (e, _) in errs.items()))
    for k, (e, bound) in errs.items():
        assert e < bound, (tag, k, e)
    return max(e / bound for e, bound in errs.values())


@pytest.mark.parametrize("pad", ["zeros", "border"])
@pytest.mark.parametrize("combo", G.COMBOS)
@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_cam2pixel_operand_combinations(cases, shape, family, combo, pad):
    """Every gradient that exists is requested.  no_rot / no_tr / neither: rot == NULL, tr == NULL in both kernels (the
    backward then runs with the identity / without the translation; g_rot / g_tr of an absent operand do not exist)."""
    _cam2pixel(cases[(shape, family)], combo, pad, True, True)


@pytest.mark.parametrize("pad", ["zeros", "border"])
@pytest.mark.parametrize("request_", ["cam", "rot_tr"])
@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_cam2pixel_gradient_requests(cases, shape, family, request_, pad):
    """cam alone: ws == NULL, the block leaves before its reduction.  rot / tr alone: g_cam == NULL."""
    _cam2pixel(cases[(shape, family)], "rot+tr", pad, request_ == "cam", request_ == "rot_tr")


@pytest.mark.parametrize("pad", ["zeros", "border"])
def test_cam2pixel_points_alone(cases, pad):
    """Neither operand and the points as the only leaf (rot = tr = None, ws == NULL) at the two-chunk shape."""
    _cam2pixel(cases[((2, 91, 91), "behind")], "neither", pad, True, False)
