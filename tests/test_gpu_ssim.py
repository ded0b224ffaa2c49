"""SSIM + L1 appearance term on the GPU: the HIP kernel pair (csrc/ssim_loss.hip) against the fp64 torch restatement
(tests/ssim_ref.py), its exact properties, the multi-scale composition in loss_functions_sfm and the training step.
Every bound is conftest.rel_err (max-abs error / max-abs reference) at the suite's fp32 bound 1e-4 unless stated."""
import pytest
import torch
import torch.nn.functional as F

import ssim_ref
from conftest import outliers, rel_err, safe_pixel_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
KINK_BAND = 5e-4        # conftest.safe_pixel_mask's band around the |x - y| kink, relative to max|x|


def _images(b, c, h, w, in_scale, seed):
    """Uniform random target / warped pair as the kernels read them (in_scale * value in [0, 1]); ~10 % of the warped pixels
    are exactly zero in all channels."""
    gen = torch.Generator().manual_seed(seed)
    amp = 1.0 / in_scale
    x = torch.rand(b, c, h, w, generator=gen) * amp
    y = torch.rand(b, c, h, w, generator=gen) * amp
    y = y * (torch.rand(b, 1, h, w, generator=gen) >= 0.1)
    y[0, :, h // 2, w // 2] = 0                                      # (tiny shapes: make sure one pixel is invalid)
    return x, y, gen


def _kink(x, y):
    """[B,1,H,W] bool: some channel has |x - y| inside the band where the sign of the L1 gradient is not determined."""
    return ((x - y).abs() < KINK_BAND * float(x.abs().max())).any(1, keepdim=True)


def _run_pair(x, y, mask, view, in_scale, alpha, c1=1e-4, c2=9e-4):
    """HIP forward + backward: (loss, g_tgt, g_warped, g_mask or None), on the CPU."""
    from dvf.ops import SsimL1LossFn
    xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    mg = mask.to(DEV).requires_grad_(True) if mask is not None else None
    loss = SsimL1LossFn.apply(xg, yg, mg, (in_scale, alpha, c1, c2, view))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), xg.grad.cpu(), yg.grad.cpu(), mg.grad.cpu() if mg is not None else None


def _run_ref(x, y, mask, view, in_scale, alpha, dt=torch.float64, c1=1e-4, c2=9e-4):
    xr, yr = x.clone().to(dt).requires_grad_(True), y.clone().to(dt).requires_grad_(True)
    mr = mask.clone().to(dt).requires_grad_(True) if mask is not None else None
    m_view = None if mr is None else (mr if view is None else mr[:, view:view + 1])
    loss = ssim_ref.ssim_l1_loss(xr, yr, m_view, alpha, c1, c2, in_scale)
    loss.backward()
    return loss.detach(), xr.grad, yr.grad, mr.grad if mr is not None else None


_ALL = [(m, s, a) for m in (True, False) for s in (1.0, 0.004) for a in (0.0, 0.85, 1.0)]
_CASES = [(shape, None) + cfg for shape in ((1, 1, 3, 3), (2, 3, 5, 9), (2, 3, 37, 75)) for cfg in _ALL] + [
    ((4, 3, 256, 832), None, True, 1.0, 0.85),          # bench size of the image term
    ((4, 3, 256, 832), None, False, 0.004, 0.85),
    ((4, 3, 256, 832), None, True, 0.004, 1.0),
    ((4, 3, 256, 832), None, False, 1.0, 0.0),
    ((2, 32, 128, 416), None, True, 1.0, 0.85),         # feature-map width
    ((2, 32, 128, 416), None, False, 0.004, 0.85),
    ((4, 3, 32, 104), 2, True, 1.0, 0.85),              # cfg 4 / 5 pyramid scales, [B,4,H,W] mask addressed by view
    ((4, 3, 32, 104), 0, True, 0.004, 0.85),
    ((8, 3, 48, 160), 3, True, 1.0, 0.85),
    ((8, 3, 48, 160), 1, True, 0.004, 0.0),
]


@pytest.mark.parametrize("shape,view,with_mask,in_scale,alpha", _CASES)
def test_kernel_pair_vs_fp64_restatement(shape, view, with_mask, in_scale, alpha):
    """Loss, g_warped, g_tgt and g_mask within 1e-4 of the fp64 restatement.  |x - y| is a kink: with a mask, the mask is
    zeroed where any channel lies inside the band (in both implementations); without one, the target is moved out of the
    band at those elements (in both)."""
    b, c, h, w = shape
    x, y, gen = _images(b, c, h, w, in_scale, seed=b * 1000 + c * 100 + h + int(alpha * 7))
    mask = None
    if with_mask:
        mask = torch.rand(b, 4 if view is not None else 1, h, w, generator=gen) * 0.9 + 0.05
        band = _kink(x, y).to(mask.dtype)
        if view is None:
            mask = mask * (1 - band)
        else:
            mask[:, view:view + 1] *= (1 - band)
    else:
        band = KINK_BAND * float(x.abs().max())
        x = torch.where((x - y).abs() < 2 * band, x + 6 * band, x)    # (2x: moving x may raise max|x|, and with it the band)
        assert not bool(_kink(x, y).any())
    d = ssim_ref.dssim(in_scale * x.double(), in_scale * y.double())
    assert 0 < float(d.min()) and float(d.max()) < 1              # the clamp is not active on these inputs
    got = _run_pair(x, y, mask, view, in_scale, alpha)
    ref = _run_ref(x, y, mask, view, in_scale, alpha)
    errs = {n: rel_err(g, r) for n, g, r in zip(("loss", "g_tgt", "g_warped", "g_mask"), got, ref) if r is not None}
    print(shape, view, with_mask, in_scale, alpha, errs)
    assert float(ref[0]) > 0
    for n, e in errs.items():
        assert e < TOL, (n, e)
    if view is not None:                                          # the other views of the mask get exactly nothing
        others = [v for v in range(4) if v != view]
        assert float(got[3][:, others].abs().max()) == 0


def test_all_zero_mask_gives_exact_zeros():
    x, y, _ = _images(2, 3, 37, 75, 1.0, seed=5)
    loss, gx, gy, gm = _run_pair(x, y, torch.zeros(2, 1, 37, 75), None, 1.0, 0.85)
    assert float(loss) == 0 and float(gx.abs().max()) == 0 and float(gy.abs().max()) == 0
    assert float(gm.abs().max()) > 0                              # the mask itself still has a gradient


def test_invalid_pixels_get_no_l1_gradient():
    """alpha = 0 leaves only the L1 part: exactly zero gradient where the warped pixel is zero in every channel, exactly
    +-in_scale / N elsewhere."""
    x, y, _ = _images(2, 3, 37, 75, 1.0, seed=6)
    _, gx, gy, _ = _run_pair(x, y, None, None, 1.0, 0.0)
    invalid = (y == 0).all(1, keepdim=True).expand_as(y)
    assert int(invalid.sum()) > 0
    assert float(gx[invalid].abs().max()) == 0 and float(gy[invalid].abs().max()) == 0
    n = x.numel()
    assert torch.equal(gy[~invalid], torch.sign(y - x)[~invalid] * torch.tensor(1.0 / n, dtype=torch.float32))
    assert torch.equal(gx[~invalid], -gy[~invalid])


def test_two_runs_are_bit_identical():
    x, y, gen = _images(4, 3, 256, 832, 1.0, seed=7)
    mask = torch.rand(4, 1, 256, 832, generator=gen)
    a = _run_pair(x, y, mask, None, 1.0, 0.85)
    b = _run_pair(x, y, mask, None, 1.0, 0.85)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_accumulate_adds_to_loss_out():
    from dvf import lib as L
    x, y, _ = _images(2, 3, 37, 75, 1.0, seed=8)
    xg, yg = x.to(DEV), y.to(DEV)
    lib = L.lib()
    out = torch.full((1,), 2.5, device=DEV)
    partials = torch.empty(int(lib.dvf_ssim_partials_floats(2, 37, 75)), device=DEV)
    fresh = torch.empty(1, device=DEV)
    for dst, acc in ((fresh, 0), (out, 1)):
        L.check(lib.dvf_ssim_loss_fwd(L.dev(xg), L.dev(yg), None, 0, L.dev(dst), L.dev(partials), 2, 3, 37, 75, 1.0, 0.85, 1e-4,
                                      9e-4, acc, L.stream()), "dvf_ssim_loss_fwd")
    torch.cuda.synchronize()
    assert float(fresh) > 0
    assert float(out) == float(torch.tensor(2.5) + fresh.cpu()[0])


# ------------------------------------------------------------------------------------------------ composition
def _kitti_K(b, h, w):
    K = torch.tensor([[0.58 * w, 0, 0.5 * w], [0, 1.92 * h, 0.5 * h], [0, 0, 1.0]]).expand(b, 3, 3).contiguous()
    return K, torch.inverse(K[0]).expand(b, 3, 3).contiguous()


def _composition_case(v, seed=11, b=2, h=128, w=416):
    """Four-scale inputs of loss_functions_sfm.photometric_reconstruction_loss: box-filtered noise images (as
    test_gpu_losses.test_photometric_vs_oracle), depth 2..22 m, small random poses, view 1 with the stereo baseline."""
    from oracle import geometry as og                                                # noqa: F401  (used by safe_pixel_mask)
    gen = torch.Generator().manual_seed(seed + v)
    smooth = lambda t: F.avg_pool2d(F.pad(t, (2, 2, 2, 2), mode="reflect"), 5, 1)    # noqa: E731
    tgt = torch.rand(b, 3, h, w, generator=gen)
    refs = [smooth(torch.rand(b, 3, h, w, generator=gen)) for _ in range(v)]
    pose = torch.randn(b, v, 6, generator=gen) * 0.03
    pose[:, 1, 0] -= 0.54
    K, Kinv = _kitti_K(b, h, w)
    depths, masks = [], []
    for s in range(4):
        hs, ws = h >> s, w >> s
        d = torch.rand(b, 1, hs, ws, generator=gen) * 20 + 2
        k_s = torch.cat((K[:, 0:2] / 2 ** s, K[:, 2:]), dim=1)
        kinv_s = torch.cat((Kinv[:, :, 0:2] * 2 ** s, Kinv[:, :, 2:]), dim=2)
        tgt_s = F.interpolate(tgt, (hs, ws), mode="area")
        refs_s = [F.interpolate(r, (hs, ws), mode="area") for r in refs]
        safe = safe_pixel_mask(d[:, 0], [pose[:, i] for i in range(v)], k_s, kinv_s, tgt=tgt_s, srcs=refs_s)
        depths.append(d)
        masks.append((torch.rand(b, v, hs, ws, generator=gen) * 0.9 + 0.05) * safe)
    return tgt, refs, K, Kinv, depths, masks, pose


def _composition_ref(case, pad, dt):
    """oracle.geometry.inverse_warp + F.interpolate(mode='area') + the restatement, per scale and view."""
    from oracle import geometry as og
    tgt, refs, K, Kinv, depths, masks, pose = case
    tgt, refs, K, Kinv = tgt.to(dt), [r.to(dt) for r in refs], K.to(dt), Kinv.to(dt)
    depths = [d.detach().clone().to(dt).requires_grad_(True) for d in depths]
    masks = [m.detach().clone().to(dt).requires_grad_(True) for m in masks]
    pose = pose.detach().clone().to(dt).requires_grad_(True)
    total = 0
    for d, m in zip(depths, masks):
        hs, ws = d.shape[2:]
        down = tgt.shape[2] / hs
        tgt_s = F.interpolate(tgt, (hs, ws), mode="area")
        k_s = torch.cat((K[:, 0:2] / down, K[:, 2:]), dim=1)
        kinv_s = torch.cat((Kinv[:, :, 0:2] * down, Kinv[:, :, 2:]), dim=2)
        for i, r in enumerate(refs):
            warped = og.inverse_warp(F.interpolate(r, (hs, ws), mode="area"), d[:, 0], pose[:, i], k_s, kinv_s, "euler", pad,
                                     False)
            total = total + ssim_ref.ssim_l1_loss(tgt_s, warped, m[:, i:i + 1], alpha=0.85)
    total.backward()
    return total.detach(), pose.grad, [d.grad for d in depths], [m.grad for m in masks]


def _outlier_share(got, ref):
    """Share of the per-pixel gradient elements, over all four scales, off by more than 1e-4 of their scale's maximum."""
    return sum(outliers(g, r, TOL) for g, r in zip(got, ref)) / sum(r.numel() for r in ref)


OUTLIER_CAP = 2e-4


@pytest.mark.parametrize("v,pad", [(2, "zeros"), (2, "border"), (4, "zeros"), (4, "border")])
def test_multiscale_composition_vs_reference(v, pad):
    """loss_functions_sfm.photometric_reconstruction_loss(ssim_weight=0.85) over 4 scales against the torch composition in
    fp32 and fp64; conftest.safe_pixel_mask (times random weights) is the explainability mask.  Loss within 1e-4 of fp64;
    pose gradient within max(1e-4, 8 x the fp32 reference's own distance to fp64); per-pixel gradients (depth, mask) by the
    share of elements off by more than 1e-4 of the maximum, at most 2e-4: a window carries its neighbours' sampler
    gradients, so masking a risky centre pixel does not remove it from the eight windows around it.
    The seed and geometry keep the fp32 reference itself at or below half the cap.  Its measured share against fp64 on
    the CPU, for (V, padding) = (2, zeros), (2, border), (4, zeros), (4, border): depth 1.4e-5, 1.4e-5, 2.8e-5, 5.7e-5 of
    141 k elements; mask 0, 0, 1.1e-5, 0 of 283 k / 566 k; pose floors 4.1e-4, 3.7e-4, 1.9e-3, 3.6e-3."""
    import loss_functions_sfm as LS
    case = _composition_case(v)
    r32 = _composition_ref(case, pad, torch.float32)
    r64 = _composition_ref(case, pad, torch.float64)
    floor_d, floor_m = _outlier_share(r32[2], r64[2]), _outlier_share(r32[3], r64[3])
    print("fp32 reference vs fp64: depth share", floor_d, "mask share", floor_m, "pose", rel_err(r32[1], r64[1]))
    assert floor_d <= OUTLIER_CAP / 2 and floor_m <= OUTLIER_CAP / 2
    tgt, refs, K, Kinv, depths, masks, pose = case
    gd = [d.to(DEV).requires_grad_(True) for d in depths]
    gm = [m.to(DEV).requires_grad_(True) for m in masks]
    gp = pose.to(DEV).requires_grad_(True)
    loss = LS.photometric_reconstruction_loss(tgt.to(DEV), [r.to(DEV) for r in refs], K.to(DEV), Kinv.to(DEV), gd, gm, gp,
                                              "euler", pad, ssim_weight=0.85)
    loss.backward()
    torch.cuda.synchronize()
    e_loss, e_pose = rel_err(loss, r64[0]), rel_err(gp.grad, r64[1])
    s_d = _outlier_share([d.grad for d in gd], r64[2])
    s_m = _outlier_share([m.grad for m in gm], r64[3])
    print("HIP vs fp64: loss", e_loss, "pose", e_pose, "depth share", s_d, "mask share", s_m)
    assert e_loss < TOL
    assert e_pose < max(TOL, 8 * rel_err(r32[1], r64[1]))
    assert s_d <= OUTLIER_CAP and s_m <= OUTLIER_CAP


# ------------------------------------------------------------------------------------------------ training step
def _sfm_step_setup():
    import DispNetS
    import PoseExpNet_sfm
    from dvf.engine import FlatAdam
    from dvf.synthetic import synthetic_batch
    torch.manual_seed(0)
    disp, pose = DispNetS.DispNetS(), PoseExpNet_sfm.PoseExpNet(nb_ref_imgs=2, output_exp=True)
    disp.init_weights()
    pose.init_weights()
    disp.to(DEV).train()
    pose.to(DEV).train()
    opt = FlatAdam(list(disp.parameters()) + list(pose.parameters()), lr=2e-4, overlap=False)
    return disp, pose, opt, synthetic_batch(2, 128, 416, seed=1234, device=DEV, n_views=2)


def test_ssim_weight_zero_changes_nothing_and_ssim_step_trains():
    """train_sfm_losses(ssim_weight=0.0) leaves the loss and the gradient arena of a call without the keyword, bit for bit
    (deterministic mode, same weights).  With 0.85 the step is finite, its photometric term differs, and two iterations
    under FlatAdam run eagerly and as HIP-graph replays."""
    from dvf import conv as C
    from dvf import lib as L
    from dvf.engine import GraphedStep
    from dvf.steps import train_sfm_losses
    disp, pose, opt, batch = _sfm_step_setup()

    def fwd_bwd(**kw):
        loss, terms = train_sfm_losses(disp, pose, batch, w2=0.2, **kw)
        opt.zero_grad()
        loss.backward()
        opt.join_wgrad()
        L.join_aux_streams()
        torch.cuda.synchronize()
        return terms, opt.flat_g.clone()

    C.set_deterministic(True)
    try:
        t_plain, g_plain = fwd_bwd()
        t_zero, g_zero = fwd_bwd(ssim_weight=0.0)
        assert torch.equal(t_plain["total"], t_zero["total"]) and torch.equal(t_plain["photo"], t_zero["photo"])
        assert torch.equal(g_plain, g_zero)
        t_ssim, g_ssim = fwd_bwd(ssim_weight=0.85)
        assert bool(torch.isfinite(t_ssim["total"])) and bool(torch.isfinite(g_ssim).all())
        assert float(t_ssim["photo"]) != float(t_plain["photo"]) and float(g_ssim.abs().max()) > 0

        def step():
            loss, terms = train_sfm_losses(disp, pose, batch, w2=0.2, ssim_weight=0.85)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return (terms["total"], terms["photo"])

        eager = [tuple(float(t) for t in step()) for _ in range(2)]
        graphed = GraphedStep(step, [], warmup=1)
        replayed = []
        for _ in range(2):
            out = graphed()
            torch.cuda.synchronize()
            replayed.append(tuple(float(t) for t in out))
    finally:
        C.set_deterministic(False)
    print("eager", eager, "replayed", replayed)
    for total, photo in eager + replayed:
        assert total == total and abs(total) < 1e6 and photo > 0
    assert eager[0] != eager[1] and replayed[0] != replayed[1]        # the weights moved
