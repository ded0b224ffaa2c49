"""Full-resolution multi-scale sampling on the GPU: the HIP kernel pair (csrc/upsample.hip) against the fp64 torch restatement
(tests/fullres_ref.py), the loss path of loss_functions_sfm fed through full_resolution, the training step and the command
line.  Every bound is conftest.rel_err (max-abs error / max-abs reference) at the suite's fp32 bound 1e-4 unless stated."""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import fullres_ref as FR
import minreproj_ref as MR
from conftest import PKG, ROOT, outliers, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
FACTORS = (2, 4, 8)


def _run_hip(x, gout, factor, recip_eps=None):
    """UpsampleIntFn forward + backward on the device: (out, gin) on the CPU."""
    from dvf.ops import UpsampleIntFn
    xg = x.to(DEV).requires_grad_(True)
    out = UpsampleIntFn.apply(xg, factor, recip_eps)
    out.backward(gout.to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), xg.grad.cpu()


def _run_ref(x, gout, factor, recip_eps=None, dt=torch.float64):
    xr = x.to(dt).requires_grad_(True)
    hw = (factor * x.shape[2], factor * x.shape[3])
    out = FR.upsample(xr, hw) if recip_eps is None else FR.upsample_depth(xr, hw, recip_eps)
    out.backward(gout.to(dt))
    return out.detach(), xr.grad


# coarse (h, w), planes as (B, C).  The backward's block owns a 32 x 128 core of fine pixels: (9, 33) spans 3 x 3 blocks at
# x8 with partial tiles on both axes; (19, 41) gives 38 x 82, 76 x 164 and 152 x 328 fine pixels -- never a multiple of the
# tile in either axis, two to five bands of rows per plane -- and its 5 planes are not a multiple of anything.
_EXACT_SHAPES = [((1, 1), (2, 3)), ((2, 3), (2, 3)), ((5, 7), (2, 3)), ((9, 33), (2, 3)), ((19, 41), (5, 1))]


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("hw,planes", _EXACT_SHAPES)
def test_plain_mode_is_bit_exact_with_integer_operands(hw, planes, factor):
    """Integer inputs in [-64, 64], integer output gradients in [-8, 8]: the weights are multiples of 1/(2 factor) per axis,
    so every product and partial sum is exact in fp32 and forward and backward must EQUAL the fp64 restatement, whatever the
    order of summation (tests/test_fullres.py shows the same for torch's own fp32 path).  Covers clamping at all four
    borders, single-row and single-pixel planes and the seams between blocks."""
    (h, w), (b, c) = hw, planes
    gen = torch.Generator().manual_seed(100 * h + w + factor)
    x = torch.randint(-64, 65, (b, c, h, w), generator=gen).float()
    gout = torch.randint(-8, 9, (b, c, factor * h, factor * w), generator=gen).float()
    out, gin = _run_hip(x, gout, factor)
    r_out, r_gin = _run_ref(x, gout, factor)
    assert float(r_gin.abs().max()) > 0
    assert torch.equal(out.double(), r_out)
    assert torch.equal(gin.double(), r_gin)


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("hw", [(5, 7), (9, 33)])
@pytest.mark.parametrize("eps", [0.0, 1e-4])
def test_reciprocal_mode_vs_fp64_restatement(hw, eps, factor):
    """Disparities in the network's range (10 * sigmoid + 0.01), random gout: the fused depth and the coarse gradient within
    1e-4 of fp64, and two runs bit-identical.  (The fp32 torch restatement is at ~7e-8 / ~8e-8 of fp64 on such inputs.)
    On an MI355X: forward at most 7.1e-8, gradient at most 2.4e-7 over the twelve cases."""
    h, w = hw
    gen = torch.Generator().manual_seed(10 * h + factor)
    x = 10 * torch.sigmoid(torch.randn(2, 3, h, w, generator=gen) * 2) + 0.01
    gout = torch.randn(2, 3, factor * h, factor * w, generator=gen)
    out, gin = _run_hip(x, gout, factor, eps)
    out2, gin2 = _run_hip(x, gout, factor, eps)
    r_out, r_gin = _run_ref(x, gout, factor, eps)
    e_out, e_gin = rel_err(out, r_out), rel_err(gin, r_gin)
    print(hw, eps, factor, "forward", e_out, "gradient", e_gin)
    assert e_out < TOL and e_gin < TOL
    assert torch.equal(out, out2) and torch.equal(gin, gin2)


def _kitti_K(b, h, w):
    K = torch.tensor([[0.58 * w, 0, 0.5 * w], [0, 1.92 * h, 0.5 * h], [0, 0, 1.0]]).expand(b, 3, 3).contiguous()
    return K, torch.inverse(K[0]).expand(b, 3, 3).contiguous()


SEED = 12               # of the composition images: see test_composition_vs_fp64_definition


@functools.lru_cache(maxsize=None)
def _case(b=2, h=64, w=208, v=2):
    """Four-scale inputs at 2x3x64x208, two views: images of twice box-filtered noise (test_gpu_minreproj._composition_case
    says why), DISPARITIES of depth 2..22 m at h >> s, explainability masks in [0.05, 0.95], small random poses, view 1 with
    the stereo baseline."""
    gen = torch.Generator().manual_seed(SEED + v)
    box = lambda t: F.avg_pool2d(F.pad(t, (2, 2, 2, 2), mode="reflect"), 5, 1)    # noqa: E731
    tgt = box(box(torch.rand(b, 3, h, w, generator=gen)))
    refs = [box(box(torch.rand(b, 3, h, w, generator=gen))) for _ in range(v)]
    pose = torch.randn(b, v, 6, generator=gen) * 0.03
    pose[:, 1, 0] -= 0.54
    K, Kinv = _kitti_K(b, h, w)
    disps = [1.0 / (torch.rand(b, 1, h >> s, w >> s, generator=gen) * 20 + 2) for s in range(4)]
    masks = [torch.rand(b, v, h >> s, w >> s, generator=gen) * 0.9 + 0.05 for s in range(4)]
    return tgt, refs, K, Kinv, disps, masks, pose


def test_loss_path_equals_torch_upsampling_in_front_of_the_same_loss_kernels():
    """photometric_reconstruction_loss fed with full_resolution(...) of four disparities and four masks against the same call
    fed with depths and masks that tests/fullres_ref.py upsampled in torch on the device: loss and the gradients with
    respect to the coarse disparities, the coarse masks and the pose within 1e-4 of each other, no outlier allowance.
    On an MI355X: loss 0, pose 1.5e-7, disparities at most 2.8e-6, masks at most 1.0e-5."""
    import loss_functions_sfm as LS
    tgt, refs, K, Kinv, disps, masks, pose = _case()
    hw = tgt.shape[2:]
    tgt, refs, K, Kinv = tgt.to(DEV), [r.to(DEV) for r in refs], K.to(DEV), Kinv.to(DEV)
    res = []
    for hip in (True, False):
        gd = [d.to(DEV).requires_grad_(True) for d in disps]
        gm = [m.to(DEV).requires_grad_(True) for m in masks]
        gp = pose.to(DEV).requires_grad_(True)
        if hip:
            depth, full_masks = LS.full_resolution(gd, hw, recip_eps=0.0), LS.full_resolution(gm, hw)
        else:
            depth, full_masks = [FR.upsample_depth(d, hw, 0.0) for d in gd], [FR.upsample(m, hw) for m in gm]
        assert all(tuple(d.shape[2:]) == tuple(hw) for d in depth + full_masks)
        loss = LS.photometric_reconstruction_loss(tgt, refs, K, Kinv, depth, full_masks, gp)
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach(), gp.grad, [d.grad for d in gd], [m.grad for m in gm]))
    (l_h, p_h, d_h, m_h), (l_t, p_t, d_t, m_t) = res
    errs = {"loss": rel_err(l_h, l_t), "pose": rel_err(p_h, p_t)}
    for s in range(4):
        errs[f"disp[{s}]"], errs[f"mask[{s}]"] = rel_err(d_h[s], d_t[s]), rel_err(m_h[s], m_t[s])
        assert float(d_t[s].abs().max()) > 0 and float(m_t[s].abs().max()) > 0
    print(errs)
    for n, e in errs.items():
        assert e < TOL, (n, e)


@functools.lru_cache(maxsize=None)
def _composition_ref(pad, dt):
    """tests/fullres_ref.upsample_depth in front of oracle.geometry.inverse_warp at FULL resolution + the minimum-reprojection
    restatement, one call per scale over all views.  Computed once per (padding, dtype); callers leave it unchanged."""
    from oracle import geometry as og
    tgt, refs, K, Kinv, disps, _, pose = _case()
    hw = tgt.shape[2:]
    tgt, refs, K, Kinv = tgt.to(dt), [r.to(dt) for r in refs], K.to(dt), Kinv.to(dt)
    disps = [d.detach().clone().to(dt).requires_grad_(True) for d in disps]
    pose = pose.detach().clone().to(dt).requires_grad_(True)
    total = 0
    for d in disps:
        depth = FR.upsample_depth(d, hw, 0.0)
        warped = [og.inverse_warp(r, depth[:, 0], pose[:, i], K, Kinv, "euler", pad, False) for i, r in enumerate(refs)]
        total = total + MR.minreproj_loss(tgt, warped, refs, alpha=0.85)[0]
    total.backward()
    return total.detach(), pose.grad, [d.grad for d in disps]


def _outlier_share(got, ref):
    """Share of the gradient elements, over all four scales, off by more than 1e-4 of their scale's maximum."""
    return sum(outliers(g, r, TOL) for g, r in zip(got, ref)) / sum(r.numel() for r in ref)


OUTLIER_CAP = 2e-4


@pytest.mark.parametrize("pad", ["zeros", "border"])
def test_composition_vs_fp64_definition(pad):
    """photometric_reconstruction_loss(ssim_weight=0.85, min_reprojection=True, auto_mask=True) over full_resolution(four
    disparities) at 2x3x64x208, V = 2, against the torch composition in fp32 and fp64.  Same criteria as
    test_gpu_minreproj.test_multiscale_composition_vs_reference: loss within 1e-4 of fp64; pose gradient within
    max(1e-4, 8 x the fp32 restatement's own distance to fp64); coarse-disparity gradients by the share of elements off by
    more than 1e-4 of their scale's maximum, at most 2e-4, the fp32 restatement itself asserted at or below half that cap.
    The seed keeps the fp32 restatement at or below half the cap (with 35 k elements the cap is seven of them): seeds 11 and
    13 gave it shares of 1.4e-4 / 8.5e-5 and 3.7e-4 / 2.5e-4.  Measured for padding = zeros, border, fp32 restatement against
    fp64: disparity share 0, 0 of 35 k elements, pose floor 4.9e-5, 5.0e-5 (on a second host 4.7e-5, 4.8e-5).  The kernels
    against fp64 on an MI355X: loss 6.1e-9, 2.3e-8; pose 5.7e-5, 5.1e-5; disparity share 8.5e-5 (three elements), 0."""
    import loss_functions_sfm as LS
    r32 = _composition_ref(pad, torch.float32)
    r64 = _composition_ref(pad, torch.float64)
    floor_d, floor_p = _outlier_share(r32[2], r64[2]), rel_err(r32[1], r64[1])
    print("fp32 restatement vs fp64: disparity share", floor_d, "pose", floor_p)
    assert floor_d <= OUTLIER_CAP / 2
    tgt, refs, K, Kinv, disps, _, pose = _case()
    gd = [d.to(DEV).requires_grad_(True) for d in disps]
    gp = pose.to(DEV).requires_grad_(True)
    counts = []
    loss = LS.photometric_reconstruction_loss(tgt.to(DEV), [r.to(DEV) for r in refs], K.to(DEV), Kinv.to(DEV),
                                              LS.full_resolution(gd, tgt.shape[2:], recip_eps=0.0), [None] * 4, gp, "euler", pad,
                                              ssim_weight=0.85, min_reprojection=True, auto_mask=True, selection_counts=counts)
    loss.backward()
    torch.cuda.synchronize()
    e_loss, e_pose = rel_err(loss, r64[0]), rel_err(gp.grad, r64[1])
    s_d = _outlier_share([d.grad for d in gd], r64[2])
    print("HIP vs fp64: loss", e_loss, "pose", e_pose, "disparity share", s_d)
    assert len(counts) == 4 and [int(c.sum()) for c in counts] == [tgt.shape[0] * tgt.shape[2] * tgt.shape[3]] * 4
    assert float(r64[0]) > 0 and float(r64[1].abs().max()) > 0 and all(float(g.abs().max()) > 0 for g in r64[2])
    assert e_loss < TOL
    assert e_pose < max(TOL, 8 * floor_p)
    assert s_d <= OUTLIER_CAP


# ------------------------------------------------------------------------------------------------ training step
def _fwd_bwd(disp, pose, opt, batch, **kw):
    from dvf import lib as L
    from dvf.steps import train_sfm_losses
    loss, terms = train_sfm_losses(disp, pose, batch, **kw)
    opt.zero_grad()
    loss.backward()
    opt.join_wgrad()
    L.join_aux_streams()
    torch.cuda.synchronize()
    return terms, opt.flat_g.clone()


def test_mode_off_changes_nothing():
    """train_sfm_losses(full_res_multiscale=False) leaves the terms and the gradient arena of a call without the keyword, bit
    for bit (deterministic mode, same weights)."""
    from dvf import conv as C
    from test_gpu_minreproj import _sfm_step_setup
    disp, pose, opt, batch = _sfm_step_setup()
    C.set_deterministic(True)
    try:
        t_plain, g_plain = _fwd_bwd(disp, pose, opt, batch, w2=0.2)
        t_off, g_off = _fwd_bwd(disp, pose, opt, batch, w2=0.2, full_res_multiscale=False)
    finally:
        C.set_deterministic(False)
    assert sorted(t_plain) == sorted(t_off)
    for k in t_plain:
        assert torch.equal(t_plain[k], t_off[k]), k
    assert torch.equal(g_plain, g_off) and float(g_plain.abs().max()) > 0


_MODES = {"masks": dict(w2=0.2), "appearance": dict(ssim_weight=0.85, min_reprojection=True, auto_mask=True)}


@pytest.mark.parametrize("mode", sorted(_MODES))
def test_mode_on_trains(mode):
    """DispNetS + PoseExpNet_sfm, batch 2 at 128x416 (disp4 is 16x52: every factor 1, 2, 4, 8 runs).  With the mode on -- alone
    with explainability masks and w2 = 0.2, and together with SSIM, minimum reprojection and auto-mask -- loss and gradients
    are finite, the photometric term differs from the native-scale one while the native-scale terms keep their bits, and two
    iterations under FlatAdam run eagerly and as HIP-graph replays with moving weights."""
    from dvf import conv as C
    from dvf.engine import GraphedStep
    from dvf.steps import train_sfm_losses
    from test_gpu_minreproj import _sfm_step_setup
    disp, pose, opt, batch = _sfm_step_setup()
    kw = _MODES[mode]
    C.set_deterministic(True)
    try:
        t_native, g_native = _fwd_bwd(disp, pose, opt, batch, **kw)
        t_on, g_on = _fwd_bwd(disp, pose, opt, batch, full_res_multiscale=True, **kw)
        assert all(bool(torch.isfinite(v)) for v in t_on.values()) and bool(torch.isfinite(g_on).all())
        assert float(t_on["photo"]) != float(t_native["photo"]) and not torch.equal(g_on, g_native)
        assert torch.equal(t_on["smooth"], t_native["smooth"]) and torch.equal(t_on["lr"], t_native["lr"])   # native-scale terms
        if mode == "masks":
            assert torch.equal(t_on["exp"], t_native["exp"])
        else:
            assert 0 <= float(t_on["automask"]) <= 1

        def step():
            loss, terms = train_sfm_losses(disp, pose, batch, full_res_multiscale=True, **kw)
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
    print(mode, "native photo", float(t_native["photo"]), "full-res photo", float(t_on["photo"]), "eager", eager, "replayed",
          replayed)
    for total, photo in eager + replayed:
        assert total == total and abs(total) < 1e6 and photo > 0
    assert eager[0] != eager[1] and replayed[0] != replayed[1]        # the weights moved


@pytest.mark.parametrize("mode", sorted(_MODES))
def test_mode_on_is_bit_reproducible_in_deterministic_mode(mode):
    """Two deterministic forward + backward passes from the same state, mode on: every term and the whole gradient arena are
    bit-identical.  The depth network's share of the arena -- everything that flows through the new kernels -- is asserted
    first, then the whole arena.
    The appearance options go through dvf.ops.InverseWarpFn, whose backward adds the pose gradient's per-block partials
    with float atomics by default: at full resolution every scale has 4 to 64 times as many blocks and the order of
    arrival showed (about 0.6 M pose-network gradient elements differed between two runs, by up to 1.9e-7 of the largest
    gradient, the depth network's none).  In deterministic mode it now takes dvf_inverse_warp_bwd_ordered, which stores the
    partials and adds them in block order, as the fused L1 kernel of the masks case always did."""
    from dvf import conv as C
    from test_gpu_minreproj import _sfm_step_setup
    disp, pose, opt, batch = _sfm_step_setup()
    kw = _MODES[mode]
    in_disp = torch.zeros(opt.flat_g.numel(), dtype=torch.bool, device=DEV)       # the depth network's share of the arena
    for p in disp.parameters():
        o = (p._dvf_grad.data_ptr() - opt.flat_g.data_ptr()) // 4
        in_disp[o:o + p.numel()] = True
    C.set_deterministic(True)
    try:
        _fwd_bwd(disp, pose, opt, batch, full_res_multiscale=True, **kw)                      # sizes every workspace
        t_a, g_a = _fwd_bwd(disp, pose, opt, batch, full_res_multiscale=True, **kw)
        t_b, g_b = _fwd_bwd(disp, pose, opt, batch, full_res_multiscale=True, **kw)
    finally:
        C.set_deterministic(False)
    differ = int((g_a != g_b).sum())
    print(mode, "arena elements", g_a.numel(), "depth network", int(in_disp.sum()), "differing", differ,
          "of them in the depth network", int(((g_a != g_b) & in_disp).sum()), "largest difference / largest gradient",
          float((g_a - g_b).abs().max() / g_a.abs().max()))
    assert float(g_a.abs().max()) > 0
    for k in t_a:
        assert torch.equal(t_a[k], t_b[k]), k
    assert torch.equal(g_a[in_disp], g_b[in_disp])
    assert torch.equal(g_a, g_b)


def test_inverse_warp_pose_gradient_is_ordered_in_deterministic_mode():
    """InverseWarpFn at 2x3x128x416 (13 x 32 blocks per image): in deterministic mode two backward passes give bit-identical
    gradients, and they agree with the default (atomic) path within 1e-4 -- the two differ only in the order of one sum."""
    from dvf import conv as C
    from dvf import lib as L
    from dvf.ops import InverseWarpFn
    gen = torch.Generator().manual_seed(5)
    b, h, w = 2, 128, 416
    box = lambda t: F.avg_pool2d(F.pad(t, (2, 2, 2, 2), mode="reflect"), 5, 1)    # noqa: E731
    img = box(torch.rand(b, 3, h, w, generator=gen)).to(DEV)
    depth = (torch.rand(b, h, w, generator=gen) * 20 + 2).to(DEV)
    pose = torch.randn(b, 6, generator=gen) * 0.03
    pose[:, 0] -= 0.54
    K, Kinv = (t.to(DEV) for t in _kitti_K(b, h, w))
    gout = torch.randn(b, 3, h, w, generator=gen).to(DEV)

    def run():
        d, p = depth.clone().requires_grad_(True), pose.to(DEV).requires_grad_(True)
        InverseWarpFn.apply(img, d, p, K, Kinv, L.geom_flags()).backward(gout)
        torch.cuda.synchronize()
        return d.grad, p.grad

    default = run()
    C.set_deterministic(True)
    try:
        first, second = run(), run()
    finally:
        C.set_deterministic(False)
    assert float(default[1].abs().max()) > 0
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert torch.equal(first[0], default[0])                       # the depth gradient is per pixel either way
    print("ordered vs atomic pose gradient", rel_err(first[1], default[1]))
    assert rel_err(first[1], default[1]) < TOL


# ------------------------------------------------------------------------------------------------ command line
def test_train_cli_with_the_whole_recipe(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "-b", "2", "--height", "128", "--width", "416", "--epochs", "1",
           "--steps-per-epoch", "2", "--full-res-multiscale", "--ssim-weight", "0.85", "--min-reprojection", "--auto-mask",
           "--output-dir", str(tmp_path / "ckpt")]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("Train epoch")]
    assert len(lines) == 1
    for name in ("total", "photo", "smooth", "lr", "automask"):
        v = float(lines[0].split(name + ":")[1].split()[0])
        assert v == v and abs(v) < 1e6, (name, v)
    assert float(lines[0].split("photo:")[1].split()[0]) > 0


def test_single_scale_entry_point_refuses_the_flag():
    res = subprocess.run([sys.executable, os.path.join(PKG, "unsupervise.py"), "--full-res-multiscale"], capture_output=True,
                         text=True, timeout=600, env=dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT))
    assert res.returncode != 0
    assert "--full-res-multiscale needs a multi-scale loss" in res.stderr, res.stderr[-2000:]
