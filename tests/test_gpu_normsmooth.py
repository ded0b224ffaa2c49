"""Edge-aware smoothness of the mean-normalised disparity on the GPU: the HIP kernel pair (csrc/norm_smooth.hip) against the
fp64 torch restatement (tests/normsmooth_ref.py, the definition of the term), the multi-scale loss of loss_functions_sfm, the
training steps, graph capture and the command line.  Every bound is conftest.rel_err (max-abs error / max-abs reference) at
the suite's fp32 bound 1e-4: both sides read the same fp32 operands, so sign(delta) cannot differ and there is no outlier
allowance."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import normsmooth_ref as NR
from conftest import PKG, ROOT, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
IMAGE_SCALES = (1.0, 3.0, 0.2)      # per-image factor of the disparities: the means differ by up to 15x

# (B, C, H, W): the minimum size, a 64x16 tile edge exactly on and one past the last column (64, 65) and, with 4 rows per
# thread, the last row (4, 5, 16), several tiles in both axes (9x130 is 1x3, and 130 = 2 * 64 + 2), C = 1, B with distinct means
SHAPES = [(1, 1, 2, 2), (2, 3, 2, 3), (3, 3, 5, 7), (2, 3, 4, 64), (2, 3, 5, 65), (3, 1, 9, 130), (2, 3, 16, 52)]


def _disparity(b, h, w, gen):
    d = 10 * torch.sigmoid(2 * torch.randn(b, 1, h, w, generator=gen)) + 0.01
    return d * torch.tensor(IMAGE_SCALES[:b]).view(b, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def _inputs(shape, in_scale):
    """fp32 disparity and image of one case; the image is in [-1, 1] for in_scale 1 and in 0..255 otherwise."""
    b, c, h, w = shape
    gen = torch.Generator().manual_seed(1000 * h + w + c)
    disp = _disparity(b, h, w, gen)
    img = torch.rand(b, c, h, w, generator=gen)
    return disp, (img * 2 - 1 if in_scale == 1.0 else img * 255)


@functools.lru_cache(maxsize=None)
def _reference(shape, in_scale, eps):
    """fp64 loss and disparity gradient of the restatement on the fp32 values of _inputs.  Computed once per case."""
    disp, img = _inputs(shape, in_scale)
    d = disp.double().requires_grad_(True)
    loss = NR.normalized_smooth_loss(d, img.double(), in_scale, eps)
    loss.backward()
    return loss.detach(), d.grad


def _run_abi(disp, img, in_scale, eps, weight=1.0, grad_loss=1.0, preset=None):
    """dvf_norm_smooth_fwd + _bwd through the C ABI: (loss_out, g_disp, stats) on the CPU.  ``preset``: loss_out starts at this
    value and the forward runs with accumulate = 1."""
    from dvf import lib as L
    lib = L.lib()
    b, c, h, w = img.shape
    d, i = disp.to(DEV).contiguous(), img.to(DEV).contiguous()
    out = torch.full((1,), float("nan") if preset is None else preset, device=DEV)
    stats = torch.empty(b, 2, device=DEV)
    partials = torch.empty(int(lib.dvf_norm_smooth_partials_floats(b, h, w)), device=DEV)
    g = torch.full_like(d, float("nan"))
    gl = torch.full((1,), grad_loss, device=DEV)
    L.check(lib.dvf_norm_smooth_fwd(L.dev(d), L.dev(i), L.dev(out), L.dev(stats), L.dev(partials), b, c, h, w, in_scale, eps, weight,
                                    0 if preset is None else 1, L.stream()), "dvf_norm_smooth_fwd")
    L.check(lib.dvf_norm_smooth_bwd(L.dev(d), L.dev(i), L.dev(stats), L.dev(gl), L.dev(g), b, c, h, w, in_scale, eps, weight,
                                    L.stream()), "dvf_norm_smooth_bwd")
    torch.cuda.synchronize()
    return out.cpu()[0], g.cpu(), stats.cpu()


@pytest.mark.parametrize("in_scale", [1.0, 0.004])
@pytest.mark.parametrize("eps", [1e-7, 0.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_pair_vs_fp64_restatement(shape, eps, in_scale):
    """Loss and g_disp within 1e-4 of fp64 with weight 1.3 and an upstream gradient of 0.7; stats holds (mean + eps, T); a
    second run is bit-identical; accumulate = 1 adds the same loss to a preset loss_out.
    On an MI355X over the 28 cases: loss at most 2.6e-7, gradient at most 2.2e-7."""
    disp, img = _inputs(shape, in_scale)
    r_loss, r_grad = _reference(shape, in_scale, eps)
    loss, g, stats = _run_abi(disp, img, in_scale, eps, weight=1.3, grad_loss=0.7)
    loss2, g2, _ = _run_abi(disp, img, in_scale, eps, weight=1.3, grad_loss=0.7)
    acc, _, _ = _run_abi(disp, img, in_scale, eps, weight=1.3, grad_loss=0.7, preset=2.5)
    mean = disp.double().mean(dim=(2, 3)).flatten() + eps
    e_loss, e_grad, e_mean = rel_err(loss, 1.3 * r_loss), rel_err(g, 1.3 * 0.7 * r_grad), rel_err(stats[:, 0], mean)
    e_t = rel_err((stats[:, 1].double() / stats[:, 0].double()).sum(), r_loss)
    print(shape, eps, in_scale, "loss", e_loss, "gradient", e_grad, "mean", e_mean, "sum T / M", e_t)
    assert float(r_loss) > 0 and float(r_grad.abs().max()) > 0
    assert bool(torch.isfinite(g).all())                      # every element written
    assert e_loss < TOL and e_grad < TOL and e_mean < TOL and e_t < TOL
    assert torch.equal(loss, loss2) and torch.equal(g, g2)
    assert torch.equal(acc, torch.tensor(2.5) + loss)


@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (3, 1, 9, 130)])
def test_gradient_is_orthogonal_to_the_disparity_per_image(shape):
    """Degree-0 homogeneity on the device, eps = 0: |sum_p disp_p g_p| <= 1e-4 * sum_p |disp_p g_p| for every image.  A kernel
    that drops the mean term, or reads another image's stats row, fails this."""
    disp, img = _inputs(shape, 1.0)
    _, g, _ = _run_abi(disp, img, 1.0, 0.0)
    dg = (disp.double() * g.double()).flatten(1)
    for b in range(shape[0]):
        print(shape, b, abs(float(dg[b].sum())), float(dg[b].abs().sum()))
        assert float(dg[b].abs().sum()) > 0
        assert abs(float(dg[b].sum())) <= TOL * float(dg[b].abs().sum())


def test_constant_disparity_per_image_is_exactly_zero():
    gen = torch.Generator().manual_seed(7)
    img = torch.rand(3, 3, 9, 130, generator=gen) * 2 - 1
    disp = torch.tensor([0.5, 7.0, 0.01]).view(3, 1, 1, 1) * torch.ones(3, 1, 9, 130)
    for eps in (1e-7, 0.0):
        loss, g, _ = _run_abi(disp, img, 1.0, eps)
        assert float(loss) == 0.0 and float(g.abs().max()) == 0.0


def test_multiscale_loss_vs_fp64_restatement():
    """LS.normalized_smooth_loss on four scales of 2x3x32x104 (32x104 ... 4x13), scale_factor 2: the loss and the gradients of
    all four disparities against the restatement's multi-scale form (the image pyramid is F.interpolate(mode='area') there,
    dvf_area_downsample here)."""
    import loss_functions_sfm as LS
    gen = torch.Generator().manual_seed(11)
    img = torch.rand(2, 3, 32, 104, generator=gen) * 2 - 1
    disps = [_disparity(2, 32 >> s, 104 >> s, gen) for s in range(4)]
    ref_d = [d.double().requires_grad_(True) for d in disps]
    r_loss = NR.multiscale_normalized_smooth_loss(ref_d, img.double(), 2.0)
    r_loss.backward()
    gd = [d.to(DEV).requires_grad_(True) for d in disps]
    loss = LS.normalized_smooth_loss(gd, img.to(DEV), 2.0)
    (0.5 * loss).backward()
    torch.cuda.synchronize()
    errs = {"loss": rel_err(loss, r_loss)}
    for s in range(4):
        assert float(ref_d[s].grad.abs().max()) > 0
        errs[f"disp[{s}]"] = rel_err(gd[s].grad, 0.5 * ref_d[s].grad)
    print(errs)
    for n, e in errs.items():
        assert e < TOL, (n, e)
    # the single-scale entry point is the first scale of the same thing
    import loss_functions as LF
    one = LF.normalized_smooth_loss(disps[0].to(DEV), img.to(DEV))
    assert rel_err(one, NR.normalized_smooth_loss(disps[0].double(), img.double())) < TOL


# ------------------------------------------------------------------------------------------------ training steps
def _sfm_setup(lr=2e-4):
    """DispNetS + PoseExpNet_sfm at 2x3x64x208 (the size test_gpu_fullres._case uses), images brought to [-1, 1]."""
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
    opt = FlatAdam(list(disp.parameters()) + list(pose.parameters()), lr=lr, overlap=False)
    batch = synthetic_batch(2, 64, 208, seed=1234, device=DEV, n_views=2)
    for k in ("img_R2", "img_R1", "img_L2"):
        batch[k] = (batch[k] / 127.5 - 1.0).contiguous()
    return disp, pose, opt, batch


def _fwd_bwd(step_fn, nets, opt, batch, **kw):
    from dvf import lib as L
    loss, terms = step_fn(*nets, batch, **kw)
    opt.zero_grad()
    loss.backward()
    opt.join_wgrad()
    L.join_aux_streams()
    torch.cuda.synchronize()
    return terms, opt.flat_g.clone()


_RECIPE = dict(ssim_weight=0.85, min_reprojection=True, auto_mask=True, full_res_multiscale=True)


@pytest.mark.parametrize("combined", [False, True], ids=["alone", "whole-recipe"])
def test_train_form_step(combined):
    """train_sfm_losses(normalized_smoothness=True), alone and together with SSIM + minimum reprojection + auto-mask +
    full-resolution sampling: terms["smooth"] is the restatement applied to the network's own four disparities at their native
    sizes against the target image; every DispNetS parameter gets a finite, non-zero gradient; in deterministic mode two steps
    from the same state give bit-identical terms and gradient arenas."""
    from dvf import conv as C
    from dvf.steps import train_sfm_losses
    disp, pose, opt, batch = _sfm_setup()
    kw = dict(_RECIPE) if combined else {}
    C.set_deterministic(True)
    try:
        with torch.no_grad():
            own = [d.double().cpu() for d in disp(batch["img_R2"])]
        torch.cuda.synchronize()
        assert [tuple(d.shape[2:]) for d in own] == [(64, 208), (32, 104), (16, 52), (8, 26)]
        want = NR.multiscale_normalized_smooth_loss(own, batch["img_R2"].double().cpu(), 2.0)
        _fwd_bwd(train_sfm_losses, (disp, pose), opt, batch, normalized_smoothness=True, **kw)      # sizes every workspace
        t_a, g_a = _fwd_bwd(train_sfm_losses, (disp, pose), opt, batch, normalized_smoothness=True, **kw)
        t_b, g_b = _fwd_bwd(train_sfm_losses, (disp, pose), opt, batch, normalized_smoothness=True, **kw)
        t_off, _ = _fwd_bwd(train_sfm_losses, (disp, pose), opt, batch, **kw)
    finally:
        C.set_deterministic(False)
    e = rel_err(t_a["smooth"], want)
    print("combined", combined, "smooth", float(t_a["smooth"]), "restatement", float(want), "rel", e, "second-order term",
          float(t_off["smooth"]))
    assert float(want) > 0 and e < TOL
    assert float(t_off["smooth"]) != float(t_a["smooth"])
    assert all(bool(torch.isfinite(v)) for v in t_a.values()) and bool(torch.isfinite(g_a).all())
    for name, p in disp.named_parameters():
        assert bool(torch.isfinite(p._dvf_grad).all()) and float(p._dvf_grad.abs().max()) > 0, name
    for k in t_a:
        assert torch.equal(t_a[k], t_b[k]), k
    assert torch.equal(g_a, g_b)


def test_smoothness_term_alone_reaches_every_disparity_head():
    """The term's own gradient (no photometric term in front of it): backward through the four disparities of DispNetS into
    the network gives every parameter a finite gradient and every disparity head a non-zero one."""
    import loss_functions_sfm as LS
    disp, _, opt, batch = _sfm_setup()
    loss = LS.normalized_smooth_loss(disp(batch["img_R2"]), batch["img_R2"], 2.0)
    opt.zero_grad()
    loss.backward()
    opt.join_wgrad()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(opt.flat_g).all())
    heads = [n for n, _ in disp.named_parameters() if "predict_disp" in n]
    assert len(heads) >= 4
    for name, p in disp.named_parameters():
        if name in heads:
            assert float(p._dvf_grad.abs().max()) > 0, name


def test_unsupervise_form_step():
    """unsupervise_losses(normalized_smoothness=True, img_scale=0.004) at one scale, images in 0..255: terms["smooth"] is the
    restatement applied to the network's finest disparity with in_scale 0.004, and the step's gradients are finite."""
    import DispNetS
    import PoseExpNet
    from dvf import conv as C
    from dvf.engine import FlatAdam
    from dvf.steps import unsupervise_losses
    from dvf.synthetic import synthetic_batch
    torch.manual_seed(0)
    disp, pose = DispNetS.DispNetS(), PoseExpNet.PoseExpNet(output_exp=True)
    disp.init_weights()
    pose.init_weights()
    disp.to(DEV).train()
    pose.to(DEV).train()
    opt = FlatAdam(list(pose.parameters()) + list(disp.parameters()), lr=1e-3, overlap=False)
    batch = synthetic_batch(2, 64, 208, seed=1234, device=DEV)
    C.set_deterministic(True)
    try:
        with torch.no_grad():
            own = disp(batch["img_R2"])[0].double().cpu()
        want = NR.normalized_smooth_loss(own, batch["img_R2"].double().cpu(), 0.004)
        terms, g = _fwd_bwd(unsupervise_losses, (disp, pose), opt, batch, img_scale=0.004, normalized_smoothness=True)
        t_off, _ = _fwd_bwd(unsupervise_losses, (disp, pose), opt, batch, img_scale=0.004)
    finally:
        C.set_deterministic(False)
    e = rel_err(terms["smooth"], want)
    print("smooth", float(terms["smooth"]), "restatement", float(want), "rel", e, "second-order term", float(t_off["smooth"]))
    assert float(want) > 0 and e < TOL
    assert float(t_off["smooth"]) != float(terms["smooth"])
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_graph_replay_gives_the_eager_smoothness():
    """One GraphedStep replay of the train-form step (forward, backward, FlatAdam with lr = 0 so that the weights stay where
    they are) against the eager step on the same batch and weights."""
    from dvf import conv as C
    from dvf.engine import GraphedStep
    from dvf.steps import train_sfm_losses
    disp, pose, opt, batch = _sfm_setup(lr=0.0)

    def step():
        loss, terms = train_sfm_losses(disp, pose, batch, normalized_smoothness=True)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return (terms["smooth"], terms["total"])

    C.set_deterministic(True)
    try:
        step()
        eager = [float(t) for t in step()]
        graphed = GraphedStep(step, [], warmup=1)
        out = graphed()
        torch.cuda.synchronize()
        replayed = [float(t) for t in out]
    finally:
        C.set_deterministic(False)
    print("eager", eager, "replayed", replayed)
    assert eager[0] > 0 and eager[1] == eager[1]
    assert rel_err(replayed[0], eager[0]) < TOL and rel_err(replayed[1], eager[1]) < TOL


# ------------------------------------------------------------------------------------------------ command line
def _cli_smooth(script, extra, tmp_path, tag):
    cmd = [sys.executable, os.path.join(PKG, script), "-b", "2", "--epochs", "1", "--steps-per-epoch", "2", "--height", "64",
           "--width", "208", "--output-dir", str(tmp_path / tag)] + extra
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("Train epoch")]
    assert len(lines) == 1, res.stdout[-2000:]
    v = float(lines[0].split("smooth:")[1].split()[0])
    assert v == v and abs(v) < 1e6, lines[0]
    return v


@pytest.mark.parametrize("script,weight", [("train.py", ["-s", "0.001"]), ("unsupervise.py", ["--smooth-weight", "0.001"])])
def test_cli_flag(script, weight, tmp_path):
    """The entry script as a fresh process, two steps at 2x3x64x208 with the recommended weight: exits 0 and prints a finite
    `smooth:` value that differs from the run without the flag."""
    on = _cli_smooth(script, weight + ["--normalized-smoothness"], tmp_path, "on")
    off = _cli_smooth(script, weight, tmp_path, "off")
    print(script, "smooth with the flag", on, "without", off)
    assert on != off
