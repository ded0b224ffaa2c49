"""The non-convolution kernels of the cfg 2-5 steps, alone, at the shapes those steps run them, against fp64 torch CPU.

Every grid-stride kernel of csrc/elementwise.hip launches at most 4096 x 256 threads (nblocks()), so its loop takes a
second iteration only above 1,048,576 elements; each group below has at least one case above that, besides the bench
shapes and ragged ones.  The depthwise transposed convolution (FeatExtractor's top-down path) is checked at its four
levels at cfg 3 (N = 24) and cfg 4 (N = 12), with bias / skip absent and every needs_input_grad combination.  The bce_ones
kernels (explainability_loss) run at cfg 5's mask size over four scales, with entries at aten's clamps.
Bounds: 1e-6 relative (max-abs error / max-abs reference) for the elementwise kernels, 1e-5 for the reductions."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
EW = 1e-6          # elementwise kernels
RED = 1e-5         # reductions
GRID_STRIDE = 4096 * 256


# ---------------------------------------------------------------------------------------------------- depthwise up-conv
# FeatExtractor (feat_extractor.py): c3 levels at full, 1/2, 1/4, 1/8, 1/16 resolution; the four top-down steps take
# 1/16 -> 1/8, ..., 1/2 -> 1.  Input sizes of those steps at 256x832: 16x52, 32x104, 64x208, 128x416.
_FEAT_LEVELS = [(16, 52), (32, 104), (64, 208), (128, 416)]
_DW_SHAPES = [(24, 32, h, w) for h, w in _FEAT_LEVELS] + [(12, 32, h, w) for h, w in _FEAT_LEVELS] + \
             [(3, 32, 37, 75), (2, 5, 33, 61), (1, 7, 1, 1), (5, 3, 301, 411)]


def _dw_ref(x, w, b, skip):
    y = F.conv_transpose2d(x, w, b, stride=2, padding=1, groups=x.shape[1])
    return y + skip if skip is not None else y


@pytest.mark.parametrize("n,c,h,w", _DW_SHAPES)
def test_depthwise_up2x_vs_torch(n, c, h, w):
    """Forward, dx, dw and db of DepthwiseUp2xFn (dvf_dwconvt4x4s2_fwd / _bwd) against fp64 conv_transpose2d + skip.
    dy is random, so that the bias gradient (a sum over N * 4HW pixels) does not cancel."""
    from dvf.conv import DepthwiseUp2xFn
    g = torch.Generator().manual_seed(n * 100003 + c * 1009 + h * 13 + w)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.rand(c, 1, 4, 4, generator=g) * 0.5 - 0.25
    b = torch.rand(c, generator=g) * 0.5 - 0.25
    skip = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    dy = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    rl = [t.double().requires_grad_(True) for t in (x, wt, b, skip)]
    ref = _dw_ref(*rl)
    ref.backward(dy.double())
    gl = [t.to(DEV).requires_grad_(True) for t in (x, wt, b, skip)]
    out = DepthwiseUp2xFn.apply(*gl)
    out.backward(dy.to(DEV))
    errs = {"fwd": rel_err(out, ref), "dx": rel_err(gl[0].grad, rl[0].grad), "dw": rel_err(gl[1].grad, rl[1].grad),
            "db": rel_err(gl[2].grad, rl[2].grad), "dskip": rel_err(gl[3].grad, rl[3].grad)}
    assert tuple(out.shape) == (n, c, 2 * h, 2 * w)
    bad = {k: v for k, v in errs.items() if not v < RED}
    assert not bad, ((n, c, h, w), bad)


@pytest.mark.parametrize("with_bias,with_skip", [(True, True), (False, True), (True, False), (False, False)])
def test_depthwise_up2x_optional_inputs_and_grads(with_bias, with_skip):
    """bias=None / skip=None, and every combination of which inputs need a gradient: each gradient that is asked for is
    the reference's, whatever else is asked for (a trainable bias beside a frozen weight included)."""
    from dvf.conv import DepthwiseUp2xFn
    n, c, h, w = 3, 6, 19, 27
    g = torch.Generator().manual_seed(77 + 2 * with_bias + with_skip)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.rand(c, 1, 4, 4, generator=g) * 0.5 - 0.25
    b = torch.rand(c, generator=g) * 0.5 - 0.25 if with_bias else None
    skip = torch.randn(n, c, 2 * h, 2 * w, generator=g) if with_skip else None
    dy = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    present = [True, True, with_bias, with_skip]
    for need in itertools.product((False, True), repeat=4):
        need = [nd and p for nd, p in zip(need, present)]
        if not any(need):
            continue
        src = (x, wt, b, skip)
        rl = [t.double().requires_grad_(nd) if t is not None else None for t, nd in zip(src, need)]
        ref = _dw_ref(*rl)
        ref.backward(dy.double())
        gl = [t.to(DEV).requires_grad_(nd) if t is not None else None for t, nd in zip(src, need)]
        out = DepthwiseUp2xFn.apply(*gl)
        out.backward(dy.to(DEV))
        assert rel_err(out, ref) < EW, need
        for name, a, r, nd in zip(("x", "weight", "bias", "skip"), gl, rl, need):
            if nd:
                assert a.grad is not None, (need, name)
                assert rel_err(a.grad, r.grad) < RED, (need, name)


# ---------------------------------------------------------------------------------------------------- elementwise kernels
@pytest.mark.parametrize("n,c,h,w", [(24, 3, 256, 832), (24, 3, 128, 416), (24, 3, 64, 208),      # cfg 3 pyramid
                                     (8, 3, 384, 1280), (8, 3, 192, 640), (8, 3, 96, 320),        # 384x1280
                                     (8, 3, 375, 1243), (8, 3, 187, 621), (2, 3, 3, 5)])          # odd sizes
def test_bilinear_half_vs_torch(n, c, h, w):
    """FeatExtractor's image pyramid step: F.interpolate(scale_factor=0.5, mode='bilinear') (feat_extractor.py)."""
    from dvf.conv import bilinear_half
    x = torch.rand(n, c, h, w, generator=torch.Generator().manual_seed(h * 7 + w)) * 255
    ref = F.interpolate(x.double(), scale_factor=0.5, mode="bilinear")
    out = bilinear_half(x.to(DEV))
    assert tuple(out.shape) == tuple(ref.shape)
    assert rel_err(out, ref) < EW
    if (n, h) in ((24, 256), (8, 375)):
        assert out.numel() > GRID_STRIDE


# loss_functions_sfm.photometric_reconstruction_loss: target and references area-downsampled to each disparity scale
@pytest.mark.parametrize("n,h,w,oh,ow", [(4, 256, 832, 128, 416), (4, 256, 832, 64, 208), (4, 256, 832, 32, 104),   # cfg 4
                                         (8, 384, 1280, 192, 640), (8, 384, 1280, 96, 320), (8, 384, 1280, 48, 160),  # cfg 5
                                         (8, 375, 1242, 192, 640), (3, 37, 75, 10, 31)])      # non-integer ratios
def test_area_downsample_vs_torch(n, h, w, oh, ow):
    from dvf.conv import area_downsample
    x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(oh * 7 + ow)) * 255
    ref = F.interpolate(x.double(), (oh, ow), mode="area")
    out = area_downsample(x.to(DEV), (oh, ow))
    assert tuple(out.shape) == tuple(ref.shape)
    assert rel_err(out, ref) < EW
    if n == 8 and oh == 192:
        assert out.numel() > GRID_STRIDE


# DispNetS: disparity 4 -> 3 -> 2 -> 1 upsampled x2 and cropped to the next level (DispNetS.py:115,121,127); cfg 5 (N = 8)
@pytest.mark.parametrize("n,c,h,w,oh,ow", [(8, 1, 48, 160, 96, 320), (8, 1, 96, 320, 192, 640), (8, 1, 192, 640, 384, 1280),
                                           (8, 2, 199, 411, 397, 821), (3, 1, 5, 7, 9, 14), (2, 1, 6, 8, 12, 16)])
def test_upsample2x_vs_torch(n, c, h, w, oh, ow):
    """Upsample2xFn: forward (dvf_resize_bilinear_fwd, scale 0.5) and its gather-form backward (dvf_upsample2x_bwd)
    against F.interpolate(scale_factor=2, bilinear) + crop."""
    from dvf.conv import Upsample2xFn
    g = torch.Generator().manual_seed(h * 31 + w)
    x = torch.rand(n, c, h, w, generator=g) * 10
    gy = torch.randn(n, c, oh, ow, generator=g)
    rx = x.double().requires_grad_(True)
    ref = F.interpolate(rx, scale_factor=2, mode="bilinear", align_corners=False)[:, :, :oh, :ow]
    ref.backward(gy.double())
    gx = x.to(DEV).requires_grad_(True)
    out = Upsample2xFn.apply(gx, (oh, ow))
    out.backward(gy.to(DEV))
    assert tuple(out.shape) == tuple(ref.shape)
    assert rel_err(out, ref) < EW and rel_err(gx.grad, rx.grad) < EW
    if (h, w) in ((192, 640), (199, 411)):
        assert out.numel() > GRID_STRIDE
    if (h, w) == (199, 411):
        assert gx.numel() > GRID_STRIDE


@pytest.mark.parametrize("eps", [0.0, 1e-4])
def test_reciprocal_vs_torch(eps):
    """disparity -> depth at cfg 5's finest scale, 8x1x384x1280 (train.py:188 eps = 0, unsupervise.py:99 eps = 1e-4);
    disparities in DispNetS' range 0.01 .. 10.01.  Also elementwise: each value within 1e-6 of its own."""
    from dvf.conv import reciprocal
    g = torch.Generator().manual_seed(5)
    x = torch.rand(8, 1, 384, 1280, generator=g) * 10 + 0.01
    gy = torch.randn(8, 1, 384, 1280, generator=g)
    rx = x.double().requires_grad_(True)
    ref = 1 / (rx + eps)
    ref.backward(gy.double())
    gx = x.to(DEV).requires_grad_(True)
    out = reciprocal(gx, eps)
    out.backward(gy.to(DEV))
    assert x.numel() > GRID_STRIDE
    assert rel_err(out, ref) < EW and rel_err(gx.grad, rx.grad) < EW
    assert float(((out.double().cpu() - ref) / ref).abs().max()) < EW
    assert float(((gx.grad.double().cpu() - rx.grad) / rx.grad).abs().max()) < EW


# PoseExpNet_sfm's pose head: pose_pred over the 1/128 map, mean over H, W, times 0.01 (PoseExpNet_sfm.py:42)
@pytest.mark.parametrize("n,c,h,w", [(8, 24, 3, 10), (4, 12, 2, 7), (64, 24, 24, 40), (3, 5, 17, 1)])
def test_spatial_mean_vs_torch(n, c, h, w):
    from dvf.conv import SpatialMeanFn
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + w)
    x = torch.randn(n, c, h, w, generator=g)
    gy = torch.randn(n, c, generator=g)
    rx = x.double().requires_grad_(True)
    ref = 0.01 * rx.mean(3).mean(2)
    ref.backward(gy.double())
    gx = x.to(DEV).requires_grad_(True)
    out = SpatialMeanFn.apply(gx, 0.01)
    out.backward(gy.to(DEV))
    assert rel_err(out, ref) < RED and rel_err(gx.grad, rx.grad) < EW
    if n == 64:
        assert x.numel() > GRID_STRIDE


# ---------------------------------------------------------------------------------------------------- explainability
def test_explainability_loss_vs_torch_bce():
    """explainability_loss over cfg 5's four mask scales (8x4x384x1280 = 15.7 M elements at the finest; the scales are
    summed through the kernel's accumulate flag) against the reference's own call, fp64 F.binary_cross_entropy(m, 1).
    The masks include exact zeros, entries below e^-100 (log clamped at -100), entries below aten's 1e-12 gradient
    clamp, and exact ones (gradient 0)."""
    import loss_functions_sfm as LS
    g = torch.Generator().manual_seed(11)
    masks = []
    for s in range(4):
        m = torch.sigmoid(torch.randn(8, 4, 384 >> s, 1280 >> s, generator=g) * 3)
        flat = m.view(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:4000]
        flat[idx[:1000]] = 0.0
        flat[idx[1000:2000]] = 1e-44                  # below e^-100 = 3.7e-44 (a float32 denormal)
        flat[idx[2000:3000]] = 1e-30                  # log above the clamp, (1 - m) m below 1e-12
        flat[idx[3000:]] = 1.0
        masks.append(m)
    assert masks[0].numel() == 8 * 4 * 384 * 1280 > GRID_STRIDE
    rm = [m.double().requires_grad_(True) for m in masks]
    ref = sum(F.binary_cross_entropy(m, torch.ones_like(m)) for m in rm)
    ref.backward()
    gm = [m.to(DEV).requires_grad_(True) for m in masks]
    out = LS.explainability_loss(gm)
    out.backward()
    assert torch.isfinite(out) and rel_err(out, ref) < RED, (float(out), float(ref))
    for s, (a, r, m) in enumerate(zip(gm, rm, masks)):
        ga, gr = a.grad.double().cpu(), r.grad
        assert torch.isfinite(ga).all(), s
        assert rel_err(ga, gr) < EW, s                 # dominated by the clamped entries
        normal = (m > 1e-6) & (m < 1)
        assert rel_err(ga[normal], gr[normal]) < EW, s
        assert float(((ga[normal] - gr[normal]) / gr[normal]).abs().max()) < 1e-5, s
        assert torch.equal(ga[m == 1], gr[m == 1]), s  # exactly 0
