"""CPU: what tests/test_gpu_resize_validation.py relies on, asserted on torch alone.  The affine restatement of
tests/resize_cases.py IS aten's fp64 bilinear resize; aten's own fp32 resize of the noise inputs is as far from fp64 as
expected (1.8e-6 at (16,52)->(37,122), 2.8e-5 at (128,416)->(375,1242), rel_err, growing with the size), which is what the GPU
test's bound max(1e-6, 4 * dev) is built from; the validation case has an image without a valid pixel, pixels beyond the cap,
and no pixel whose ratio lies within depth_metrics_ref.NEAR of a threshold in any of the three configurations run."""
import pytest
import torch

import resize_cases as C
from conftest import rel_err


@pytest.mark.parametrize("src,dst", C.AFFINE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_affine_restatement_is_atens_fp64_resize(src, dst):
    want, inside, span = C.affine_expected(src, dst)
    ref = C.interpolate(C.affine(*src).double(), dst)
    assert float((want - ref).abs().max()) < 1e-12 * span
    sy, sx = C.src_coords(src[0], dst[0]), C.src_coords(src[1], dst[1])
    a, b, c = C.AFFINE
    free = a * sx[None, :] + b * sy[:, None] + c                              # the field at the unclamped coordinate
    assert torch.equal(free[inside], want[0][inside])
    if src[0] < dst[0] or src[1] < dst[1]:                                    # an axis that grows has samples beyond the ends
        assert bool(inside.any()) and not bool(inside.all())                  # interior and clamped border both occur
        assert float((free - want[0])[~inside].abs().min()) > 1e-3 * span     # ... and the clamp changes the value there
    elif src != dst:
        assert bool(inside.all())
    else:
        assert bool(inside.all()) and torch.equal(want, C.affine(*src).double())


def test_affine_cases_tell_the_axes_apart():
    """Swapped scales, a missing half-pixel offset or align_corners = True each move an affine case by more than ten times
    the GPU test's 1e-5 of the range."""
    for src, dst in C.AFFINE_SHAPES:
        if src == dst:
            continue
        want, _, span = C.affine_expected(src, dst)
        x = C.affine(*src).double()[None]
        aligned = torch.nn.functional.interpolate(x, dst, mode="bilinear", align_corners=True)[0]
        assert float((aligned - want).abs().max()) > 1e-4 * span
        a, b, c = C.AFFINE
        sy = ((src[0] / dst[0]) * torch.arange(dst[0], dtype=torch.float64)).clamp(0, src[0] - 1)      # no half-pixel offset
        sx = ((src[1] / dst[1]) * torch.arange(dst[1], dtype=torch.float64)).clamp(0, src[1] - 1)
        assert float((a * sx[None, :] + b * sy[:, None] + c - want[0]).abs().max()) > 1e-4 * span
    assert any(s[0] / d[0] > 1 > s[1] / d[1] for s, d in C.AFFINE_SHAPES) and any(s[0] / d[0] < 1 < s[1] / d[1] for s, d in C.AFFINE_SHAPES)


@pytest.mark.parametrize("planes,src,dst", C.SHAPES, ids=lambda s: "%dx%d" % s if isinstance(s, tuple) else str(s))
def test_atens_fp32_deviation_on_the_noise_inputs(planes, src, dst):
    x = C.noise(planes, *src)
    assert float(x.min()) >= 0.01 and x.dtype == torch.float32
    dev = rel_err(C.interpolate(x, dst), C.interpolate(x.double(), dst))
    print(f"{src}->{dst}: aten fp32 against fp64 {dev:.3g}")
    assert dev < 1e-4
    if src == (1, 1):
        assert rel_err(C.interpolate(x.double(), dst), x.double().expand(planes, *dst)) < 1e-15
    if src == dst:
        assert torch.equal(C.interpolate(x.double(), dst), x.double())


@pytest.fixture(scope="module")
def validation():
    return C.make_validation()


def test_validation_case_shapes_and_the_empty_image(validation):
    assert len(validation.loader) == 2
    for k, ((img, gt), size) in enumerate(zip(validation.loader, C.GT_SIZES)):
        assert tuple(img.shape) == (C.BATCH, 3) + C.IMG and tuple(gt.shape) == (C.BATCH,) + size
        assert img.dtype == gt.dtype == torch.float32 and float(gt.min()) == 0.0
        for i in range(C.BATCH):
            valid = int(((gt[i] > 0) & (gt[i] < 80)).sum())
            assert (valid == 0) == ((k, i) == C.EMPTY), (k, i, valid)
    assert any(bool((gt > 80).any()) for _, gt in validation.loader)
    disp = validation.stub(validation.loader[0][0])
    assert type(disp) is list and tuple(disp[0].shape) == (C.BATCH, 1, C.IMG[0] // 4, C.IMG[1] // 4)
    assert float(disp[0].min()) > 0.01 and float(disp[0].max() - disp[0].min()) > 1.0


@pytest.mark.parametrize("crop,median_scaling", [(True, True), (False, True), (True, False)])
def test_validation_case_has_no_pixel_near_a_threshold(validation, crop, median_scaling):
    disps = [validation.stub(img)[0] for img, _ in validation.loader]
    mean, rows, near = C.expected_metrics(disps, validation.loader, crop=crop, median_scaling=median_scaling)
    assert all(int(n.sum()) == 0 for n in near), near
    assert sum(int((r[:, 8] > 0).sum()) for r in rows) == 2 * C.BATCH - 1
    assert float(rows[C.EMPTY[0]][C.EMPTY[1]].abs().sum()) == 0.0
    assert bool((mean[:5] > 0).all()) and bool(torch.isfinite(mean).all())
    if median_scaling:
        assert 0.05 < float(mean[5]) < 0.95                                   # a1 has pixels on both sides
    # the mean divides by the number of images WITH a valid pixel, not by the number of images
    wrong = sum(r[:, :8].sum(0) for r in rows) / (2 * C.BATCH)
    assert rel_err(wrong[1], mean[1]) > 0.1
