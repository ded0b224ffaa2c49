"""dvf_resize_bilinear_fwd at the scales dvf.validation.validate_depth calls it with (h / Hg, w / Wg: non-dyadic, above and
below 1, different per axis) against torch's fp64 F.interpolate, and validate_depth itself against its definition restated
from torch alone (tests/resize_cases.py) -- the only other test of that pass, test_gpu_cli_depth_val.py, builds its expected
value with the same kernel.

Bounds.  Noise inputs: the kernel within max(1e-6, 4 * dev) of fp64 (conftest.rel_err), dev being the distance of torch's own
fp32 CPU resize of the same input from fp64: the fp32 source coordinate scale * (dst + 0.5) - 0.5 is an ulp or two of the
coordinate off in either implementation, on either side, and noise turns that into value.  Affine field: 1e-5 of the field's
range from the field at the fp64 source coordinate, clamped at the border, which does not depend on noise.  validate_depth:
the five error means within 1e-4 (as test_gpu_depth_metrics.py), a1..a3 equal up to the pixels depth_metrics_ref reports as
near a threshold (none for this case: tests/test_resize_cases.py).
Measured, rel_err against fp64 as (dev, kernel): (16,52)->(37,122) 1.78e-6, 1.78e-6; (16,52)->(40,130) 2.08e-6, 2.08e-6;
(48,160)->(37,122) 7.94e-6, 7.94e-6; (7,5)->(3,9) 2.79e-7, 2.79e-7; (1,1)->(4,6) 6.0e-8, 6.0e-8; (2,3)->(2,3) 0, 0;
3 x (128,416)->(375,1242) 2.83e-5, 2.83e-5 -- the kernel lands where aten's fp32 does at every shape.  Affine field: at most
1.7e-7 of the range.  validate_depth: worst error-mean deviation 4.9e-7 (crop off); a1..a3 equal, no pixel near a threshold."""
import pytest
import torch

import resize_cases as C
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
EW = 1e-6


def _resize(x, dst):
    from dvf import lib as L
    planes, h, w = x.shape
    g = x.to(DEV).contiguous()
    out = torch.empty(planes, dst[0], dst[1], device=DEV, dtype=torch.float32)
    L.check(L.lib().dvf_resize_bilinear_fwd(L.dev(g, "input"), L.dev(out), planes, h, w, dst[0], dst[1], h / dst[0], w / dst[1],
                                            L.stream()), "dvf_resize_bilinear_fwd")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("planes,src,dst", C.SHAPES, ids=lambda s: "%dx%d" % s if isinstance(s, tuple) else str(s))
def test_resize_general_scale_vs_fp64(planes, src, dst):
    x = C.noise(planes, *src)
    ref = C.interpolate(x.double(), dst)
    dev = rel_err(C.interpolate(x, dst), ref)
    out = _resize(x, dst)
    err = rel_err(out, ref)
    print(f"{planes} x {src}->{dst}: aten fp32 dev {dev:.3g}, kernel {err:.3g}, bound {max(EW, 4 * dev):.3g}")
    assert tuple(out.shape) == (planes,) + dst
    assert err < max(EW, 4 * dev), (err, dev)
    if src == dst:                                      # weights 1 and 0: the input's own bits
        assert torch.equal(out, x)


@pytest.mark.parametrize("src,dst", C.AFFINE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_resize_affine_field_pins_offset_scales_and_clamp(src, dst):
    want, inside, span = C.affine_expected(src, dst)
    out = _resize(C.affine(*src), dst).double()
    err_in = float((out - want)[0][inside].abs().max()) / span
    err_out = float((out - want)[0][~inside].abs().max()) / span if not bool(inside.all()) else 0.0
    print(f"affine {src}->{dst}: interior {err_in:.3g}, clamped border {err_out:.3g} of the range")
    assert err_in < 1e-5 and err_out < 1e-5


# ------------------------------------------------------------------------------------------------ validate_depth
@pytest.fixture(scope="module")
def validation():
    case = C.make_validation()
    case.stub.to(DEV)
    with torch.no_grad():
        case.disps = [case.stub(img.to(DEV))[0] for img, _ in case.loader]
    return case


@pytest.mark.parametrize("crop,median_scaling", [(True, True), (False, True), (True, False)])
def test_validate_depth_against_its_definition(validation, crop, median_scaling):
    from dvf.metrics import METRICS
    from dvf.validation import validate_depth
    validation.stub.train()
    got = validate_depth(validation.stub, validation.loader, DEV, crop=crop, median_scaling=median_scaling)
    assert validation.stub.training                      # the pass restores the mode it found
    assert tuple(got) == tuple(METRICS)
    want, rows, near = C.expected_metrics(validation.disps, validation.loader, crop=crop, median_scaling=median_scaling)
    images = sum(int((r[:, 8] > 0).sum()) for r in rows)
    assert images == 2 * C.BATCH - 1
    worst = 0.0
    for c, k in enumerate(METRICS[:5]):
        err = rel_err(got[k], want[c])
        worst = max(worst, err)
        assert err < 1e-4, (k, got[k], float(want[c]))
    for e, k in enumerate(METRICS[5:]):
        # per image a_e = count / n_valid: `near` pixels of an image may fall on the other side of the threshold
        slack = sum(float(n[i, e]) / float(r[i, 8]) for r, n in zip(rows, near) for i in range(r.shape[0]) if r[i, 8] > 0) / images
        assert abs(got[k] - float(want[5 + e])) <= slack + 1e-6, (k, got[k], float(want[5 + e]), slack)
    print(f"validate_depth crop={crop} median_scaling={median_scaling}: worst error-mean deviation {worst:.3g}; "
          f"near-threshold pixels {sum(int(n.sum()) for n in near)}")
