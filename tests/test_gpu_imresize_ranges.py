"""dvf.image_ops.gpu_imresize (dvf_imresize_u8, csrc/image_io.hip) against the host path un_dataset.imresize, EXACTLY
(np.array_equal, as test_gpu_image_ops.py), over what that test's integers(7, 240) x 3-channel images never reach: other
(min, max) pairs -- the identity, a constant image (the cscale = 1 branch), two adjacent values (the largest scale), the
+ 0.5 truncation at other scales -- and C = 1, an axis whose size does not change, a large down-scale (ksize 27 and 33, windows
clipped at both ends) and one-pixel sources and destinations.  Images: tests/imresize_cases.py."""
import numpy as np
import pytest
import torch

import imresize_cases as I

pytestmark = pytest.mark.gpu


def _check(img, dst):
    from dvf.image_ops import gpu_imresize
    ref = I.host(img, dst)
    out = gpu_imresize(torch.from_numpy(img).cuda(), dst)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (img.shape[2], dst[0], dst[1])
    got = out.cpu().numpy()
    assert np.array_equal(got, ref), (int((got != ref).sum()), float(np.abs(got - ref).max()))
    return got


@pytest.mark.parametrize("lo,hi", I.RANGES)
@pytest.mark.parametrize("src,dst", I.RANGE_SIZES, ids=lambda s: "%dx%d" % s)
def test_value_ranges(src, dst, lo, hi):
    got = _check(I.image(lo, hi, *src), dst)
    if lo == hi:
        assert not got.any()                    # the constant image: bytescale gives 0 everywhere


@pytest.mark.parametrize("src,dst,c", I.SHAPES, ids=lambda s: "%dx%d" % s if isinstance(s, tuple) else "C%d" % s)
def test_shapes(src, dst, c):
    _check(I.image(*I.BASE, *src, c=c), dst)
