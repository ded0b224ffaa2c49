"""CPU: the images of tests/imresize_cases.py have the value ranges they claim, the host path does to them what the GPU test
expects the kernel to reproduce (a constant image becomes 0, a full-range image is resized as it is, a two-valued image
becomes {0, 255} before the resize), and the coefficient tables of the shape cases have the sizes and clipped windows
imresize_cases.SHAPES claims."""
import numpy as np
import pytest

import imresize_cases as I
import un_dataset


@pytest.mark.parametrize("lo,hi", I.RANGES)
@pytest.mark.parametrize("src,dst", I.RANGE_SIZES, ids=lambda s: "%dx%d" % s)
def test_range_images(src, dst, lo, hi):
    img = I.image(lo, hi, *src)
    assert img.dtype == np.uint8 and img.shape == src + (3,)
    assert int(img.min()) == lo and int(img.max()) == hi
    assert set(np.unique(img).tolist()) == set(range(lo, hi + 1))
    scaled = un_dataset.bytescale(img.astype(np.float32))
    if lo == hi:
        assert not scaled.any()                                         # cscale = 1: (v - min) * 255 = 0
    elif (lo, hi) == (0, 255):
        assert np.array_equal(scaled, img)
    else:
        assert int(scaled.min()) == 0 and int(scaled.max()) == 255
    if hi - lo == 1:
        assert set(np.unique(scaled).tolist()) == {0, 255}
    out = I.host(img, dst)
    assert out.shape == (3,) + dst and out.dtype == np.float32
    if lo != hi:
        assert len(np.unique(out)) > 2                                   # the resize mixes: not a copy of two levels


def test_ranges_give_different_scales():
    scales = {np.float32(255.0 / max(hi - lo, 1)) for lo, hi in I.RANGES}
    assert len(scales) == 5         # 1 (identity and constant), 255/254 (twice), 255 (twice, at min 0 and 7), 255/127, 51
    assert I.BASE not in I.RANGES


@pytest.mark.parametrize("src,dst,c", I.SHAPES, ids=lambda s: "%dx%d" % s if isinstance(s, tuple) else "C%d" % s)
def test_shape_images_and_tables(src, dst, c):
    from dvf.image_ops import _coeffs
    img = I.image(*I.BASE, *src, c=c)
    assert img.shape == src + (c,) and int(img.min()) == I.BASE[0] and int(img.max()) == I.BASE[1]
    out = I.host(img, dst)
    assert out.shape == (c,) + dst
    for n_in, n_out in ((src[0], dst[0]), (src[1], dst[1])):
        bounds, fixed, ksize = _coeffs(n_in, n_out)
        assert bounds[0, 0] == 0 and bounds[-1, 0] + bounds[-1, 1] == n_in          # the windows reach both ends
        assert (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= ksize).all()
        if n_in == n_out:                                                           # unchanged axis: the identity table
            assert (fixed[:, 0] == 1 << 22).all() and not fixed[:, 1:].any()
    if (src, dst) == ((97, 311), (8, 20)):
        assert (_coeffs(97, 8)[2], _coeffs(311, 20)[2]) == (27, 33)
        for n_in, n_out in ((97, 8), (311, 20)):
            b = _coeffs(n_in, n_out)[0]
            full = int(b[:, 1].max())
            assert b[0, 1] < full and b[-1, 1] < full                               # clipped at both ends
