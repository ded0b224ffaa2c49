"""Images for dvf_imresize_u8 (bytescale + PIL's fixed-point bilinear resize, csrc/image_io.hip) over value ranges and shapes
(tests/test_imresize_cases.py, tests/test_gpu_imresize_ranges.py).  The reference is the host path, un_dataset.imresize.

bytescale maps [min, max] to [0, 255] with s = 255 / (max - min) in fp32 and truncates after + 0.5; max == min takes
cscale = 1 and maps everything to 0.  test_gpu_image_ops.py draws integers(7, 240) everywhere: one (min, max) = (7, 239),
one s.  RANGES adds the identity (0, 255), its two neighbours, the largest scale (two adjacent values, at 0 and away from
it), a constant image, a scale below 2 with an odd span, and a narrow range at the top."""
import numpy as np

import un_dataset

RANGES = [(0, 255), (0, 254), (1, 255), (0, 1), (7, 8), (100, 100), (3, 130), (250, 255)]
RANGE_SIZES = [((37, 123), (64, 128)), ((64, 128), (37, 123))]
BASE = (7, 239)
# (source, destination, channels) at range BASE
SHAPES = [
    ((37, 123), (64, 128), 1),          # C = 1 (PIL takes a 2-D array)
    ((40, 60), (40, 90), 3),            # the height does not change: PIL skips the vertical pass, the kernel runs an identity table
    ((40, 60), (25, 60), 3),            # the width does not change
    ((97, 311), (8, 20), 3),            # large down-scale: ksize 27 and 33, xmin / xn clipped at both ends
    ((5, 7), (1, 1), 3),                # one-pixel destination: one window over the whole source
    ((1, 1), (4, 6), 3),                # one-pixel source (per channel a constant; the three channels span the range)
    ((2, 2), (3, 3), 3),
]


def image(lo, hi, h, w, c=3, seed=0):
    """uint8 [h, w, c] with min = lo and max = hi: every value of [lo, hi] occurs where the image has room for all of
    them (lo and hi always do), the other pixels are uniform in [lo, hi]."""
    rng = np.random.default_rng(100000 * lo + 1000 * hi + 10 * h + w + c + seed)
    flat = rng.integers(lo, hi + 1, size=h * w * c, dtype=np.int64)
    every = np.arange(lo, hi + 1) if hi - lo + 1 <= flat.size else np.array([lo, hi])
    flat[rng.permutation(flat.size)[:every.size]] = every
    return flat.astype(np.uint8).reshape(h, w, c)


def host(img, dst):
    """The loaders' host path on a uint8 [h, w, c] image: float32 [c, OH, OW]."""
    arr = img.astype(np.float32)
    out = un_dataset.imresize(arr[:, :, 0] if img.shape[2] == 1 else arr, dst)
    return (out[:, :, None] if out.ndim == 2 else out).astype(np.float32).transpose(2, 0, 1)
