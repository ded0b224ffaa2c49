"""Inputs and the fp64 truth for the second-order smoothness kernels at their seams (tests/test_smooth_seams_inputs.py,
tests/test_gpu_smooth_seams.py).

smooth_fwd_kernel / smooth_bwd_kernel (csrc/warp_loss.hip) work on tiles of SX = 64 columns by SY = 4 rows with a halo of 2.
The forward guards a stencil by its origin (x + 2 < W, x + 1 < W && y + 1 < H, y + 2 < H); the gather-form backward has twelve
guarded terms, each reading the halo: three per second difference along an axis (the pixel is the stencil's first, middle or
last sample) and four for the two mixed terms (the pixel is one of the 2x2 corners).  SHAPES lists, per shape, which of these
guards it is the first to put on a tile seam or on the image's edge inside a partial tile.

Two input families per shape.  "float": seeded rand * 10 + 0.5, as the golden fixture; every second difference is far from 0
(min_abs_term()), so every sign is the same in fp32 and fp64.  "int": integers in [-3, 3] with a flat band across a seam (flat_band()); every difference is exact in any
precision, many are exactly 0 (sgn(0) = 0 is the contract: |.|'s subgradient as autograd takes it), and a gradient element is
exactly 0 only where the three integer sign sums are 0 each (zero_is_structural()), never through two different weights
cancelling -- so an fp32 kernel has to give an exact 0 there as well."""
import torch

from oracle import losses as ol

SX, SY, HALO = 64, 4, 2

# (B, C, H, W) -> the guards of smooth_bwd_kernel (and of smooth_fwd_kernel) the shape stands for
SHAPES = {
    (2, 1, 3, 3): "every stencil clipped: x - 2 >= 0, x + 2 < W, y - 2 >= 0, y + 2 < H hold at one pixel each; "
                  "x - 1 >= 0 && x + 1 < W only at the middle column; fwd: one dx2 / dy2 origin per row / column",
    (1, 1, 4, 64): "exactly one tile: x + 1 < W and x + 2 < W fail at columns 63 / 62-63 inside the tile, y + 1 < H at "
                   "row 3; the right and lower halo is all padding",
    (2, 1, 5, 65): "one past both seams: x - 2 >= 0 and x - 1 >= 0 read the left halo at column 64, x + 1 < W at column "
                   "63|64 reads the right halo, y + 1 < H / y - 1 >= 0 across row 3|4; the second tiles hold one pixel row / column",
    (1, 2, 6, 66): "x + 2 < W at columns 62, 63 reads both right-halo columns; x - 2 >= 0 at 64, 65 both left-halo columns; "
                   "y + 2 < H at rows 2, 3 both lower-halo rows; two planes (blockIdx.z as the plane index)",
    (1, 1, 7, 67): "as 6x66 with one more row and column: x - 1 >= 0 && x + 1 < W holds at columns 64, 65 of a 3-column "
                   "tile; y + 2 < H in a partial tile (rows 4..6, only row 4 passes)",
    (3, 1, 9, 130): "two x seams (63|64, 127|128) and a partial third tile of 2 columns; three y tiles, the last of 1 row; "
                    "fwd: 9 blocks per plane, 27 in all for the reduce",
    (2, 3, 37, 75): "the suite's ragged shape: 10 y tiles (the last of 1 row), 2 x tiles (the second of 11 columns), 6 planes",
    (1, 1, 3, 200): "minimum height across three x seams: y - 2 >= 0, y + 2 < H hold at one row each, y - 1 >= 0 && "
                    "y + 1 < H at the middle row only, in a partial (3 of 4 rows) y tile",
    (1, 1, 131, 3): "minimum width over 33 y tiles: x - 2 >= 0, x + 2 < W at one column each, every y guard at a y seam; "
                    "61 of a tile's 64 columns are idle",
}
FAMILIES = ("float", "int")
MULTI = ((5, 65), (3, 33))                      # the multi-scale call: accumulate = 1 on the second map, scale_factor 2
MULTI_B = 2


def make(shape, family, seed=0):
    """One fp32 CPU map of `shape` = (B, C, H, W)."""
    b, c, h, w = shape
    gen = torch.Generator().manual_seed(100000 * b + 10000 * c + 100 * h + w + 7 * seed + (1 if family == "int" else 0))
    if family == "float":
        return torch.rand(shape, generator=gen) * 10 + 0.5
    m = torch.randint(-3, 4, shape, generator=gen).float()
    level = torch.randint(-3, 4, (b, c, 1, 1), generator=gen).float()
    (x0, x1), (y0, y1) = flat_band(h, w)
    m[:, :, y0:y1, x0:x1] = level
    return m


def flat_band(h, w):
    """((x0, x1), (y0, y1)) of the integer family's flat band, a stand-in for a saturated disparity: nine columns over the
    full height that end at the image's edge (W = 64) or straddle the first x seam 63|64, or, where the image is too
    narrow, ten rows over the full width across the y seams at 60, 64 and 68.  Two samples inside the band every stencil
    reads the band only and the gradient is exactly 0.  No band in an image below 8 x 8."""
    if w >= 8:
        x0 = max(0, min(60, w - 8))
        return (x0, min(w, x0 + 9)), (0, h)
    if h >= 8:
        return (0, w), (min(59, h - 8), min(59, h - 8) + 10)
    return (0, 0), (0, 0)


def make_multi(family):
    return [make((MULTI_B, 1, h, w), family, seed=3) for h, w in MULTI]


def oracle(maps, scale_factor=1, dtype=torch.float64):
    """oracle.losses.smooth_loss and its gradients in `dtype`: (loss, [gradient per map])."""
    leaves = [m.detach().clone().to(dtype).requires_grad_(True) for m in maps]
    loss = ol.smooth_loss(leaves if len(leaves) > 1 else leaves[0], scale_factor)
    loss.backward()
    return loss.detach(), [x.grad for x in leaves]


def term_sums(m):
    """The four partial sums sum|dx2|, sum|dxdy|, sum|dydx|, sum|dy2| of one map, fp64."""
    return [float(t.abs().sum()) for t in ol._second_order_terms(m.double())]


def min_abs_term(m):
    """Smallest |second difference| of the map over the four terms, fp64."""
    return min(float(t.abs().min()) for t in ol._second_order_terms(m.double()))


def zero_terms(m):
    """Number of second differences that are exactly 0, per term."""
    return [int((t == 0).sum()) for t in ol._second_order_terms(m.double())]


def sign_sums(m):
    """The integer gradients of the three UNWEIGHTED sums (sum|dx2|, sum|dxdy| + sum|dydx|, sum|dy2|) per element: what
    smooth_bwd_kernel calls g1, g2, g3.  fp64, exact for any input whose signs are determinate."""
    out = []
    for pick in ((0,), (1, 2), (3,)):
        x = m.detach().double().clone().requires_grad_(True)
        terms = ol._second_order_terms(x)
        sum(terms[k].abs().sum() for k in pick).backward()
        out.append(x.grad)
    return out


def zero_is_structural(m):
    """(every exactly-zero element of the fp64 gradient has g1 = g2 = g3 = 0, the number of such elements)."""
    grad = oracle([m])[1][0]
    g1, g2, g3 = sign_sums(m)
    zero = grad == 0
    structural = (g1 == 0) & (g2 == 0) & (g3 == 0)
    return bool((structural | ~zero).all()), int(zero.sum())
