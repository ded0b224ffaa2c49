"""Cases for dvf_resize_bilinear_fwd at general scales and for dvf.validation.validate_depth against its definition
(tests/test_resize_cases.py, tests/test_gpu_resize_validation.py).

The kernel's contract is aten's upsample_bilinear2d with align_corners = False and scale = in / out per axis:
src = max(scale * (dst + 0.5) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1), weight src - i0.  For an affine field
that is the field itself at the source coordinate clamped to [0, in - 1], which pins the half-pixel offset, the per-axis
scales and the clamp without depending on noise (affine_expected()).

validate_depth's definition, restated from torch alone (expected_metrics()): the network's first output in fp64 ->
F.interpolate(bilinear, align_corners = False) to the ground truth's size -> 1 / x -> depth_metrics_ref.rows -> the mean over
the images that have a valid pixel.  The network here is a stub of torch ops (StubDisp), so the definition needs no kernel."""
import types

import torch
import torch.nn.functional as F

import depth_metrics_ref as R

# (planes, (H, W), (OH, OW)) of the noise cases
SHAPES = [
    (2, (16, 52), (37, 122)),           # the CLI test's tree: up, non-dyadic, different per axis
    (2, (16, 52), (40, 130)),
    (2, (48, 160), (37, 122)),          # down on both axes
    (2, (7, 5), (3, 9)),                # down in y, up in x
    (2, (1, 1), (4, 6)),                # one-pixel source: both taps clamped on both axes
    (2, (2, 3), (2, 3)),                # identity
    (3, (128, 416), (375, 1242)),       # the product's ratio; 1.4 M outputs: a second grid-stride trip of 4096 x 256 threads
]
AFFINE = (0.5, 0.25, 3.0)               # a, b, c of a * x + b * y + c: dyadic, exact in fp32 at every pixel
AFFINE_SHAPES = [((16, 52), (37, 122)), ((48, 160), (37, 122)), ((7, 5), (3, 9)), ((5, 7), (9, 3)), ((2, 3), (2, 3))]


def noise(planes, h, w, seed=0):
    gen = torch.Generator().manual_seed(1000 * h + w + seed)
    return torch.rand(planes, h, w, generator=gen) * 10 + 0.01


def interpolate(x, size):
    """F.interpolate of [planes, H, W] in x's own precision."""
    return F.interpolate(x[None], size, mode="bilinear", align_corners=False)[0]


def affine(h, w):
    a, b, c = AFFINE
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return (a * xx + b * yy + c)[None].contiguous()


def src_coords(n_in, n_out):
    """fp64 source coordinate of every destination sample, unclamped: (in / out) * (dst + 0.5) - 0.5."""
    return (n_in / n_out) * (torch.arange(n_out, dtype=torch.float64) + 0.5) - 0.5


def affine_expected(src, dst):
    """([1, OH, OW] fp64 expected resize of affine(*src), interior mask [OH, OW], the field's range)."""
    a, b, c = AFFINE
    sy, sx = src_coords(src[0], dst[0]), src_coords(src[1], dst[1])
    inside = ((sy >= 0) & (sy <= src[0] - 1))[:, None] & ((sx >= 0) & (sx <= src[1] - 1))[None, :]
    want = a * sx.clamp(0, src[1] - 1)[None, :] + b * sy.clamp(0, src[0] - 1)[:, None] + c
    return want[None], inside, a * (src[1] - 1) + b * (src[0] - 1)


# ------------------------------------------------------------------------------------------------ validate_depth
IMG = (64, 208)
GT_SIZES = ((37, 122), (40, 130))
BATCH = 2
EMPTY = (1, 0)                          # (batch, image) whose ground truth has no valid pixel
SEED = 5


class StubDisp(torch.nn.Module):
    """[B,3,h,w] -> [ [B,1,h/4,w/4] ]: a smooth positive disparity in (0.01, 10.01), from torch ops only."""

    def forward(self, img):
        pooled = F.avg_pool2d(img.mean(1, keepdim=True), 4)
        return [10 * torch.sigmoid(8 * (pooled - 0.5)) + 0.01, pooled]


def upsampled_depth(disp, size):
    """The definition's middle: fp64 bilinear resize of the disparity [B,1,h,w] to `size`, inverted; [B,Hg,Wg] fp64."""
    return 1.0 / F.interpolate(disp.detach().double().cpu(), size, mode="bilinear", align_corners=False)[:, 0]


def make_validation(seed=SEED):
    """loader: a list of (img [B,3,h,w], gt [B,Hg,Wg]) fp32 CPU batches, one per ground-truth size.  The ground truth is
    150 x the stub's own depth with 20 % noise (so that median scaling and the thresholds have work to do), half of the
    pixels dropped to 0 = no measurement, a few beyond the 80 m cap, and one image all zeros."""
    gen = torch.Generator().manual_seed(seed)
    stub = StubDisp()
    loader = []
    for k, size in enumerate(GT_SIZES):
        img = F.interpolate(torch.rand(BATCH, 3, IMG[0] // 8, IMG[1] // 8, generator=gen), IMG, mode="bilinear",
                            align_corners=False)
        depth = upsampled_depth(stub(img)[0], size)
        gt = 150.0 * depth * (1 + 0.2 * torch.randn(depth.shape, generator=gen, dtype=torch.float64))
        gt = torch.where(torch.rand(depth.shape, generator=gen) < 0.5, torch.zeros_like(gt), gt.clamp(min=0.0))
        gt = gt.float()
        if k == EMPTY[0]:
            gt[EMPTY[1]] = 0.0
        loader.append((img.contiguous(), gt.contiguous()))
    return types.SimpleNamespace(loader=loader, stub=stub)


def expected_metrics(disps, loader, crop=True, median_scaling=True):
    """(mean of the eight metrics over the images with a valid pixel [8] fp64, rows per batch, near per batch) from the
    stub's outputs `disps` (one [B,1,h,w] tensor per batch, any device)."""
    total, count, all_rows, all_near = torch.zeros(8, dtype=torch.float64), 0, [], []
    for disp, (_, gt) in zip(disps, loader):
        depth = upsampled_depth(disp, tuple(gt.shape[1:]))
        rows, near = R.rows(gt, depth.float(), crop=crop, median_scaling=median_scaling)
        keep = rows[:, 8] > 0
        total += rows[keep, :8].sum(0)
        count += int(keep.sum())
        all_rows.append(rows)
        all_near.append(near)
    return total / max(count, 1), all_rows, all_near
