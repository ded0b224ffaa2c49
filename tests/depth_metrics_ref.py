"""Test-side definition of the depth validation metrics (dvf_depth_metrics of include/dvf_hip.h).

The front end is fp32 exactly as the reference's compute_errors (loss_functions_sfm.py:80-116) does it -- mask, clamp,
torch.median (the lower median), the fp32 scale med(gt) / med(pred) and the fp32 product -- and every sum is fp64.  Besides the
twelve columns of a row it returns, per threshold 1.25^e, the number of valid pixels whose fp64 ratio max(g/p, p/g) lies within
NEAR = 1e-6 (relative) of the threshold: an fp32 implementation forms the ratio with two correctly rounded operations, which
puts it within 2.5e-7 of the fp64 value, so only those pixels (a four-fold margin) may fall on the other side."""
import torch

NEAR = 1e-6
COLUMNS = ("abs_diff", "abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "n_valid", "med_gt", "med_pred", "n_nan")


def garg_rect(h, w):
    return int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w)


def gen_case(b, h, w, seed=None, dropout=0.5, quantum=None):
    """The generator of tests/golden/gen_golden.py::gen_metrics at another size, dropout and seed (default 1000*h + w):
    sparse ground truth in [0, 95) m with 0 = no measurement, a noisy, differently scaled prediction, and the first rows of
    image 0 negative so that the clamp works: four rows as there, but at most a quarter of the image -- with half of an
    8-row image clamped to 1e-3 the median prediction is the clamp value itself, every clamped pixel scales to exactly
    med(gt), and a quantised gt of 1.25 * med(gt) then sits exactly ON a threshold.  ``quantum``: the ground truth rounded to
    multiples of it (heavy duplicates, as KITTI's 1/256 m steps give); the prediction stays continuous."""
    g = torch.Generator().manual_seed(1000 * h + w if seed is None else seed)
    gt = torch.rand(b, h, w, generator=g, dtype=torch.float64) * 95.0
    gt = torch.where(torch.rand(b, h, w, generator=g, dtype=torch.float64) < dropout, torch.zeros_like(gt), gt).float()
    pred = (gt.double() * 0.37 * (1 + 0.25 * torch.randn(b, h, w, generator=g, dtype=torch.float64)) +
            torch.rand(b, h, w, generator=g, dtype=torch.float64) * 0.5).float()
    pred[0, :min(4, h // 4)] = -1.0
    if quantum:
        gt = (torch.round(gt / quantum) * quantum).float()
    return gt, pred


def rows(gt, pred, crop=True, rect=None, min_depth=0.0, max_depth=80.0, clamp=(1e-3, 80.0), median_scaling=True, reclamp=False):
    """(rows [B,12] float64, near [B,3] int64) of fp32 CPU tensors gt, pred [B,H,W]."""
    gt, pred = gt.detach().cpu().float(), pred.detach().cpu().float()
    b, h, w = gt.shape
    y1, y2, x1, x2 = rect if rect is not None else (garg_rect(h, w) if crop else (0, h, 0, w))
    region = torch.zeros(h, w, dtype=torch.bool)
    region[y1:y2, x1:x2] = True
    lo, hi = torch.tensor(min_depth, dtype=torch.float32), torch.tensor(max_depth, dtype=torch.float32)
    c_lo, c_hi = float(torch.tensor(clamp[0], dtype=torch.float32)), float(torch.tensor(clamp[1], dtype=torch.float32))
    out = torch.zeros(b, 12, dtype=torch.float64)
    near = torch.zeros(b, 3, dtype=torch.int64)
    for i in range(b):
        keep = (gt[i] > lo) & (gt[i] < hi) & region
        n = int(keep.sum())
        if n == 0:
            continue
        g, p = gt[i][keep], pred[i][keep].clamp(c_lo, c_hi)
        n_nan = int(torch.isnan(p).sum())
        med_g, med_p = g.median(), p.median()            # fp32; a NaN anywhere makes the median NaN
        if median_scaling:
            p = p * (med_g / med_p)                      # fp32 quotient, fp32 product
        if reclamp:
            p = p.clamp(c_lo, c_hi)
        out[i, 8], out[i, 9], out[i, 10], out[i, 11] = n, float(med_g), float(med_p), n_nan
        if n_nan:
            out[i, :8] = float("nan")
            continue
        gd, pd = g.double(), p.double()
        d = gd - pd
        ratio = torch.maximum(gd / pd, pd / gd)
        out[i, 0] = d.abs().mean()
        out[i, 1] = (d.abs() / gd).mean()
        out[i, 2] = (d * d / gd).mean()
        out[i, 3] = (d * d).mean().sqrt()
        out[i, 4] = ((gd.log() - pd.log()) ** 2).mean().sqrt()
        for e in (1, 2, 3):
            out[i, 4 + e] = (ratio < 1.25 ** e).double().mean()
            near[i, e - 1] = int(((ratio / 1.25 ** e - 1).abs() <= NEAR).sum())
    return out, near


def reference_six(out):
    """The reference's six batch means [abs_diff, abs_rel, sq_rel, a1, a2, a3] from rows."""
    return (out[:, [0, 1, 2, 5, 6, 7]].sum(0) / out.shape[0]).tolist()


SMALL_SHAPES = [(1, 2, 2), (2, 5, 7), (2, 8, 63), (2, 8, 64), (3, 9, 65), (2, 17, 257)]
SMALL_CASES = [(s, crop, q) for s in SMALL_SHAPES for crop in (True, False) for q in (None, 0.25)]
