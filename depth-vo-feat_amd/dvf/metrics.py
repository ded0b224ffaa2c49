"""Depth validation metrics on the device (csrc/depth_metrics.hip, ``dvf_depth_metrics`` of include/dvf_hip.h).

``depth_metrics`` returns one row of twelve numbers per image, still on the device and without a synchronisation:
[abs_diff, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, n_valid, med_gt, med_pred, n_nan].  The definition is the
reference's ``compute_errors`` (loss_functions_sfm.py:80-116) with the rmse columns of the Eigen protocol added; the median
is torch.median's lower median, found exactly.  ``reduce_rows`` averages rows over the images that have a valid pixel."""
import torch

from depth_eval import garg_rect
from . import lib as L

COLUMNS = ("abs_diff", "abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "n_valid", "med_gt", "med_pred", "n_nan")
METRICS = COLUMNS[:8]


def depth_metrics(gt, pred, crop=True, min_depth=0.0, max_depth=80.0, clamp=(1e-3, 80.0), median_scaling=True, reclamp=False,
                  rect=None):
    """Rows [B,12] (``COLUMNS``) of ``pred`` against ``gt``, both [B,H,W] fp32 on the device.  valid = min_depth < gt <
    max_depth inside the Garg crop (``crop``) or inside ``rect`` = (y1, y2, x1, x2) when given; the prediction is clamped to
    ``clamp``, median-scaled (``median_scaling``) and optionally clamped again (``reclamp``, depth_eval.evaluate's order).
    No synchronisation; the result is ordered on the current stream."""
    L.dev(gt, "gt")
    L.dev(pred, "pred")
    if gt.dim() != 3 or gt.shape != pred.shape:
        raise ValueError(f"depth_metrics: gt and pred must be [B,H,W] of one size, got {tuple(gt.shape)} and {tuple(pred.shape)}")
    B, H, W = gt.shape
    y1, y2, x1, x2 = rect if rect is not None else (garg_rect(H, W) if crop else (0, H, 0, W))
    out = torch.empty(B, 12, device=gt.device, dtype=torch.float32)
    n = int(L.lib().dvf_depth_metrics_ws_floats(B, H, W))
    ws = L.workspace(("dvf_depth_metrics", B, H, W), n, torch.float32, gt.device)
    flags = (L.DM_MEDIAN_SCALE if median_scaling else 0) | (L.DM_RECLAMP if reclamp else 0)
    L.check(L.lib().dvf_depth_metrics(gt.data_ptr(), pred.data_ptr(), out.data_ptr(), ws.data_ptr(), n, B, H, W, y1, y2, x1, x2,
                                      float(min_depth), float(max_depth), float(clamp[0]), float(clamp[1]), flags, L.stream()),
            "dvf_depth_metrics")
    return out


def sum_rows(rows):
    """(sum of the first eight columns over the images with n_valid > 0 [8], the number of those images []), on the device."""
    keep = (rows[:, 8] > 0).to(rows.dtype)
    return (rows[:, :8] * keep[:, None]).sum(0), keep.sum()


def mean_rows(total, count):
    """sum_rows' two results, of one batch or added up over several, as the mean; zeros when no image has a valid pixel."""
    return total / count.clamp(min=1.0)


def reduce_rows(rows):
    """Mean of the first eight columns over the images with n_valid > 0 ([8], on the device, no synchronisation; zeros when
    no image has a valid pixel)."""
    return mean_rows(*sum_rows(rows))
