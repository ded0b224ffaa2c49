"""Depth evaluation metrics of the reference's tools (host side, numpy; not on the training hot path).

``compute_errors`` follows ``tools/eval_depth_utils.py:10-28`` (after Godard's monodepth evaluation): for ground-truth
and predicted depths of the valid pixels it returns (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3).  The reference module
imports cv2 (absent in the build image), so it cannot be imported for vectors: parity is pinned by hand-computed known
answers in tests/test_depth_eval.py.  ``evaluate`` applies the usual KITTI protocol of tools/eval_depth.py around it:
depth cap, optional Garg crop, optional median scaling.

Run as a script (``python depth_eval.py --pretrained-disp CKPT --val-depth-root DIR``) it evaluates a checkpoint on the GPU
through dvf.validation.validate_depth / dvf.metrics.depth_metrics instead.  The two differ in one documented place: ``evaluate``
uses numpy's median, the MEAN OF THE TWO middle elements for an even count, while the device path takes torch.median's lower
median as the reference's training-side compute_errors does (loss_functions_sfm.py:104); the mean-of-two form is not
reproduced on the device.  The device path also clamps once, before scaling, unless asked to reclamp."""
import numpy as np


def compute_errors(gt, pred):
    gt, pred = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    thresh = np.maximum(gt / pred, pred / gt)
    a1, a2, a3 = ((thresh < 1.25 ** e).mean() for e in (1, 2, 3))
    rmse = np.sqrt(((gt - pred) ** 2).mean())
    rmse_log = np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean())
    abs_rel = np.mean(np.abs(gt - pred) / gt)
    sq_rel = np.mean(((gt - pred) ** 2) / gt)
    return abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3


def garg_rect(h, w):
    """(y1, y2, x1, x2) of the crop of Garg et al. (ECCV16) used to reproduce Eigen's results: the int(...) constants of
    loss_functions_sfm.py:92-93.  dvf.metrics.depth_metrics takes its default rectangle from here."""
    return int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w)


def garg_crop_mask(h, w):
    """garg_rect as a boolean [h, w] mask."""
    y1, y2, x1, x2 = garg_rect(h, w)
    m = np.zeros((h, w), dtype=bool)
    m[y1:y2, x1:x2] = True
    return m


def evaluate(gt_depths, pred_depths, min_depth=1e-3, max_depth=80.0, garg_crop=True, median_scaling=True):
    """Mean of compute_errors over a list of (gt, pred) depth maps of equal size per pair."""
    rows = []
    for gt, pred in zip(gt_depths, pred_depths):
        gt, pred = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
        mask = (gt > min_depth) & (gt < max_depth)
        if garg_crop:
            mask &= garg_crop_mask(*gt.shape)
        g, p = gt[mask], np.clip(pred[mask], min_depth, max_depth)
        if median_scaling:
            p = p * (np.median(g) / np.median(p))
            p = np.clip(p, min_depth, max_depth)
        rows.append(compute_errors(g, p))
    return tuple(np.mean(np.array(rows), axis=0))


def main(argv=None):
    """Evaluate a depth checkpoint against a depth validation tree on the GPU and print the seven Eigen metrics plus
    abs_diff (the line train.py --val-depth-root prints after every epoch)."""
    import argparse
    import torch
    from DispNetS import DispNetS
    from dataset import depth_validation_set
    from dvf import cli, validation
    parser = argparse.ArgumentParser(description="Depth evaluation against ground truth on MI355X",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--pretrained-disp", required=True, metavar="PATH", help="DispNetS checkpoint (best_depth_checkpoint.pth.tar)")
    parser.add_argument("--val-depth-root", required=True, metavar="DIR",
                        help="val.txt, image/<stem>.png|jpg, depth/<stem>.npy in metres (0 = no measurement)")
    parser.add_argument("--height", type=int, default=256)
    parser.add_argument("--width", type=int, default=832)
    parser.add_argument("-b", "--batch-size", type=int, default=4)
    parser.add_argument("--no-crop", action="store_true", help="all pixels instead of the Garg crop")
    parser.add_argument("--no-median-scaling", action="store_true", help="compare the prediction as it is")
    args = parser.parse_args(argv)
    cli.require_gpu()
    device = torch.device("cuda", 0)
    net = DispNetS()
    cli.load_pretrained(net, args.pretrained_disp)
    net.to(device)
    loader = depth_validation_set(args.val_depth_root, args.height, args.width).loader(args.batch_size)
    metrics = validation.validate_depth(net, loader, device, crop=not args.no_crop, median_scaling=not args.no_median_scaling)
    print(validation.format_depth_metrics(metrics), flush=True)
    return metrics


if __name__ == "__main__":
    main()
