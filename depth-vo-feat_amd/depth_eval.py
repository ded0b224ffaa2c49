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
reproduced on the device.  The device path also clamps once, before scaling, unless asked to reclamp.

With ``--kitti-raw-root DIR --split FILE`` instead of ``--val-depth-root`` the ground truth is built on the GPU from the LiDAR
sweeps of a KITTI raw tree (dvf.velodyne.depth_maps: the reference's generate_depth_map, tools/eval_depth_utils.py:172-224,
whose module is Python 2 and imports cv2 as well), and ``--export-depth-root OUT`` writes it as a tree --val-depth-root reads."""
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
    """Evaluate a depth checkpoint against a depth validation tree, or against the LiDAR sweeps of a KITTI raw tree, on the GPU
    and print the seven Eigen metrics plus abs_diff (the line train.py --val-depth-root prints after every epoch)."""
    import argparse
    import torch
    from DispNetS import DispNetS
    from dataset import depth_validation_set, kitti_raw_depth_set
    from dvf import cli, validation
    parser = argparse.ArgumentParser(description="Depth evaluation against ground truth on MI355X",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--pretrained-disp", required=True, metavar="PATH", help="DispNetS checkpoint (best_depth_checkpoint.pth.tar)")
    parser.add_argument("--val-depth-root", default=None, metavar="DIR",
                        help="val.txt, image/<stem>.png|jpg, depth/<stem>.npy in metres (0 = no measurement); "
                             "this or --kitti-raw-root is required")
    parser.add_argument("--kitti-raw-root", default=None, metavar="DIR",
                        help="KITTI raw tree (<date>/<drive>/image_0<cam>/data, velodyne_points/data, the calibration files in "
                             "<date>/ or <date>/<drive>/calib/): the ground truth is built from the LiDAR sweeps on the GPU; needs --split")
    parser.add_argument("--split", default=None, metavar="FILE",
                        help="with --kitti-raw-root: the frames to evaluate, one <date>/<drive>/image_0<cam>/data/<id>.png per line "
                             "(an Eigen split list; later fields of a line are ignored)")
    parser.add_argument("--cam", type=int, choices=[2, 3], default=2, help="with --kitti-raw-root: the colour camera, 2 = left, 3 = right")
    parser.add_argument("--velodyne-depth", action="store_true",
                        help="with --kitti-raw-root: the ground truth is the LiDAR's forward distance instead of the camera depth")
    parser.add_argument("--export-depth-root", default=None, metavar="OUT",
                        help="with --kitti-raw-root: also write the ground truth as a tree that --val-depth-root reads "
                             "(val.txt, image/<stem>.png copied, depth/<stem>.npy)")
    parser.add_argument("--height", type=int, default=256)
    parser.add_argument("--width", type=int, default=832)
    parser.add_argument("-b", "--batch-size", type=int, default=4)
    parser.add_argument("--no-crop", action="store_true", help="all pixels instead of the Garg crop")
    parser.add_argument("--no-median-scaling", action="store_true", help="compare the prediction as it is")
    args = parser.parse_args(argv)
    if (args.val_depth_root is None) == (args.kitti_raw_root is None):
        parser.error("exactly one of --val-depth-root and --kitti-raw-root is required")
    if args.kitti_raw_root is not None and args.split is None:
        parser.error("--kitti-raw-root needs --split")
    if args.kitti_raw_root is None and (args.split is not None or args.velodyne_depth or args.export_depth_root is not None):
        parser.error("--split, --velodyne-depth and --export-depth-root need --kitti-raw-root")
    cli.require_gpu()
    device = torch.device("cuda", 0)
    net = DispNetS()
    cli.load_pretrained(net, args.pretrained_disp)
    net.to(device)
    if args.kitti_raw_root is not None:
        loader = kitti_raw_depth_set(args.kitti_raw_root, args.split, args.height, args.width, cam=args.cam).loader(args.batch_size)
        if args.export_depth_root is not None:
            validation.export_depth_tree(loader, args.export_depth_root, device, velodyne_depth=args.velodyne_depth)
    else:
        loader = depth_validation_set(args.val_depth_root, args.height, args.width).loader(args.batch_size)
    metrics = validation.validate_depth(net, loader, device, crop=not args.no_crop, median_scaling=not args.no_median_scaling,
                                        velodyne_depth=args.velodyne_depth)
    print(validation.format_depth_metrics(metrics), flush=True)
    return metrics


if __name__ == "__main__":
    main()
