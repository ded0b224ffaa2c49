#!/usr/bin/env python3
"""MI355X drop-in for the reference's ``pytorch_version/train.py``: DispNetS + PoseExpNet(sfm) trained with the
4-scale photometric loss (explainability masks), explainability regulariser, smoothness and the stereo-pose MSE.

Same flags and defaults as the reference (train.py:31-67).  Differences, all forced by scope:
data is the seeded synthetic stream unless --data-root is given, multi-GPU is one process per GPU with RCCL all-reduce
instead of nn.DataParallel.  ``validate()`` (odometry L1 against the ground-truth relative poses of the test sequences,
train.py:220-247) runs after every epoch when --val-root points at a KITTI-odometry tree (sequences/<seq>/image_2,
poses/<seq>.txt) and then decides the best checkpoint like the reference; otherwise the best training loss does.
With --val-depth-root the depth network is validated against ground-truth depth after every epoch as well (Eigen metrics,
computed on the GPU) and best_depth_checkpoint.pth.tar follows the best abs_rel; --val-kitti-raw-root with --val-split does
the same against ground truth built on the GPU from the LiDAR sweeps of a KITTI raw tree.  With --val-odometry (and --val-root) the pose
network's outputs over each test sequence are chained into a trajectory after every epoch and scored with the KITTI odometry
errors, on the GPU as well; best_odometry_checkpoint.pth.tar follows the best t_err.  --val-odometry-align MODE first brings
every trajectory onto its ground truth (scale, 6dof, 7dof: a monocular network's scale is arbitrary), so that t_err is the
aligned one, and prints ATE, RPE and the 5-frame-snippet ATE in a Trajectory line.

    python train.py -b 4 --epochs 2                       # 1 GPU
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py -b 4
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from DispNetS import DispNetS  # noqa: E402
from PoseExpNet_sfm import PoseExpNet  # noqa: E402
from dvf import cli, validation  # noqa: E402
from dvf.odometry import ALIGN_MODES  # noqa: E402
from dvf.steps import train_sfm_losses  # noqa: E402

parser = argparse.ArgumentParser(description="Unsupervised depth + pose training (sfm loss form) on MI355X",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
parser.add_argument("--dataset-dir", default="/home/share/kitti_odometry/dataset/", type=str, help="accepted for compatibility; unused (synthetic data)")
parser.add_argument("--train-sequences", default=["01", "02", "03", "04", "05", "06", "07", "08", "09", "10"], type=str, nargs="*")
parser.add_argument("--test-sequences", default=["00"], type=str, nargs="*")
parser.add_argument("--rotation-mode", type=str, choices=["euler", "quat"], default="euler")
parser.add_argument("--padding-mode", type=str, choices=["zeros", "border"], default="zeros")
parser.add_argument("-j", "--workers", default=4, type=int, metavar="N")
parser.add_argument("--epochs", default=200, type=int, metavar="N")
parser.add_argument("--epoch-size", default=0, type=int, metavar="N", help="iterations per epoch (0: --steps-per-epoch)")
parser.add_argument("-b", "--batch-size", default=4, type=int, metavar="N", help="mini-batch size PER GPU")
parser.add_argument("--lr", "--learning-rate", default=2e-4, type=float, metavar="LR")
parser.add_argument("--momentum", default=0.9, type=float, metavar="M", help="alpha parameter for adam")
parser.add_argument("--beta", default=0.999, type=float, metavar="M", help="beta parameter for adam")
parser.add_argument("--weight-decay", "--wd", default=0, type=float, metavar="W")
parser.add_argument("--pretrained-disp", dest="pretrained_disp", default=None, metavar="PATH")
parser.add_argument("--pretrained-exppose", dest="pretrained_exp_pose", default=None, metavar="PATH")
parser.add_argument("--seed", default=0, type=int)
parser.add_argument("-p", "--photo-loss-weight", type=float, metavar="W", default=1)
parser.add_argument("-m", "--mask-loss-weight", type=float, metavar="W", default=0)
parser.add_argument("-s", "--smooth-loss-weight", type=float, metavar="W", default=0.1)
parser.add_argument("--smooth-loss-factor", type=float, metavar="W", default=2)
parser.add_argument("-g", "--gpu-id", type=int, metavar="N", default=-1, help="accepted for compatibility; ranks pick LOCAL_RANK")
parser.add_argument("--output-dir", type=str, default="./checkpoints")
parser.add_argument("--nb-ref-imgs", type=int, default=2, help="reference views (2 = temporal + stereo; 4 = 5-frame window)")
parser.add_argument("--val-root", default=None, help="KITTI odometry tree for validate() on --test-sequences (train.py:220-247)")
parser.add_argument("--val-depth-root", default=None, metavar="DIR",
                    help="depth validation tree (val.txt, image/<stem>.png|jpg, depth/<stem>.npy in metres, 0 = no measurement): "
                         "after every epoch rank 0 prints the Eigen depth metrics of the depth network against it "
                         "(dvf.validation.validate_depth) and best_depth_checkpoint.pth.tar is saved on the best abs_rel")
parser.add_argument("--val-kitti-raw-root", default=None, metavar="DIR",
                    help="in place of --val-depth-root: a KITTI raw tree; the ground truth of the frames of --val-split is built "
                         "from their LiDAR sweeps on the GPU (dvf.velodyne.depth_maps), same Depth line and checkpoint rule")
parser.add_argument("--val-split", default=None, metavar="FILE",
                    help="needs --val-kitti-raw-root: one <date>/<drive>/image_0<cam>/data/<id>.png per line (an Eigen split list)")
parser.add_argument("--val-cam", type=int, choices=[2, 3], default=2, help="with --val-kitti-raw-root: the colour camera")
parser.add_argument("--val-odometry", action="store_true",
                    help="needs --val-root: after every epoch rank 0 also chains the pose network's output over each of "
                         "--test-sequences into a trajectory and prints its KITTI odometry errors (t_err in %%, r_err in deg / 100 m, "
                         "computed on the GPU: dvf.validation.validate_odometry); best_odometry_checkpoint.pth.tar is saved on the best t_err")
parser.add_argument("--pose-convention", choices=list(validation.POSE_CONVENTIONS), default="se3",
                    help="how --val-odometry reads the pose network's six outputs: se3 = (w, u) through the exponential map, what "
                         "validate() scores; euler = (t, r-euler), what the photometric loss of this script trains them as")
parser.add_argument("--val-odometry-align", choices=list(ALIGN_MODES), default=None, metavar="MODE",
                    help="needs --val-odometry: every chained trajectory is first brought onto its ground truth by one of " +
                         ", ".join(ALIGN_MODES) + " (a monocular network's scale is arbitrary: scale or 7dof removes it); "
                         "best_odometry_checkpoint.pth.tar then follows the aligned t_err, and a Trajectory line (ATE, RPE, "
                         "5-frame-snippet ATE) is printed after the Odometry line")
cli.add_common_flags(parser)


def main():
    args = parser.parse_args()
    if args.val_odometry and not args.val_root:
        parser.error("--val-odometry needs --val-root")
    if args.val_odometry_align is not None and not args.val_odometry:
        parser.error("--val-odometry-align needs --val-odometry")
    if args.val_kitti_raw_root and args.val_depth_root:
        parser.error("--val-kitti-raw-root and --val-depth-root exclude each other")
    if bool(args.val_kitti_raw_root) != bool(args.val_split):
        parser.error("--val-kitti-raw-root and --val-split go together")
    args._rank, args._world, args._device = cli.init_distributed()
    if args.epoch_size:
        args.steps_per_epoch = args.epoch_size
    torch.manual_seed(args.seed)
    disp_net = DispNetS()
    pose_exp_net = PoseExpNet(nb_ref_imgs=args.nb_ref_imgs, output_exp=True)      # train.py:126-127
    if args.pretrained_exp_pose:
        cli.load_pretrained(pose_exp_net, args.pretrained_exp_pose, strict=False)
    else:
        pose_exp_net.init_weights()
    if args.pretrained_disp:
        cli.load_pretrained(disp_net, args.pretrained_disp)
    else:
        disp_net.init_weights()
    disp_net.to(args._device).train()
    pose_exp_net.to(args._device).train()

    def loss_fn(batch):
        return train_sfm_losses(disp_net, pose_exp_net, batch, args.photo_loss_weight, args.mask_loss_weight,
                                args.smooth_loss_weight, args.smooth_loss_factor, args.rotation_mode, args.padding_mode,
                                **cli.ssim_kwargs(args), **cli.minreproj_kwargs(args), **cli.fullres_kwargs(args),
                                **cli.normsmooth_kwargs(args))

    terms = ["total", "photo", "smooth", "lr"] + (["exp"] if args.mask_loss_weight > 0 else []) + \
        (["automask"] if args.auto_mask else [])
    validators = []
    if args.val_root and args._rank == 0:
        from dataset import pose_framework_KITTI
        val_set = pose_framework_KITTI(args.val_root, args.test_sequences, img_height=args.height, img_width=args.width,
                                       shuffle=False)
        val_loader = torch.utils.data.DataLoader(val_set, batch_size=args.batch_size, shuffle=False, num_workers=0)
        # (ckpts=None: the reference's criterion for best_vo / best_depth, in place of the training loss)
        validators.append(cli.Validator(lambda _: validation.validate(pose_exp_net, val_loader, args._device), float,
                                        validation.pose_epoch_lines, None))
    if (args.val_depth_root or args.val_kitti_raw_root) and args._rank == 0:
        from dataset import depth_validation_set, kitti_raw_depth_set
        depth_set = (depth_validation_set(args.val_depth_root, args.height, args.width) if args.val_depth_root else
                     kitti_raw_depth_set(args.val_kitti_raw_root, args.val_split, args.height, args.width, cam=args.val_cam))
        depth_loader = depth_set.loader(args.batch_size)
        validators.append(cli.Validator(lambda _: validation.validate_depth(disp_net, depth_loader, args._device),
                                        lambda m: m["abs_rel"], validation.depth_epoch_lines,
                                        [("best_depth_checkpoint.pth.tar", disp_net)]))
    if args.val_odometry and args._rank == 0:
        from dataset import odometry_sequences
        sequences = odometry_sequences(args.val_root, args.test_sequences, args.height, args.width)
        validators.append(cli.Validator(lambda _: validation.validate_odometry(pose_exp_net, sequences, args._device, args.batch_size,
                                                                               convention=args.pose_convention,
                                                                               align=args.val_odometry_align),
                                        lambda m: m["t_err"], validation.odometry_epoch_lines,
                                        [("best_odometry_checkpoint.pth.tar", pose_exp_net)]))
    cli.run_training(args, [disp_net, pose_exp_net], loss_fn, args.lr, (args.momentum, args.beta), args.weight_decay,
                     terms, [("best_vo_checkpoint.pth.tar", pose_exp_net), ("best_depth_checkpoint.pth.tar", disp_net)],
                     n_views=max(2, args.nb_ref_imgs), validators=validators)


if __name__ == "__main__":
    main()
