"""Pose-trajectory output and KITTI odometry evaluation: the host-side utilities either side of the
training hot path, rewritten with vectorised numpy.

  save_result_poses / se3_cam2world / compute_pose_error   reference pytorch_version/inference.py:43-88
  load_poses / trajectory_distances / sequence_errors / overall_error   reference tools/evaluation_tools.py:384-508
                                                             (class kittiEvalOdom, the KITTI devkit metric)
  trajectory_alignment / apply_alignment / trajectory_errors / snippet_errors   alignment of a predicted trajectory to ground
                                                             truth (scale, 6-DoF, 7-DoF Umeyama), ATE, RPE and compute_pose_error
                                                             over scale-aligned snippets (the factor inference.py:75 comments out)
The reference tool cannot be imported here (caffe, h5py, cv2), so these follow its published algorithm and are
checked by known-answer tests (tests/test_odometry_eval.py): parity unpinned against the reference itself.

Run as a script (``python odometry_eval.py --pretrained-pose CKPT --val-root DIR --sequences 09 10``) it evaluates a pose
checkpoint on the GPU through dvf.validation.validate_odometry / dvf.odometry (csrc/odometry.hip), for which se3_cam2world,
sequence_errors and overall_error below, and with ``--align MODE`` the four alignment functions, are the definition; importing
this module needs numpy only."""
import os

import numpy as np

SEGMENT_LENGTHS = (100, 200, 300, 400, 500, 600, 700, 800)     # metres (evaluation_tools.py:391)
FIRST_FRAME, FRAME_STEP, FRAME_PERIOD = 9, 10, 0.1             # :456,:458 and the 10 Hz speed constant of :482


def pose_line(se3):
    """One pose ([3,4] or [4,4]) as a KITTI line: the 3x4 [R|t] in row-major order, 12 numbers (inference.py:43-61)."""
    return " ".join(str(v) for v in np.asarray(se3, dtype=np.float64)[:3, :4].reshape(12)) + "\n"


def save_result_poses(se3, output_dir, filename):
    """Append one pose as a KITTI line (pose_line)."""
    with open(os.path.join(output_dir, filename), "a") as f:
        f.write(pose_line(se3))


def se3_cam2world(rel_poses):
    """Chain frame-to-frame [4,4] poses into camera-to-world poses, identity first (inference.py:63-70)."""
    out = [np.eye(4)]
    for p in rel_poses:
        out.append(out[-1] @ np.asarray(p, dtype=np.float64))
    return out


def compute_pose_error(gt, pred):
    """ATE and mean rotation error of a snippet of [N,3,4] poses (inference.py:72-88)."""
    gt, pred = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    n = gt.shape[0]
    ate = np.linalg.norm((gt[:, :, -1] - pred[:, :, -1]).reshape(-1))
    R = gt[:, :, :3] @ np.linalg.inv(pred[:, :, :3])
    s = np.sqrt((R[:, 0, 1] - R[:, 1, 0]) ** 2 + (R[:, 1, 2] - R[:, 2, 1]) ** 2 + (R[:, 0, 2] - R[:, 2, 0]) ** 2)
    c = np.trace(R, axis1=1, axis2=2) - 1.0
    return ate / n, float(np.arctan2(s, c).sum()) / n


ALIGN_MODES = ("none", "scale", "scale_7dof", "6dof", "7dof")


def _as44(traj):
    """[n,4,4] float64 copy of [n,3,4] or [n,4,4] poses, the last row 0 0 0 1."""
    a = np.asarray(traj, dtype=np.float64)
    out = np.tile(np.eye(4), (a.shape[0], 1, 1))
    out[:, :3, :4] = a[:, :3, :4]
    return out


def trajectory_alignment(gt, res, mode):
    """The transform (c, R, t, sv) that brings the trajectory ``res`` onto ``gt`` (both [n,3,4] or [n,4,4], dense: frame i is
    row i of both), fitted on the translation columns x_i of res and y_i of gt alone.  Nothing is re-based: KITTI ground truth
    and se3_cam2world both start at the identity; other inputs must be re-based by the caller.

      none        c = 1, R = I, t = 0
      scale       c = sum y.x / sum x.x about the origin (the factor inference.py:75 comments out), 1 when the denominator is 0
      7dof        Umeyama: Sigma = 1/n sum (y - my)(x - mx)^T = U D V^T, S = diag(1, 1, sign(det U det V)), R = U S V^T (a proper
                  rotation, never a reflection), c = tr(D S) / var_x (1 when var_x is 0), t = my - c R mx
      6dof        the same with c = 1
      scale_7dof  c of 7dof, R = I, t = 0

    sv holds the singular values of Sigma (zeros for none / scale): a straight line has sv[1] = sv[2] = 0 and no unique
    rotation.  The centred sums are a second pass over the data after the means, so a large common offset costs nothing."""
    if mode not in ALIGN_MODES:
        raise ValueError(f"mode must be one of {ALIGN_MODES}, got {mode!r}")
    x = np.asarray(res, dtype=np.float64)[:, :3, 3]
    y = np.asarray(gt, dtype=np.float64)[:, :3, 3]
    if x.shape != y.shape or x.shape[0] < 1:
        raise ValueError(f"gt and res must hold the same n >= 1 poses, got {y.shape[0]} and {x.shape[0]}")
    c, R, t, sv = 1.0, np.eye(3), np.zeros(3), np.zeros(3)
    if mode == "none":
        return c, R, t, sv
    if mode == "scale":
        den = float((x * x).sum())
        return (float((y * x).sum()) / den if den != 0.0 else 1.0), R, t, sv
    n = x.shape[0]
    if n < 3:
        raise ValueError(f"mode {mode!r} needs n >= 3 poses, got {n}")
    mx, my = x.mean(0), y.mean(0)
    xc, yc = x - mx, y - my
    var = float((xc * xc).sum()) / n
    U, sv, Vt = np.linalg.svd(yc.T @ xc / n)
    S = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    rot = U @ S @ Vt
    c7 = float(np.trace(np.diag(sv) @ S)) / var if var != 0.0 else 1.0
    if mode == "scale_7dof":
        return c7, R, t, sv
    c = c7 if mode == "7dof" else 1.0
    return c, rot, my - c * rot @ mx, sv


def apply_alignment(res, c, R, t):
    """Every pose [R_i | t_i] of ``res`` mapped to [R R_i | c R t_i + t]; the result has the shape of ``res``."""
    out = np.array(res, dtype=np.float64)
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    out[:, :3, :3] = R @ out[:, :3, :3]
    out[:, :3, 3] = c * (out[:, :3, 3] @ R.T) + t
    return out


def _angles(R):
    """atan2(|skew part|, trace - 1) of [m,3,3]: the angle form of compute_pose_error, exact down to zero (arccos of the
    trace loses eight digits at 1e-4 rad)."""
    s = np.sqrt((R[:, 0, 1] - R[:, 1, 0]) ** 2 + (R[:, 1, 2] - R[:, 2, 1]) ** 2 + (R[:, 0, 2] - R[:, 2, 0]) ** 2)
    return np.arctan2(s, np.trace(R, axis1=1, axis2=2) - 1.0)


def trajectory_errors(gt, res):
    """(ate, rpe_trans, rpe_rot) of dense trajectories, as they come (align first): ate = sqrt(mean |y_i - x_i|^2) over the
    translations; for every consecutive pair E = inv(inv(gt_i) gt_{i+1}) (inv(res_i) res_{i+1}) with the affine inverse,
    rpe_trans the mean of |E_t| and rpe_rot the mean of the atan2 angle of E_R (radians).  Both RPE values are NaN for n < 2."""
    g, r = _as44(gt), _as44(res)
    if g.shape != r.shape or g.shape[0] < 1:
        raise ValueError(f"gt and res must hold the same n >= 1 poses, got {g.shape[0]} and {r.shape[0]}")
    ate = float(np.sqrt(((g[:, :3, 3] - r[:, :3, 3]) ** 2).sum(1).mean()))
    if g.shape[0] < 2:
        return ate, float("nan"), float("nan")
    d_gt = np.linalg.inv(g[:-1]) @ g[1:]
    d_res = np.linalg.inv(r[:-1]) @ r[1:]
    E = np.linalg.inv(d_gt) @ d_res
    return ate, float(np.linalg.norm(E[:, :3, 3], axis=1).mean()), float(_angles(E[:, :3, :3]).mean())


def snippet_errors(gt, res, length=5):
    """[n - length + 1, 2] rows [ate, re] of every ``length``-frame snippet (start frames 0 .. n - length): both snippets are
    re-based to their first frame, the predicted translations are multiplied by s = sum g.p / sum p.p over the snippet (1 when
    the denominator is 0; the factor of inference.py:75), and the row is compute_pose_error of the two.  [0, 2] when
    n < length; 2 <= length <= 8."""
    if not 2 <= length <= 8:
        raise ValueError(f"length must be within 2..8, got {length}")
    g, r = _as44(gt), _as44(res)
    if g.shape != r.shape:
        raise ValueError(f"gt and res must hold the same number of poses, got {g.shape[0]} and {r.shape[0]}")
    rows = np.zeros((max(g.shape[0] - length + 1, 0), 2))
    for i in range(rows.shape[0]):
        a = np.linalg.inv(g[i]) @ g[i:i + length]
        p = np.linalg.inv(r[i]) @ r[i:i + length]
        den = float((p[:, :3, 3] * p[:, :3, 3]).sum())
        s = float((a[:, :3, 3] * p[:, :3, 3]).sum()) / den if den != 0.0 else 1.0
        p[:, :3, 3] *= s
        rows[i] = compute_pose_error(a[:, :3], p[:, :3])
    return rows


def load_poses(file_name):
    """{frame index: [4,4]} from lines of 12 numbers, or 13 with a leading frame index (evaluation_tools.py:394-417)."""
    poses = {}
    with open(file_name) as f:
        for cnt, line in enumerate(f):
            vals = [float(v) for v in line.split()]
            if not vals:
                continue
            with_idx = len(vals) == 13
            P = np.eye(4)
            P[:3, :4] = np.asarray(vals[with_idx:with_idx + 12]).reshape(3, 4)
            poses[int(vals[0]) if with_idx else cnt] = P
    return poses


def trajectory_distances(poses):
    """Cumulative path length along the sorted frames (evaluation_tools.py:419-435)."""
    keys = sorted(poses)
    t = np.stack([poses[k][:3, 3] for k in keys])
    return np.concatenate(([0.0], np.cumsum(np.linalg.norm(np.diff(t, axis=0), axis=1))))


def sequence_errors(poses_gt, poses_result):
    """Rows [first_frame, rot_err/len (rad/m), trans_err/len, len, speed] for every start frame 9, 19, ... and every
    segment length whose end exists in both trajectories (evaluation_tools.py:452-485).  Frames are positions in the
    sorted ground-truth list, as in the reference (its dict keys are 0..N-1)."""
    keys = sorted(poses_gt)
    dist = trajectory_distances(poses_gt)
    err = []
    for first in range(FIRST_FRAME, len(keys), FRAME_STEP):
        for length in SEGMENT_LENGTHS:
            beyond = np.nonzero(dist[first:] > dist[first] + length)[0]
            if beyond.size == 0:
                continue
            last = first + int(beyond[0])
            if first not in poses_result or last not in poses_result:
                continue
            d_gt = np.linalg.inv(poses_gt[first]) @ poses_gt[last]
            d_res = np.linalg.inv(poses_result[first]) @ poses_result[last]
            e = np.linalg.inv(d_res) @ d_gt
            r_err = float(np.arccos(np.clip(0.5 * (np.trace(e[:3, :3]) - 1.0), -1.0, 1.0)))
            t_err = float(np.linalg.norm(e[:3, 3]))
            speed = length / (FRAME_PERIOD * (last - first + 1.0))
            err.append([first, r_err / length, t_err / length, length, speed])
    return err


def overall_error(seq_err):
    """(average translational error, average rotational error) over the rows of sequence_errors (:494-508)."""
    if not seq_err:
        return float("nan"), float("nan")
    a = np.asarray(seq_err, dtype=np.float64)
    return float(a[:, 2].mean()), float(a[:, 1].mean())


def main(argv=None):
    """Evaluate a pose checkpoint on KITTI odometry sequences on the GPU (dvf.validation.validate_odometry: the functions above
    are its definition, restated in csrc/odometry.hip) and print one ``Odometry:`` line per sequence, then the line over all
    segments of all sequences (the line train.py --val-odometry prints after every epoch).  torch and the GPU are touched
    only here: importing this module stays numpy-only."""
    import argparse
    import torch
    from PoseExpNet_sfm import PoseExpNet
    from dataset import odometry_sequences
    from dvf import cli, validation
    parser = argparse.ArgumentParser(description="KITTI odometry evaluation of a pose network on MI355X",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--pretrained-pose", required=True, metavar="PATH",
                        help="PoseExpNet checkpoint (best_odometry_checkpoint.pth.tar / best_vo_checkpoint.pth.tar of train.py)")
    parser.add_argument("--val-root", required=True, metavar="DIR", help="KITTI odometry tree: sequences/<seq>/image_2, poses/<seq>.txt")
    parser.add_argument("--sequences", default=["09", "10"], type=str, nargs="+")
    parser.add_argument("--height", type=int, default=256)
    parser.add_argument("--width", type=int, default=832)
    parser.add_argument("-b", "--batch-size", type=int, default=4)
    parser.add_argument("--pose-convention", choices=list(validation.POSE_CONVENTIONS), default="se3",
                        help="se3 = (w, u) through the exponential map, what validate() scores; euler = (t, r-euler), what "
                             "train.py's photometric loss trains the outputs as")
    parser.add_argument("--output-dir", default=None, metavar="DIR", help="write <seq>.txt, one KITTI pose line per frame")
    parser.add_argument("--align", choices=list(ALIGN_MODES), default=None, metavar="MODE",
                        help="bring every chained trajectory onto its ground truth first, by one of " + ", ".join(ALIGN_MODES) +
                             " (scale: least squares about the origin; 6dof: rigid; 7dof: similarity, Umeyama; scale_7dof: the "
                             "scale of 7dof alone): the Odometry line is then that of the aligned trajectory, a Trajectory line "
                             "with ATE, RPE and the 5-frame-snippet ATE follows it, and --output-dir also gets <seq>_aligned.txt")
    args = parser.parse_args(argv)
    cli.require_gpu()
    device = torch.device("cuda", 0)
    net = PoseExpNet(nb_ref_imgs=2, output_exp=True)                     # validate()'s call feeds two reference views
    cli.load_pretrained(net, args.pretrained_pose, strict=False)
    net.to(device)
    sequences = odometry_sequences(args.val_root, args.sequences, args.height, args.width)
    if not sequences:
        raise SystemExit(f"no sequence of {args.sequences} under {args.val_root}/sequences")
    metrics = validation.validate_odometry(net, sequences, device, args.batch_size, convention=args.pose_convention,
                                           output_dir=args.output_dir, align=args.align)
    for name, m in metrics["per_sequence"].items():
        print(validation.format_odometry(m, name), flush=True)
        if args.align is not None:
            print(validation.format_trajectory(m, name), flush=True)
    print(validation.format_odometry(metrics), flush=True)
    if args.align is not None:
        print(validation.format_trajectory(metrics), flush=True)
    return metrics


if __name__ == "__main__":
    main()
