"""Inputs of the trajectory-alignment tests, built on tests/odometry_ref.py.  The DEFINITION of everything compared is
odometry_eval.py's numpy code (trajectory_alignment, apply_alignment, trajectory_errors, snippet_errors); this module only
makes (gt, res) pairs for it and holds a second, independent rotation solver (Horn's quaternion form) to show that the
definition's answer is a property of the problem, not of numpy's SVD."""
import functools

import numpy as np

import odometry_eval as oe
import odometry_ref as R

SEED = 16
ALIGN_SIZES = (3, 5, 255, 256, 257, 1000, 1500, 4541)    # block boundaries of 256-frame partial sums; 4541 = KITTI's longest
MIRROR_SIZES = (257, 1500)
ERROR_SIZES = (2, 257, 1500)
SNIPPET_SIZES = (5, 6, 256, 260, 261, 1500)              # length 5: 1, 2, 252, 256, 257 rows (one block, a block and one row)
SNIPPET_LENGTHS = (2, 5, 8)
OFFSET = (3e5, 0.0, 5.7e6)                               # a UTM-sized common offset
SIMILARITY = (1.0 / 1.7, (0.3, -0.2, 0.1), (5.0, -3.0, 11.0))
CONDITION = 5e-4                                         # (sv[1] +- sv[2]) / sv[0] of every case compared relatively
MIN_ANGLE = 1e-4                                         # rad, of every angle compared relatively


def pair(n, seed=SEED):
    """(gt, res) = (curved, drifted) of n frames, [n,4,4] each."""
    return R.curved(n, seed), R.drifted(n, seed)


@functools.lru_cache(maxsize=None)
def similar(n=1500, seed=SEED):
    """(gt, res): res is gt under the similarity SIMILARITY (scale 1/1.7, a rotation, a shift), so 7dof recovers c = 1.7."""
    scale, angles, shift = SIMILARITY
    gt = R.curved(n, seed)
    res = np.array(gt)
    rot = R._euler(*angles)
    res[:, :3, :3] = rot @ gt[:, :3, :3]
    res[:, :3, 3] = scale * (gt[:, :3, 3] @ rot.T) + np.asarray(shift)
    res.setflags(write=False)
    return gt, res


def mirrored(traj):
    """The trajectory with its x-translations negated: no rotation maps it back, det U det V < 0 in the definition."""
    out = np.array(traj)
    out[:, 0, 3] *= -1.0
    return out


def shifted(traj, offset=OFFSET):
    out = np.array(traj)
    out[:, :3, 3] += np.asarray(offset)
    return out


def zero_translations(traj):
    out = np.array(traj)
    out[:, :3, 3] = 0.0
    return out


def aligned_pair(n, mode="7dof", seed=SEED):
    """(gt, the definition's aligned res)."""
    gt, res = pair(n, seed)
    c, rot, t, _ = oe.trajectory_alignment(gt, res, mode)
    return gt, oe.apply_alignment(res, c, rot, t)


def end_to_end_gt(n=20, step=12.0, yaw=0.05, pitch=0.01):
    """Ground truth of the end-to-end tree: a chained walk of 12 m steps that turns by ``yaw`` and ``pitch`` every frame, so
    its positions are not collinear (odometry_ref.end_to_end_gt turns the camera on a straight line of positions, which has
    no unique alignment rotation) and the 100 m segment from frame 9 exists."""
    rel = np.tile(np.eye(4), (n - 1, 1, 1))
    rel[:, :3, :3] = R._euler(yaw, pitch, 0.0)
    rel[:, 2, 3] = step
    return R.world_of(rel)


def horn(gt, res):
    """(c, R) of the similarity res -> gt by Horn's closed form (unit quaternion = the top eigenvector of a 4x4 symmetric
    matrix of the cross-covariance, numpy eigh): independent of the SVD, and a proper rotation by construction."""
    x = np.asarray(res, dtype=np.float64)[:, :3, 3]
    y = np.asarray(gt, dtype=np.float64)[:, :3, 3]
    xc, yc = x - x.mean(0), y - y.mean(0)
    S = xc.T @ yc / len(x)                                 # S[a][b] = mean x_a y_b
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    w, v = np.linalg.eigh(N)
    q0, q1, q2, q3 = v[:, -1]
    rot = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                    [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                    [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])
    c = float((yc * (xc @ rot.T)).sum() / (xc * xc).sum())
    return c, rot


def pair_angles(gt, res):
    """The per-pair RPE angles (radians) of the definition, one per consecutive pair."""
    g, r = oe._as44(gt), oe._as44(res)
    E = np.linalg.inv(np.linalg.inv(g[:-1]) @ g[1:]) @ (np.linalg.inv(r[:-1]) @ r[1:])
    return oe._angles(E[:, :3, :3])


def snippet_stats(rows):
    """(mean ate, population std of ate, mean re) of the definition's rows, by numpy."""
    return float(rows[:, 0].mean()), float(rows[:, 0].std()), float(rows[:, 1].mean())
