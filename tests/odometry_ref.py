"""Trajectory generators and host-side helpers of the odometry-evaluation tests.  The DEFINITION of everything compared is
odometry_eval.py's numpy code (se3_cam2world, sequence_errors, overall_error); this module only makes inputs for it: seeded,
float64, steps of 0.5-1.5 m, yaw / pitch / roll increments large enough that the products do not commute."""
import functools
import math

import numpy as np

import odometry_eval as oe

CHAIN_SIZES = (0, 1, 2, 255, 256, 257, 1000, 4541)       # chunk and block boundaries of a 256-wide scan; 4541 = KITTI's longest
RAGGED_OFFSETS = (0, 0, 300, 1000)                       # an empty sequence first
SHORT_SIZES = (9, 10, 11, 60)


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])


def _euler(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


@functools.lru_cache(maxsize=None)
def relative_poses(n, seed, yaw_bias=0.0, noise=0.0, scale=1.0, noise_seed=0):
    """[n,4,4] float64 frame-to-frame poses: forward steps of 0.5-1.5 m with some sideways motion, yaw within +-0.05 rad and
    pitch / roll within +-0.02 rad per step.  ``yaw_bias`` / ``noise`` / ``scale`` perturb THE SAME walk (a constant yaw drift
    per frame, rotation noise of that size per step, a scale error of the steps): every output is rigid."""
    rng = np.random.default_rng(seed)
    prng = np.random.default_rng(10_000 + noise_seed)
    out = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        yaw, pitch, roll = rng.uniform(-0.05, 0.05), rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)
        t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05), rng.uniform(0.5, 1.5)])
        dy, dp, dr = prng.uniform(-1, 1, 3) * noise
        out[i, :3, :3] = _euler(yaw + yaw_bias + dy, pitch + dp, roll + dr)
        out[i, :3, 3] = t * scale
    out.setflags(write=False)
    return out


def chain_input(n, seed=7):
    """The chain tests' input: the walk rounded to fp32 (what a network hands over), as [n,4,4] float32."""
    return relative_poses(n, seed).astype(np.float32)


def world_of(rel):
    """[n+1,4,4]: the definition's chain."""
    return np.stack(oe.se3_cam2world(list(rel)))


def world_reversed(rel):
    """The chain with the operands swapped, T_k = P_k @ T_{k-1}: what a left/right mistake computes."""
    out = [np.eye(4)]
    for p in rel:
        out.append(np.asarray(p, dtype=np.float64) @ out[-1])
    return np.stack(out)


def tree_prefix(rel):
    """Inclusive prefix products of [n,4,4] in Hillis-Steele (pairwise) association, the earlier factor on the left."""
    out = np.asarray(rel, dtype=np.float64).copy()
    d = 1
    while d < out.shape[0]:
        out[d:] = out[:-d] @ out[d:]
        d *= 2
    return out


def straight(n, step):
    """[n,4,4]: identity rotations, z = i * step (tests/test_odometry_eval.py::_straight)."""
    out = np.tile(np.eye(4), (n, 1, 1))
    out[:, 2, 3] = np.arange(n) * step
    return out


def as_dict(traj):
    return {i: np.asarray(p, dtype=np.float64) for i, p in enumerate(traj)}


@functools.lru_cache(maxsize=None)
def curved(n, seed):
    w = world_of(relative_poses(n - 1, seed))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def drifted(n, seed):
    """The walk of ``curved(n, seed)`` with a yaw drift of 3e-4 rad per frame, rotation noise of 2e-4 rad per step and a 3 %
    scale error: over a segment of >= 67 frames the rotation error is >= 1e-2 rad."""
    w = world_of(relative_poses(n - 1, seed, yaw_bias=3e-4, noise=2e-4, scale=1.03, noise_seed=seed))
    w.setflags(write=False)
    return w


# ---- the (gt, res) pairs the GPU tests evaluate, by name.  "relative": rows are compared at a relative tolerance
# (seeds picked for the input condition of test_odometry_device.py: no frame within 1e-6 * length of a segment threshold)
CURVED = (1500, 16)
ACCUMULATE = ((1500, 16), (800, 12))


def error_case(name):
    if name == "identical":
        return straight(1200, 1.0), straight(1200, 1.0)
    if name == "scale":
        return straight(400, 1.0), straight(400, 1.1)
    if name == "yaw":
        gt = straight(300, 1.0)
        return gt, np.stack([rot_y(YAW * i) @ gt[i] for i in range(300)])
    if name == "curved":
        return curved(*CURVED), drifted(*CURVED)
    if name == "second":
        return curved(*ACCUMULATE[1]), drifted(*ACCUMULATE[1])
    if name.startswith("short"):
        n = int(name[5:])
        return straight(n, 1.0), straight(n, 1.1)
    raise KeyError(name)


YAW = 0.002
ERROR_CASES = ("identical", "scale", "yaw", "curved", "second") + tuple(f"short{n}" for n in SHORT_SIZES)
RELATIVE_CASES = ("curved", "second")


def end_to_end_gt(n=20, step=12.0):
    """Ground truth of the end-to-end tree: steps of 12 m along z with a slow yaw, so the 100 m segment from frame 9 exists."""
    return np.stack([straight(n, step)[i] @ rot_y(0.01 * i) for i in range(n)])


def threshold_margin(traj):
    """min over (first, length, k) of |dist[k] - (dist[first] + length)| / length: how far, relative to the segment length,
    any frame lies from a segment-end threshold."""
    dist = oe.trajectory_distances(as_dict(traj))
    best = float("inf")
    for first in range(oe.FIRST_FRAME, len(dist), oe.FRAME_STEP):
        for length in oe.SEGMENT_LENGTHS:
            best = min(best, float(np.abs(dist - (dist[first] + length)).min()) / length)
    return best


def exact_distances(traj):
    """True when every step length is a whole number below 2^20: the path length is then exact in fp64 in ANY summation order
    and a reordered sum reproduces the sequential one bit for bit, ties with a threshold included."""
    steps = np.linalg.norm(np.diff(np.asarray(traj)[:, :3, 3], axis=0), axis=1)
    return bool(np.all(steps == np.round(steps)) and steps.sum() < 2 ** 20)


def make_tree(root, gt, seq="00", h=64, w=208, seed=3):
    """A KITTI-odometry-shaped tree of one sequence: sequences/<seq>/image_2/%06d.png (h x w noise) and poses/<seq>.txt."""
    import os
    from PIL import Image
    rng = np.random.default_rng(seed)
    d = os.path.join(str(root), "sequences", seq, "image_2")
    os.makedirs(d)
    os.makedirs(os.path.join(str(root), "poses"), exist_ok=True)
    for i in range(len(gt)):
        Image.fromarray(rng.integers(10, 240, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(d, f"{i:06d}.png"))
    with open(os.path.join(str(root), "poses", f"{seq}.txt"), "w") as f:
        for p in gt:
            f.write(" ".join(repr(float(v)) for v in np.asarray(p)[:3, :4].reshape(12)) + "\n")
    return str(root)
