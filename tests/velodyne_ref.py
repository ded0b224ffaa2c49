"""Test-side definition of the LiDAR depth maps (dvf_velodyne_depth of include/dvf_hip.h), the inputs the tests share and a
tiny KITTI raw tree.

Two numpy fp64 functions, both written from the description of the reference's generate_depth_map
(tools/eval_depth_utils.py:172-224), not copied from it:
  reference_form   its steps in its order: project, divide, round, bounds, plain assignment (the last point of a pixel stays),
                   then the collision pass over the keys row * (W - 1) + col - 1 found with a Counter, then the clamp
  per_pixel_min    the definition of include/dvf_hip.h as a plain loop over the points; it also returns the smallest distance
                   of any projected coordinate to a half-integer, the margin by which a different fp64 evaluation order (about
                   1e-13) would have to move a coordinate before it rounds to another pixel
The reference's key is shared by pixel (r, W-1) and pixel (r+1, 0): the two forms may differ in columns 0 and W-1 and nowhere else.

No golden file can come from the reference itself: its module is Python 2 (iteritems, np.array(map(...)), np.int) and imports
cv2, so it does not import.  The calibration constants are KITTI's published 2011_09_26 calibration."""
import os
from collections import Counter

import numpy as np

# calib_cam_to_cam.txt / calib_velo_to_cam.txt of 2011_09_26
P_RECT_02 = [7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01, 0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01, 0.0, 0.0, 1.0, 2.745884e-03]
P_RECT_03 = [7.215377e+02, 0.0, 6.095593e+02, -3.395242e+02, 0.0, 7.215377e+02, 1.728540e+02, 2.199936e+00, 0.0, 0.0, 1.0, 2.729905e-03]
R_RECT_00 = [9.999239e-01, 9.837760e-03, -7.445048e-03, -9.869795e-03, 9.999421e-01, -4.278459e-03, 7.402527e-03, 4.351614e-03, 9.999631e-01]
VELO_R = [7.533745e-03, -9.999714e-01, -6.166020e-04, 1.480249e-02, 7.280733e-04, -9.998902e-01, 9.998621e-01, 7.523790e-03, 1.480755e-02]
VELO_T = [-4.069766e-03, -7.631618e-02, -2.717806e-01]
SHAPE = (37, 124)                       # KITTI's 375 x 1242 at a tenth
COUNTS = (1, 257, 5000, 20000)


def scaled(p_rect, scale=0.1):
    """A P_rect whose image is ``scale`` times the size: its first two rows scaled."""
    p = np.array(p_rect, dtype=np.float64).reshape(3, 4).copy()
    p[:2] *= scale
    return p


def compose(p_rect, r_rect, velo_r, velo_t):
    """P_rect @ R_rect (as 4x4) @ [R|T; 0 0 0 1], formed by hand."""
    rect, velo = np.eye(4), np.eye(4)
    rect[:3, :3] = np.array(r_rect, dtype=np.float64).reshape(3, 3)
    velo[:3, :3] = np.array(velo_r, dtype=np.float64).reshape(3, 3)
    velo[:3, 3] = np.array(velo_t, dtype=np.float64)
    return np.array(p_rect, dtype=np.float64).reshape(3, 4) @ rect @ velo


def base_proj(scale=0.1):
    return compose(scaled(P_RECT_02, scale), R_RECT_00, VELO_R, VELO_T)


def gen_points(n, seed):
    """n float32 points uniform in [-5,60] x [-25,25] x [-2,1.5] (forward, left, up) with a random reflectance."""
    rng = np.random.RandomState(seed)
    lo, hi = np.array([-5.0, -25.0, -2.0, 0.0]), np.array([60.0, 25.0, 1.5, 1.0])
    return (lo + (hi - lo) * rng.uniform(size=(n, 4))).astype(np.float32)


def _project(P, points):
    """(kept points, raw coordinates [n,2], camera depth [n]) of the points with forward >= 0."""
    pts = np.asarray(points, dtype=np.float64)[:, :3]
    pts = pts[pts[:, 0] >= 0]
    hom = np.concatenate([pts, np.ones((pts.shape[0], 1))], axis=1)
    cam = hom @ np.asarray(P, dtype=np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = cam[:, :2] / cam[:, 2:3]
    return pts, raw, cam[:, 2]


def reference_form(P, points, shape, vel_depth=False):
    H, W = shape
    pts, raw, z = _project(P, points)
    d = pts[:, 0] if vel_depth else z
    with np.errstate(invalid="ignore"):
        col, row = np.round(raw[:, 0]) - 1, np.round(raw[:, 1]) - 1
        val = (col >= 0) & (row >= 0) & (col < W) & (row < H)
    col, row, d = col[val], row[val], d[val]
    depth = np.zeros((H, W), dtype=np.float64)
    depth[row.astype(np.int64), col.astype(np.int64)] = d
    keys = row * (W - 1) + col - 1
    for key in [k for k, count in Counter(keys.tolist()).items() if count > 1]:
        hit = np.where(keys == key)[0]
        depth[int(row[hit[0]]), int(col[hit[0]])] = d[hit].min()
    depth[depth < 0] = 0
    return depth


def per_pixel_min(P, points, shape, vel_depth=False):
    """(depth [H,W] float64, margin): margin = min |c - round-half-boundary| over every finite projected coordinate c of a
    point with forward >= 0 (inf when there is none)."""
    H, W = shape
    pts, raw, z = _project(P, points)
    d = pts[:, 0] if vel_depth else z
    best = np.full((H, W), np.inf)
    margin = np.inf
    for i in range(pts.shape[0]):
        cu, cv = raw[i]
        for c in (cu, cv):
            if np.isfinite(c):
                margin = min(margin, abs(c - np.floor(c) - 0.5))
        if not (np.isfinite(cu) and np.isfinite(cv)):
            continue
        u, v = np.round(cu) - 1, np.round(cv) - 1
        if u >= 0 and v >= 0 and u < W and v < H:
            best[int(v), int(u)] = min(best[int(v), int(u)], d[i])
    depth = np.where(np.isinf(best) & (best > 0), 0.0, np.maximum(best, 0.0))
    return depth, margin


# ------------------------------------------------------------------ the hand-worked case
# proj = K @ [axes | t]: camera x = -left, y = -up, z = forward - 1, K = [[4,0,4],[0,4,2],[0,0,1]].  With X = forward - 1:
# raw column = 4 - 4 * left / X, raw row = 2 - 4 * up / X, depth = X; every entry and every X is a power of two (or -1/2), so
# every product, sum and quotient below is exact in fp64 whatever the evaluation order.
HAND_SHAPE = (6, 8)
HAND_PROJ = np.array([[4.0, -4.0, 0.0, -4.0], [2.0, 0.0, -4.0, -2.0], [1.0, 0.0, 0.0, -1.0]])
HAND_POINTS = np.array([
    [9.0, 2.0, 0.0, 0.3],        # raw (3, 2) -> pixel (row 1, col 2), depth 8
    [5.0, 1.0, 0.0, 0.1],        # the same pixel, depth 4: the nearer point comes second
    [5.0, -1.0, 0.0, 0.9],       # raw (5, 2) -> (1, 4), depth 4: the nearer point comes first
    [9.0, -2.0, 0.0, 0.0],       # the same pixel, depth 8
    [-1.0, 0.5, 0.0, 0.5],       # forward < 0: dropped (it would land on (1, 4) with depth -2 and zero it)
    [17.0, 15.0, 0.0, 0.5],      # raw column 0.25 rounds to 0 -> -1: dropped
    [9.0, 0.0, 3.0, 0.5],        # raw row 0.5 rounds (half to even) to 0 -> -1: dropped
    [3.0, -2.0, 0.0, 0.5],       # raw column 8 = W -> column 7: (1, 7), depth 2
    [17.0, -17.0, -4.0, 0.5],    # raw (8.25, 3) -> (2, 7), depth 16
    [9.0, -9.0, -4.0, 0.5],      # raw (8.5, 4): half to even gives 8 -> (3, 7), depth 8
    [5.0, -5.0, 0.0, 0.5],       # raw column 9 -> 8 = W: dropped
    [3.0, 0.0, -2.0, 0.5],       # raw (4, 6): row 6 = H -> row 5: (5, 3), depth 2
    [5.0, 0.0, -5.0, 0.5],       # raw row 7 -> 6 = H: dropped
    [9.0, 3.0, -2.0, 0.5],       # raw column 2.5 -> 2 (half to even) -> column 1: (2, 1), depth 8
    [9.0, 1.0, -2.0, 0.5],       # raw column 3.5 -> 4 (half to even) -> column 3: (2, 3), depth 8
    [5.0, -2.0, -3.0, 0.5],      # raw (6, 5) -> (4, 5), depth 4
    [0.5, 0.25, 0.375, 0.5],     # forward >= 0 but X = -1/2: raw (6, 5) -> (4, 5) with depth -1/2: the pixel becomes 0
    [1.0, 1.0, 0.0, 0.5],        # X = 0: -4 / 0 = -inf: dropped
    [1.0, 0.0, 0.0, 0.5],        # X = 0: 0 / 0 = NaN: dropped
    [np.nan, 0.0, 0.0, 0.5],     # NaN forward: dropped
], dtype=np.float32)
HAND_DEPTH = np.array([
    [0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 4, 0, 4, 0, 0, 2],
    [0, 8, 0, 8, 0, 0, 0, 16],
    [0, 0, 0, 0, 0, 0, 0, 8],
    [0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 2, 0, 0, 0, 0]], dtype=np.float32)
HAND_DEPTH_VELODYNE = np.array([        # vel_depth: the forward distance X + 1; the X = -1/2 point stores 0.5, the nearest of (4, 5)
    [0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 5, 0, 5, 0, 0, 3],
    [0, 9, 0, 9, 0, 0, 0, 17],
    [0, 0, 0, 0, 0, 0, 0, 9],
    [0, 0, 0, 0, 0, 0.5, 0, 0],
    [0, 0, 0, 3, 0, 0, 0, 0]], dtype=np.float32)


# ------------------------------------------------------------------ the inputs of tests/test_gpu_velodyne.py
BATCH_COUNTS = (257, 0, 5000)


def batch_case():
    """One B = 3 call at SHAPE: (points [total,4], offsets [4], proj [3,3,4]) with an empty frame in the middle and the
    translation column of the base matrix perturbed per frame."""
    frames = [gen_points(n, seed=100 + i) for i, n in enumerate(BATCH_COUNTS)]
    proj = np.stack([base_proj() for _ in BATCH_COUNTS])
    for b in range(len(BATCH_COUNTS)):
        proj[b, :, 3] += np.array([0.37, -0.21, 0.013]) * b
    offsets = np.concatenate([[0], np.cumsum(BATCH_COUNTS)]).astype(np.int32)
    return np.concatenate(frames), offsets, proj


CONTENTION_SHAPE = (4, 4)
CONTENTION_PROJ = np.array([[2.5, -1.0, 0.0, 0.0], [2.5, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])


def contention_case(n=20000, seed=7):
    """n points that all land on a 4 x 4 map: raw coordinates 2.5 + a with a uniform in (-1.9, 1.9), depth = forward."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(2.0, 50.0, size=n)
    a = rng.uniform(-1.9, 1.9, size=(n, 2))
    return np.stack([x, -a[:, 0] * x, -a[:, 1] * x, rng.uniform(size=n)], axis=1).astype(np.float32)


def gpu_inputs():
    """(name, proj [3,4], points, shape) of every random single-frame input the GPU tests compare exactly: the half-integer
    margin of each must be large against fp64 evaluation-order differences (tests/test_velodyne.py asserts it).  The
    hand-worked case is not listed: its coordinates are exact by construction, half-integers included."""
    points, offsets, proj = batch_case()
    out = [(f"batch frame {b}", proj[b], points[offsets[b]:offsets[b + 1]], SHAPE) for b in range(len(BATCH_COUNTS))]
    out.append(("contention", CONTENTION_PROJ, contention_case(), CONTENTION_SHAPE))
    # the offsets test re-splits the batch's points: frame 0 under a clamped end, frame 2's matrix over the whole buffer
    out.append(("clamped range", proj[0], points, SHAPE))
    out.append(("whole buffer, frame 2", proj[2], points, SHAPE))
    for name, sizes, n in RAW_TREE_FRAMES:
        out.append((f"raw tree {name}", tree_proj(), tree_points(name, n), sizes))
    return out


# ------------------------------------------------------------------ a tiny KITTI raw tree
DATE = "2011_09_26"
DRIVES = (DATE + "_drive_0002_sync", DATE + "_drive_0009_sync")
# (frame name = <drive index>/<id>, original image size, points)
RAW_TREE_FRAMES = (("0/0000000005", (37, 122), 3000), ("0/0000000007", (37, 122), 2500), ("1/0000000000", (40, 130), 3000),
                   ("1/0000000013", (40, 130), 2000))


def tree_points(name, n):
    return gen_points(n, seed=sum(ord(c) for c in name))


def _fmt(values):
    return " ".join("%.6e" % v for v in values)


def calib_texts(scale=0.1):
    """The two calibration files as text: a date line, scientific notation, keys the readers do not need."""
    cam = ("calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\n"
           f"S_02: 1.392000e+03 5.120000e+02\nR_rect_00: {_fmt(R_RECT_00)}\n"
           f"P_rect_02: {_fmt(scaled(P_RECT_02, scale).ravel())}\nP_rect_03: {_fmt(scaled(P_RECT_03, scale).ravel())}\n")
    velo = (f"calib_time: 15-Mar-2012 11:37:16\nR: {_fmt(VELO_R)}\nT: {_fmt(VELO_T)}\n"
            "delta_f: 0.000000e+00 0.000000e+00\ndelta_c: 0.000000e+00 0.000000e+00\n")
    return cam, velo


def written(values):
    """The numbers a reader gets back from _fmt's text."""
    return [float("%.6e" % v) for v in values]


def tree_proj(cam=2, scale=0.1):
    """What velo_to_image must return for the files of calib_texts, formed by hand from the numbers as written."""
    p = P_RECT_02 if cam == 2 else P_RECT_03
    return compose(written(scaled(p, scale).ravel()), written(R_RECT_00), written(VELO_R), written(VELO_T))


def write_calib(directory, scale=0.1):
    os.makedirs(directory, exist_ok=True)
    for name, text in zip(("calib_cam_to_cam.txt", "calib_velo_to_cam.txt"), calib_texts(scale)):
        with open(os.path.join(directory, name), "w") as f:
            f.write(text)


def make_raw_tree(root, frames=RAW_TREE_FRAMES, calib_in_drive=False, cams=(2,), seed=3):
    """A KITTI raw tree under ``root`` with the frames of ``frames`` (random PNG images of the given size, sweeps of
    tree_points) and a split file whose lines carry a trailing field; returns the split file's path."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    lines = []
    if not calib_in_drive:
        write_calib(os.path.join(root, DATE))
    for name, (h, w), n in frames:
        drive, frame_id = DRIVES[int(name.split("/")[0])], name.split("/")[1]
        base = os.path.join(root, DATE, drive)
        if calib_in_drive:
            write_calib(os.path.join(base, "calib"))
        for cam in cams:
            os.makedirs(os.path.join(base, f"image_0{cam}", "data"), exist_ok=True)
            Image.fromarray(rng.randint(0, 256, size=(h, w, 3), dtype=np.uint8)).save(
                os.path.join(base, f"image_0{cam}", "data", frame_id + ".png"))
        os.makedirs(os.path.join(base, "velodyne_points", "data"), exist_ok=True)
        tree_points(name, n).tofile(os.path.join(base, "velodyne_points", "data", frame_id + ".bin"))
        lines.append(f"{DATE}/{drive}/image_02/data/{frame_id}.png {DATE}/{drive}/image_03/data/{frame_id}.png")
    split = os.path.join(root, "split.txt")
    with open(split, "w") as f:
        f.write("\n".join(lines) + "\n")
    return split
