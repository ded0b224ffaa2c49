"""dvf_velodyne_depth on the GPU against the test-side definition (tests/velodyne_ref.py), and the command lines that use it.

Every comparison is exact: occupancy on all pixels, values equal to the fp32 cast of the fp64 definition.  That is legitimate
because no projected coordinate of these inputs lies within 1e-9 of a rounding boundary (tests/test_velodyne.py asserts it; fp64
evaluation-order differences are about 1e-13), so every point lands on the pixel the definition gives it, and the stored
depth is one cast of an fp64 value that differs from the definition's by about 1e-16 relative, against fp32 steps of 6e-8."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import velodyne_ref as V
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _call(points, offsets, proj, out, total=None, flags=0):
    """The C entry on device tensors, with an output buffer and a point count of the caller's choosing."""
    from dvf import lib as L
    B, H, W = out.shape
    total = points.shape[0] if total is None else total
    rc = L.lib().dvf_velodyne_depth(points.data_ptr() if points.numel() else None, offsets.data_ptr(), proj.data_ptr(),
                                    out.data_ptr(), B, H, W, total, flags, L.stream())
    torch.cuda.synchronize()
    return rc


def _dev(points, offsets, proj):
    return (torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(DEV),
            torch.from_numpy(np.asarray(offsets, dtype=np.int32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(proj, dtype=np.float64)).reshape(-1, 3, 4).to(DEV))


def _maps(points, offsets, proj, shape, vel=False):
    from dvf.velodyne import depth_maps
    out = depth_maps(*_dev(points, offsets, proj), *shape, velodyne_depth=vel)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.is_cuda
    return out.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def batch():
    """The B = 3 case and both test-side forms of each of its frames, for both flag values, computed once."""
    points, offsets, proj = V.batch_case()
    ref = {}
    for vel in (False, True):
        for b in range(len(V.BATCH_COUNTS)):
            pts = points[offsets[b]:offsets[b + 1]]
            ref[vel, b] = (V.per_pixel_min(proj[b], pts, V.SHAPE, vel)[0], V.reference_form(proj[b], pts, V.SHAPE, vel))
    return points, offsets, proj, ref


@pytest.mark.parametrize("vel", [False, True])
def test_hand_worked_case_overwrites_a_nan_filled_buffer(vel):
    points, offsets, proj = _dev(V.HAND_POINTS, [0, len(V.HAND_POINTS)], V.HAND_PROJ)
    out = torch.full((1,) + V.HAND_SHAPE, float("nan"), device=DEV)
    assert _call(points, offsets, proj, out, flags=1 if vel else 0) == 0
    want = V.HAND_DEPTH_VELODYNE if vel else V.HAND_DEPTH
    assert _same_bits(out.cpu().numpy()[0], want), out.cpu().numpy()[0]
    # the Python entry, and the points in the other order
    assert _same_bits(_maps(V.HAND_POINTS[::-1].copy(), [0, len(V.HAND_POINTS)], V.HAND_PROJ, V.HAND_SHAPE, vel)[0], want)


@pytest.mark.parametrize("vel", [False, True])
def test_batch_of_three_frames_against_both_forms(batch, vel):
    points, offsets, proj, ref = batch
    got = _maps(points, offsets, proj, V.SHAPE, vel)
    assert got.shape == (3,) + V.SHAPE
    for b, n in enumerate(V.BATCH_COUNTS):
        mine, form = ref[vel, b]
        assert np.array_equal(got[b] > 0, mine > 0), (b, "occupancy")
        assert _same_bits(got[b], mine.astype(np.float32)), (b, int((got[b] != mine.astype(np.float32)).sum()))
        assert _same_bits(got[b][:, 1:-1], form[:, 1:-1].astype(np.float32)), (b, "reference form")
        assert (got[b] > 0).any() == (n > 0)
    assert not np.array_equal(got[0], got[2])


def test_contention_on_a_four_by_four_map():
    pts = V.contention_case()
    want, _ = V.per_pixel_min(V.CONTENTION_PROJ, pts, V.CONTENTION_SHAPE)
    got = _maps(pts, [0, len(pts)], V.CONTENTION_PROJ, V.CONTENTION_SHAPE)[0]
    assert (want > 0).all() and _same_bits(got, want.astype(np.float32)), (got, want)


def test_wrong_offsets_are_clamped(batch):
    """A decreasing pair is an empty frame and every end is clamped to [0, total].  The buffer holds rows beyond ``total`` up to
    the largest offset used, so a missing clamp would read allocated memory and show as a wrong map, not as a fault."""
    points, offsets, proj, _ = batch
    total, beyond = len(points), 6000
    near = np.tile(np.array([[3.0, 0.0, -0.5, 0.0]], dtype=np.float32), (beyond - total, 1))    # would land mid-image, 3 m away
    padded, _, dproj = _dev(np.concatenate([points, near]), [0], proj)
    assert (V.per_pixel_min(proj[0], near, V.SHAPE)[0] > 0).any()

    def frame(b, lo, hi):
        return V.per_pixel_min(proj[b], points[lo:hi], V.SHAPE)[0].astype(np.float32)

    # an entry beyond total
    off = torch.tensor([0, beyond, total], dtype=torch.int32, device=DEV)
    out = torch.full((2,) + V.SHAPE, float("nan"), device=DEV)
    assert _call(padded, off, dproj[:2].contiguous(), out, total=total) == 0
    got = out.cpu().numpy()
    assert _same_bits(got[0], frame(0, 0, total)) and not got[1].any()
    # a negative entry and a decreasing pair
    off = torch.tensor([-5, 3000, 1000, total], dtype=torch.int32, device=DEV)
    out = torch.full((3,) + V.SHAPE, float("nan"), device=DEV)
    assert _call(padded, off, dproj, out, total=total) == 0
    got = out.cpu().numpy()
    assert _same_bits(got[0], frame(0, 0, 3000)) and not got[1].any() and _same_bits(got[2], frame(2, 1000, total))


def test_eager_runs_and_graph_replays_are_bit_identical(batch):
    from dvf.velodyne import depth_maps
    points, offsets, proj, ref = batch
    dp, do, dj = _dev(points, offsets, proj)
    runs = []
    for _ in range(2):
        runs.append(depth_maps(dp, do, dj, *V.SHAPE))
        torch.cuda.synchronize()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = depth_maps(dp, do, dj, *V.SHAPE)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        runs.append(out.clone())
    first = runs[0].cpu().numpy()
    assert _same_bits(first[2], ref[False, 2][0].astype(np.float32))
    for r in runs[1:]:
        assert _same_bits(r.cpu().numpy(), first)


# ------------------------------------------------------------------ the command lines

def _depth_lines(stdout):
    return [line for line in stdout.splitlines() if line.startswith("Depth: ")]


@pytest.fixture(scope="module")
def raw_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("raw"))
    return root, V.make_raw_tree(root)


def test_depth_eval_on_the_raw_tree_and_on_its_export(raw_tree, tmp_path):
    from DispNetS import DispNetS
    root, split = raw_tree
    torch.manual_seed(11)
    net = DispNetS()
    net.init_weights()
    ckpt = str(tmp_path / "disp.pth.tar")
    torch.save(net.state_dict(), ckpt)
    out = str(tmp_path / "export")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    common = [sys.executable, os.path.join(PKG, "depth_eval.py"), "--pretrained-disp", ckpt, "--height", "64", "--width", "208", "-b", "2"]
    raw = subprocess.run(common + ["--kitti-raw-root", root, "--split", split, "--export-depth-root", out], capture_output=True,
                         text=True, timeout=600, env=env)
    assert raw.returncode == 0, raw.stderr[-2000:]
    first = _depth_lines(raw.stdout)
    assert len(first) == 1 and len(first[0].split()) == 17, raw.stdout[-2000:]
    numbers = [float(v) for v in first[0].split()[2::2]]
    assert all(v == v for v in numbers) and numbers[1] > 0                       # abs_rel of a real comparison
    # the exported tree: the stems, the image bytes, and every map equal to the definition
    frames = V.RAW_TREE_FRAMES
    stems = [V.DRIVES[int(name.split("/")[0])] + "_" + name.split("/")[1] for name, _, _ in frames]
    assert open(os.path.join(out, "val.txt")).read().split() == stems
    for stem, (name, shape, n) in zip(stems, frames):
        src = os.path.join(root, V.DATE, V.DRIVES[int(name.split("/")[0])], "image_02", "data", name.split("/")[1] + ".png")
        assert open(os.path.join(out, "image", stem + ".png"), "rb").read() == open(src, "rb").read()
        depth = np.load(os.path.join(out, "depth", stem + ".npy"))
        assert depth.dtype == np.float32 and depth.shape == shape
        want = V.per_pixel_min(V.tree_proj(), V.tree_points(name, n), shape)[0].astype(np.float32)
        assert _same_bits(depth, want) and (depth > 0).sum() > 100
    again = subprocess.run(common + ["--val-depth-root", out], capture_output=True, text=True, timeout=600, env=env)
    assert again.returncode == 0, again.stderr[-2000:]
    assert _depth_lines(again.stdout) == first                                   # string for string


def test_train_validates_depth_on_the_raw_tree(raw_tree, tmp_path):
    root, split = raw_tree
    out = tmp_path / "ckpt"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "-b", "2", "--epochs", "1", "--steps-per-epoch", "1", "--height", "64",
           "--width", "208", "--val-kitti-raw-root", root, "--val-split", split, "--output-dir", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = _depth_lines(res.stdout)
    assert len(lines) == 1 and "[BEST:True]" in lines[0], res.stdout[-2000:]
    assert os.path.exists(os.path.join(out, "best_depth_checkpoint.pth.tar"))
