"""The LiDAR depth maps without a GPU: the two test-side forms against each other and against a hand-worked case, the host
checks of dvf_velodyne_depth, the calibration readers and the KITTI raw set (definitions: tests/velodyne_ref.py,
include/dvf_hip.h)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import velodyne_ref as V


@pytest.fixture(scope="module")
def forms():
    """{(n, vel_depth): (reference_form, per_pixel_min, margin)} over the seeded inputs, computed once."""
    P, out = V.base_proj(), {}
    for n in V.COUNTS:
        pts = V.gen_points(n, seed=n)
        for vel in (False, True):
            out[n, vel] = (V.reference_form(P, pts, V.SHAPE, vel),) + V.per_pixel_min(P, pts, V.SHAPE, vel)
    return out


@pytest.mark.parametrize("vel", [False, True])
@pytest.mark.parametrize("n", V.COUNTS)
def test_the_two_forms_agree_inside_the_border_columns(forms, n, vel):
    ref, mine, _ = forms[n, vel]
    a, b = ref[:, 1:-1], mine[:, 1:-1]
    assert np.array_equal(a > 0, b > 0)
    assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b))
    assert np.array_equal(a.astype(np.float32), b.astype(np.float32))
    rows, cols = np.nonzero(ref != mine)
    assert set(cols.tolist()) <= {0, V.SHAPE[1] - 1}, sorted(set(cols.tolist()))
    if n >= 257:
        assert (mine > 0).sum() > 20                                   # the case is not vacuous


def test_half_integer_margin_of_every_exactly_compared_input(forms):
    """An exact comparison needs every projected coordinate well away from a rounding boundary: fp64 evaluation-order
    differences are about 1e-13."""
    for (n, vel), (_, _, margin) in forms.items():
        assert margin > 1e-9, (n, margin)
    for name, proj, points, shape in V.gpu_inputs():
        margin = V.per_pixel_min(proj, points, shape)[1]
        print(f"{name}: margin {margin:.3g}")
        assert margin > 1e-9, (name, margin)


def test_hand_worked_case():
    for vel, want in ((False, V.HAND_DEPTH), (True, V.HAND_DEPTH_VELODYNE)):
        mine, margin = V.per_pixel_min(V.HAND_PROJ, V.HAND_POINTS, V.HAND_SHAPE, vel)
        assert margin == 0.0                                           # it holds exact half-integers, on purpose
        assert np.array_equal(mine, want.astype(np.float64)), mine
        ref = V.reference_form(V.HAND_PROJ, V.HAND_POINTS, V.HAND_SHAPE, vel)
        assert np.array_equal(ref[:, 1:-1], want[:, 1:-1].astype(np.float64)), ref
    # either order of the two points of a pixel
    flipped = V.HAND_POINTS[::-1].copy()
    assert np.array_equal(V.per_pixel_min(V.HAND_PROJ, flipped, V.HAND_SHAPE)[0], V.HAND_DEPTH.astype(np.float64))


def test_contention_case_lands_on_the_map():
    pts = V.contention_case()
    depth, _ = V.per_pixel_min(V.CONTENTION_PROJ, pts, V.CONTENTION_SHAPE)
    assert np.all(depth > 0)
    _, raw, _ = V._project(V.CONTENTION_PROJ, pts)
    assert raw.min() > 0.5 and raw.max() < 4.5                         # every point is kept: 20 000 points on 16 pixels


def test_host_checks_of_dvf_velodyne_depth():
    """Every check returns DVF_ERR_INVALID_ARG before anything is launched: the pointers are fake and never dereferenced."""
    from dvf import lib as L
    assert "dvf_velodyne_depth" in L.SIGNATURES
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    good = dict(points=fake, offsets=fake, proj=fake, depth=fake, B=2, H=8, W=16, total=10, flags=0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.dvf_velodyne_depth(a["points"], a["offsets"], a["proj"], a["depth"], a["B"], a["H"], a["W"], a["total"],
                                      a["flags"], None)

    bad = [dict(points=None), dict(offsets=None), dict(proj=None), dict(depth=None), dict(points=None, total=1), dict(B=0),
           dict(B=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1), dict(total=-1), dict(B=4, H=32768, W=16384),
           dict(B=1, H=65536, W=32768), dict(flags=2), dict(flags=3), dict(flags=0x80000000),
           dict(points=ctypes.c_void_p(0x1004))]
    for kw in bad:
        assert call(**kw) == -1, kw


def _write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def test_read_calib_file(tmp_path):
    from dvf.velodyne import read_calib_file
    cam, velo = V.calib_texts()
    _write(str(tmp_path / "c.txt"), cam)
    got = read_calib_file(str(tmp_path / "c.txt"))
    assert got["calib_time"] == "09-Jan-2012 13:57:47"
    assert got["corner_dist"].dtype == np.float64 and got["corner_dist"].tolist() == [9.95e-02]
    assert got["S_02"].tolist() == [1392.0, 512.0]
    assert got["R_rect_00"].tolist() == V.written(V.R_RECT_00)
    assert got["P_rect_02"].shape == (12,) and got["P_rect_03"].tolist() == V.written(V.scaled(V.P_RECT_03).ravel())


@pytest.mark.parametrize("in_drive", [False, True])
@pytest.mark.parametrize("cam", [2, 3])
def test_velo_to_image_at_both_calibration_locations(tmp_path, in_drive, cam):
    from dvf.velodyne import find_calib_dir, velo_to_image
    root, drive = str(tmp_path), V.DRIVES[0]
    where = os.path.join(root, V.DATE, drive, "calib") if in_drive else os.path.join(root, V.DATE)
    V.write_calib(where)
    assert find_calib_dir(root, V.DATE, drive) == where
    got = velo_to_image(where, cam)
    assert got.dtype == np.float64 and got.shape == (3, 4)
    want = V.tree_proj(cam)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want).max())
    assert not np.allclose(V.tree_proj(2), V.tree_proj(3))
    with pytest.raises(ValueError, match="cam"):
        velo_to_image(where, 1)


def test_missing_calibration_names_both_locations(tmp_path):
    from dvf.velodyne import find_calib_dir
    with pytest.raises(FileNotFoundError, match="calib_cam_to_cam.txt") as e:
        find_calib_dir(str(tmp_path), V.DATE, V.DRIVES[0])
    assert os.path.join(str(tmp_path), V.DATE, V.DRIVES[0], "calib") in str(e.value)


def test_kitti_raw_depth_set(tmp_path, capsys):
    from dataset import kitti_raw_depth_set
    root = str(tmp_path / "raw")
    split = V.make_raw_tree(root)
    # a listed frame without an image: reported and skipped
    with open(split, "a") as f:
        f.write(f"{V.DATE}/{V.DRIVES[1]}/image_02/data/0000000099.png x y\n")
    ds = kitti_raw_depth_set(root, split, 64, 208)
    absent = os.path.join(root, V.DATE, V.DRIVES[1], "image_02", "data", "0000000099.png")
    assert f"{absent} missing" in capsys.readouterr().out and ds.missing == [absent]
    assert len(ds) == 4 and ds.shapes == [f[1] for f in V.RAW_TREE_FRAMES]
    assert ds.stems == [V.DRIVES[0] + "_0000000005", V.DRIVES[0] + "_0000000007", V.DRIVES[1] + "_0000000000",
                        V.DRIVES[1] + "_0000000013"]
    frame, points, proj = ds[2]
    assert frame.dtype == torch.float32 and tuple(frame.shape) == (3, 64, 208) and float(frame.max()) > 1.5
    assert points.dtype == torch.float32 and np.array_equal(points.numpy(), V.tree_points("1/0000000000", 3000))
    assert proj.dtype == torch.float64 and np.all(np.abs(proj.numpy() - V.tree_proj()) <= 1e-12 * np.abs(V.tree_proj()).max())
    assert ds.batches(2) == [[0, 1], [2, 3]] and ds.batches(3) == [[0, 1], [2, 3]] and ds.batches(1) == [[0], [1], [2], [3]]
    seen = 0
    for batch in ds.loader(4):
        frames, pts, offsets, projs, size = batch
        b = frames.shape[0]
        assert len(batch) == 5 and tuple(size) in ((37, 122), (40, 130))
        assert all(ds.shapes[seen + i] == tuple(size) for i in range(b))            # a batch never mixes sizes
        assert offsets.dtype == torch.int32 and offsets.numel() == b + 1 and int(offsets[0]) == 0
        assert bool((offsets[1:] >= offsets[:-1]).all()) and int(offsets[-1]) == pts.shape[0]
        assert pts.dtype == torch.float32 and pts.shape[1] == 4 and projs.dtype == torch.float64 and tuple(projs.shape) == (b, 3, 4)
        for i in range(b):
            assert torch.equal(pts[int(offsets[i]):int(offsets[i + 1])], ds[seen + i][1])
        seen += b
    assert seen == 4
    # the right camera: the same sweeps, another matrix; its images do not exist in this tree
    assert len(kitti_raw_depth_set(root, split, 64, 208, cam=3)) == 0
    with pytest.raises(ValueError, match="cam"):
        kitti_raw_depth_set(root, split, 64, 208, cam=1)


def test_kitti_raw_depth_set_needs_the_sweep_and_the_calibration(tmp_path):
    from dataset import kitti_raw_depth_set
    root = str(tmp_path / "raw")
    split = V.make_raw_tree(root, calib_in_drive=True)
    assert len(kitti_raw_depth_set(root, split, 64, 208)) == 4                        # calibration found next to the drive
    sweep = os.path.join(root, V.DATE, V.DRIVES[0], "velodyne_points", "data", "0000000007.bin")
    os.rename(sweep, sweep + ".away")
    with pytest.raises(FileNotFoundError) as e:
        kitti_raw_depth_set(root, split, 64, 208)
    assert sweep in str(e.value)
    os.rename(sweep + ".away", sweep)
    calib = os.path.join(root, V.DATE, V.DRIVES[1], "calib", "calib_velo_to_cam.txt")
    os.remove(calib)
    with pytest.raises(FileNotFoundError) as e:
        kitti_raw_depth_set(root, split, 64, 208)
    assert os.path.join(root, V.DATE, V.DRIVES[1], "calib") in str(e.value)


def test_depth_maps_refuses_cpu_tensors():
    from dvf.velodyne import depth_maps
    points, offsets, proj = V.batch_case()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        depth_maps(torch.from_numpy(points), torch.from_numpy(offsets), torch.from_numpy(proj), *V.SHAPE)


class _ArgumentsAccepted(Exception):
    """Raised in place of the first GPU step: the command line was parsed and passed its checks."""


def _accepted():
    raise _ArgumentsAccepted()


def test_depth_eval_takes_exactly_one_ground_truth_source(monkeypatch, capsys):
    """--val-depth-root or --kitti-raw-root, not both, not neither; the raw options need the raw root.  Each refusal is
    argparse's exit 2 with the check's own message; an accepted command line reaches the first GPU step."""
    import depth_eval
    from dvf import cli
    monkeypatch.setattr(cli, "require_gpu", _accepted)
    ck = ["--pretrained-disp", "x"]
    refused = [(ck, "exactly one of --val-depth-root and --kitti-raw-root"),
               (ck + ["--val-depth-root", "a", "--kitti-raw-root", "b", "--split", "s"], "exactly one of --val-depth-root and --kitti-raw-root"),
               (ck + ["--kitti-raw-root", "b"], "--kitti-raw-root needs --split"),
               (ck + ["--val-depth-root", "a", "--export-depth-root", "o"], "need --kitti-raw-root"),
               (ck + ["--val-depth-root", "a", "--split", "s"], "need --kitti-raw-root"),
               (ck + ["--val-depth-root", "a", "--velodyne-depth"], "need --kitti-raw-root"),
               (ck + ["--kitti-raw-root", "b", "--split", "s", "--cam", "1"], "--cam")]
    for argv, message in refused:
        with pytest.raises(SystemExit) as e:
            depth_eval.main(argv)
        assert e.value.code == 2 and message in capsys.readouterr().err, argv
    for argv in (ck + ["--val-depth-root", "a"], ck + ["--kitti-raw-root", "b", "--split", "s"],
                 ck + ["--kitti-raw-root", "b", "--split", "s", "--cam", "3", "--velodyne-depth", "--export-depth-root", "o"]):
        with pytest.raises(_ArgumentsAccepted):
            depth_eval.main(argv)


def test_train_takes_one_depth_validation_source(monkeypatch, capsys):
    """train.py: --val-kitti-raw-root excludes --val-depth-root and goes with --val-split."""
    import sys
    import train
    from dvf import cli
    monkeypatch.setattr(cli, "init_distributed", _accepted)
    refused = [(["--val-depth-root", "a", "--val-kitti-raw-root", "b", "--val-split", "s"], "exclude each other"),
               (["--val-kitti-raw-root", "b"], "go together"), (["--val-split", "s"], "go together"),
               (["--val-kitti-raw-root", "b", "--val-split", "s", "--val-cam", "1"], "--val-cam")]
    for argv, message in refused:
        monkeypatch.setattr(sys, "argv", ["train.py"] + argv)
        with pytest.raises(SystemExit) as e:
            train.main()
        assert e.value.code == 2 and message in capsys.readouterr().err, argv
    for argv in (["--val-depth-root", "a"], ["--val-kitti-raw-root", "b", "--val-split", "s", "--val-cam", "3"], []):
        monkeypatch.setattr(sys, "argv", ["train.py"] + argv)
        with pytest.raises(_ArgumentsAccepted):
            train.main()
