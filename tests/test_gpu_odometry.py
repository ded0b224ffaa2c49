"""dvf_pose_chain / dvf_odometry_errors / dvf.validation.validate_odometry on the GPU against the numpy definition
(odometry_eval.py: se3_cam2world, sequence_errors, overall_error; inputs from tests/odometry_ref.py).

Bound: conftest.rel_err < 1e-9 for world poses and for the t_err/len, r_err/len and speed columns; first, length, the valid
flag and the row count EQUAL the definition.  The bound is derived: a re-associated fp64 product of N <= 4541 rigid transforms
errs by about N * 2^-53 ~ 1e-12 relative (tests/test_odometry_device.py measures the numpy tree-order product), an fp32
accumulation by about N * 6e-8 ~ 3e-4; 1e-9 separates the two by orders of magnitude on both sides.  The input conditions under
which the comparison is fair (no frame near a segment threshold, rotation errors >= 1e-3 rad where compared relatively) are
asserted on the reference alone in tests/test_odometry_device.py.  Every case prints its figure (pytest -s).
Measured worst values over the cases of this file: world poses 5.2e-15 (chain, n = 4541; 1.2e-15 at n = 1000 and in the ragged
call), r_err/len 9.9e-13 (curved, n = 1500: the arccos of both sides at angles down to 1e-2 rad), t_err/len 3.6e-14, speed 0,
the overall means 3.1e-15; end to end: world 6.7e-16, t_err 5.3e-16, r_err 2.9e-13."""
import math
import os

import numpy as np
import pytest
import torch

import odometry_eval as oe
import odometry_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-9


def _bits(x):
    return x.contiguous().view(torch.int64)


def _chain(rel32, offsets=None):
    from dvf.odometry import chain_poses
    rel = torch.from_numpy(np.ascontiguousarray(rel32)).to(DEV)
    world = chain_poses(rel, offsets)
    again = chain_poses(rel, offsets)
    torch.cuda.synchronize()
    assert world.dtype == torch.float64 and _bits(world).equal(_bits(again)), "a second run differs"
    return world.cpu().numpy()


@pytest.mark.parametrize("n", R.CHAIN_SIZES)
def test_chain_against_se3_cam2world(n):
    rel = R.chain_input(n)
    want = R.world_of(rel)[:, :3]
    got = _chain(rel)
    assert got.shape == (n + 1, 3, 4)
    assert np.array_equal(got[0], np.eye(4)[:3])
    err = rel_err(got, want)
    print(f"chain n={n}: rel_err {err:.3e}")
    assert err < TOL
    if n >= 255:                                   # the data would show a left/right swap: it is an O(1) error
        assert rel_err(R.world_reversed(rel)[:, :3], want) > 1e-2


def test_chain_ragged_sequences_land_at_offset_plus_index():
    offsets = list(R.RAGGED_OFFSETS)
    rel = R.chain_input(offsets[-1], seed=9)
    got = _chain(rel, offsets)
    assert got.shape == (offsets[-1] + 3, 3, 4)
    for s in range(3):
        want = R.world_of(rel[offsets[s]:offsets[s + 1]])[:, :3]
        part = got[offsets[s] + s:offsets[s + 1] + s + 1]
        assert np.array_equal(part[0], np.eye(4)[:3])
        err = rel_err(part, want)
        print(f"ragged sequence {s} ({len(want) - 1} poses): rel_err {err:.3e}")
        assert err < TOL


def _errors(gt, res, summary=None):
    from dvf.odometry import sequence_errors
    g = torch.from_numpy(np.ascontiguousarray(gt[:, :3])).to(DEV)
    r = torch.from_numpy(np.ascontiguousarray(res[:, :3])).to(DEV)
    return sequence_errors(g, r, summary)


def _check_rows(rows, gt, res, tag):
    """Device rows against the definition's list; returns the definition's rows."""
    rows = rows.cpu().numpy()
    want = np.array(oe.sequence_errors(R.as_dict(gt), R.as_dict(res)), dtype=np.float64).reshape(-1, 5)
    n = len(gt)
    assert rows.shape == (len(range(9, n, 10)) * 8, 6)
    valid = rows[:, 5] == 1.0
    assert np.all(rows[~valid] == 0.0)
    got = rows[valid]
    assert len(got) == len(want), (tag, len(got), len(want))
    idx = np.nonzero(valid)[0]
    assert np.array_equal(got[:, 0], 9 + 10 * (idx // 8)) and np.array_equal(got[:, 3], 100.0 * (idx % 8 + 1))   # start-major
    if len(want):
        assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 3], want[:, 3])
        for col, name in ((1, "r_err/len"), (2, "t_err/len"), (4, "speed")):
            err = rel_err(got[:, col], want[:, col])
            print(f"{tag}: {name} rel_err {err:.3e}")
            assert err < TOL, (tag, name, err)
    return want


def _check_summary(summary, wants, gt_last, tag):
    from dvf.odometry import overall
    t, r = overall(summary)
    s, t, r = summary.cpu().numpy(), float(t), float(r)
    want = np.concatenate(wants) if wants else np.zeros((0, 5))
    assert s[2] == len(want)
    path = oe.trajectory_distances(R.as_dict(gt_last))[-1]
    assert abs(s[3] - path) <= 1e-12 * max(path, 1.0), (tag, s[3], path)
    wt, wr = oe.overall_error([list(x) for x in want])
    if len(want) == 0:
        assert math.isnan(t) and math.isnan(r) and math.isnan(wt) and s[0] == 0.0 and s[1] == 0.0
        return
    for name, g, w in (("t", t, wt), ("r", r, wr)):
        err = rel_err(np.float64(g), np.float64(w))             # (float64 scalars: a python float would become fp32)
        print(f"{tag}: overall {name} rel_err {err:.3e}")
        assert err < TOL, (tag, name, g, w)


@pytest.mark.parametrize("name", R.ERROR_CASES)
def test_errors_against_sequence_errors(name):
    gt, res = R.error_case(name)
    rows, summary = _errors(gt, res)
    rows2, summary2 = _errors(gt, res)
    torch.cuda.synchronize()
    assert _bits(rows).equal(_bits(rows2)) and _bits(summary).equal(_bits(summary2)), "a second run differs"
    want = _check_rows(rows, gt, res, name)
    _check_summary(summary, [want], gt, name)
    got = rows.cpu().numpy()
    n = len(gt)
    if name == "identical":                      # the known answers of test_identical_trajectories_have_zero_error
        # every segment that ends inside the sequence is valid: 1 m per frame, so (first, L) needs frame first + L + 1 <= 1199
        idx = np.arange(120 * 8)
        assert len(got) == 120 * 8 and np.array_equal(got[:, 5] == 1.0, 9 + 10 * (idx // 8) + 100 * (idx % 8 + 1) + 1 <= 1199)
        assert np.all(got[:, 2] == 0.0)
        assert float((got[:, 1] * got[:, 3]).max()) < 1e-6            # arccos near 1: sqrt(2 N eps)
        v = got[got[:, 5] == 1.0]
        assert set(v[:, 3]) == set(float(x) for x in oe.SEGMENT_LENGTHS)
        assert got[0, 0] == 9 and got[0, 3] == 100 and abs(got[0, 4] - 100 / (0.1 * 102)) < 1e-12
        assert float(np.abs(v[:, 4] - v[:, 3] / (0.1 * (v[:, 3] + 2.0))).max()) < 1e-12      # L m in L + 2 frames at 10 Hz
    elif name == "scale":                        # test_scale_drift_gives_the_analytic_translation_error
        v = got[got[:, 5] == 1.0]
        assert len(v)
        for first, r_err, t_err, length, speed, _ in v:
            frames = next(i for i in range(int(first), n) if i - first > length) - first
            assert abs(r_err) < 1e-12 and abs(t_err - 0.1 * frames / length) < 1e-9
    elif name == "yaw":                          # test_constant_yaw_drift_gives_the_analytic_rotation_error
        v = got[got[:, 5] == 1.0]
        assert len(v)
        for first, r_err, t_err, length, speed, _ in v:
            frames = next(i for i in range(int(first), n) if i - first > length) - first
            assert abs(r_err * length - R.YAW * frames) < 1e-9
    elif name.startswith("short"):
        assert len(want) == 0 and np.all(got == 0.0) and got.shape[0] == (0 if n == 9 else (8 if n < 20 else 48))


def test_two_sequences_accumulate_into_one_summary():
    a, b = (R.error_case("curved"), R.error_case("second"))
    rows_a, summary = _errors(*a)
    rows_b, same = _errors(*b, summary=summary)
    assert same is summary
    wants = [_check_rows(rows_a, *a, "first"), _check_rows(rows_b, *b, "second")]
    _check_summary(summary, wants, b[0], "accumulated")
    summary2 = _errors(*b, summary=_errors(*a)[1])[1]
    torch.cuda.synchronize()
    assert _bits(summary).equal(_bits(summary2)), "a second run differs"


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import dataset
    gt = R.end_to_end_gt()
    root = R.make_tree(tmp_path_factory.mktemp("odo"), gt)
    return gt, dataset.odometry_sequences(root, ["00"], 64, 208)


@pytest.mark.parametrize("convention", ["se3", "euler"])
def test_validate_odometry_end_to_end(tree, tmp_path, convention):
    from PoseExpNet_sfm import PoseExpNet
    from dvf import validation
    gt, seqs = tree
    assert np.array_equal(seqs[0][2], gt[:, :3])
    torch.manual_seed(0)
    net = PoseExpNet(nb_ref_imgs=2, output_exp=True)
    net.init_weights()
    net.to(DEV).train()
    out = validation.validate_odometry(net, seqs, torch.device(DEV, 0), 4, convention=convention, output_dir=str(tmp_path), keep=True)
    assert net.training                                                  # the mode is restored
    rel = out["rel"].cpu().numpy()
    assert rel.dtype == np.float32 and rel.shape == (19, 4, 4) and np.all(rel[:, 3] == np.array([0, 0, 0, 1], dtype=np.float32))
    assert float(np.abs(rel[:, :3] - np.eye(4, dtype=np.float32)[:3]).max()) > 0          # the network said something
    world = np.stack(oe.se3_cam2world(list(rel)))
    err = rel_err(out["world"], world[:, :3])
    print(f"end to end ({convention}): world rel_err {err:.3e}")
    assert out["offsets"] == [0, 19] and err < TOL
    rows = oe.sequence_errors(R.as_dict(gt), R.as_dict(world))
    t, r = oe.overall_error(rows)
    assert out["segments"] == len(rows) == 1
    for name, g, w in (("t_err", out["t_err"], 100.0 * t), ("r_err", out["r_err"], r * 180.0 / math.pi * 100.0)):
        e = rel_err(np.float64(g), np.float64(w))
        print(f"end to end ({convention}): {name} {g} rel_err {e:.3e}")
        assert e < TOL, (name, g, w)
    per = out["per_sequence"]["00"]
    assert per["segments"] == 1 and rel_err(np.float64(per["t_err"]), np.float64(out["t_err"])) < TOL and abs(per["path_length"] - 19 * 12.0) < 1e-9
    back = oe.load_poses(os.path.join(tmp_path, "00.txt"))
    assert sorted(back) == list(range(20))
    assert np.array_equal(np.stack([back[i] for i in range(20)])[:, :3], out["world"].cpu().numpy())
    other = validation.validate_odometry(net, seqs, torch.device(DEV, 0), 4, convention="euler" if convention == "se3" else "se3", keep=True)
    assert not torch.equal(other["rel"], out["rel"])                     # the two readings of the six outputs differ
