"""Host-side half of the device odometry evaluation (csrc/odometry.hip, dvf/odometry.py): the argument checks of the two entry
points, dataset.odometry_sequences, train.py's flag check, and the INPUT CONDITIONS under which tests/test_gpu_odometry.py may
compare at its tolerance -- asserted here, on the reference alone, so that no GPU result can move them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import odometry_eval as oe
import odometry_ref as R
from conftest import PKG, ROOT, rel_err
from dvf import lib as L

FAKE = ctypes.c_void_p(0x1000)          # never dereferenced: every call below fails its host-side check first


def test_pose_chain_rejects_bad_arguments_without_touching_the_gpu():
    lib = L.lib()
    ok = L.int_array([0, 4])
    assert lib.dvf_pose_chain(None, ok, 1, FAKE, None) == -1
    assert lib.dvf_pose_chain(FAKE, None, 1, FAKE, None) == -1
    assert lib.dvf_pose_chain(FAKE, ok, 1, None, None) == -1
    assert lib.dvf_pose_chain(FAKE, ok, 0, FAKE, None) == -1                                   # S = 0
    assert lib.dvf_pose_chain(FAKE, L.int_array(list(range(34))), 33, FAKE, None) == -1        # S = 33
    assert lib.dvf_pose_chain(FAKE, L.int_array([0, 5, 3]), 2, FAKE, None) == -1               # decreasing
    assert lib.dvf_pose_chain(FAKE, L.int_array([1, 5]), 1, FAKE, None) == -1                  # offsets[0] != 0
    assert lib.dvf_pose_chain(FAKE, L.int_array([0, 1 << 24]), 1, FAKE, None) == -1            # N >= 2^24


def test_odometry_errors_rejects_bad_arguments_without_touching_the_gpu():
    lib = L.lib()
    assert lib.dvf_odometry_errors_ws_doubles(0) == 0 and lib.dvf_odometry_errors_ws_doubles(4541) >= 4541
    assert lib.dvf_odometry_errors(FAKE, FAKE, 0, FAKE, FAKE, 0, FAKE, 100, None) == -1        # n = 0
    assert lib.dvf_odometry_errors(None, FAKE, 20, FAKE, FAKE, 0, FAKE, 100, None) == -1
    assert lib.dvf_odometry_errors(FAKE, None, 20, FAKE, FAKE, 0, FAKE, 100, None) == -1
    assert lib.dvf_odometry_errors(FAKE, FAKE, 20, None, FAKE, 0, FAKE, 100, None) == -1       # n > 9 has rows
    assert lib.dvf_odometry_errors(FAKE, FAKE, 20, FAKE, None, 0, FAKE, 100, None) == -1
    assert lib.dvf_odometry_errors(FAKE, FAKE, 20, FAKE, FAKE, 0, None, 100, None) == -1
    assert lib.dvf_odometry_errors(FAKE, FAKE, 20, FAKE, FAKE, 0, FAKE, 19, None) == -1        # workspace too small


def test_public_functions_refuse_cpu_tensors():
    import torch
    from dvf import odometry
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        odometry.chain_poses(torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        odometry.sequence_errors(torch.zeros(20, 3, 4, dtype=torch.float64), torch.zeros(20, 3, 4, dtype=torch.float64))
    assert odometry.n_starts(9) == 0 and odometry.n_starts(10) == 1 and odometry.n_starts(20) == 2 and odometry.n_starts(4541) == 454


def test_odometry_sequences_are_ordered_pairs_with_float64_poses(tmp_path):
    import dataset
    gt = R.curved(7, 5)
    R.make_tree(tmp_path, gt, seq="04", h=20, w=60)
    R.make_tree(tmp_path, R.curved(5, 6), seq="02", h=20, w=60)
    seqs = dataset.odometry_sequences(str(tmp_path), ["04", "02"], 16, 48)
    assert [s[0] for s in seqs] == ["02", "04"]                      # directory order, as read_scene_data
    name, pairs, poses = seqs[1]
    assert len(pairs) == 6 and poses.dtype == np.float64 and poses.shape == (7, 3, 4)
    assert np.array_equal(poses, gt[:, :3])                          # the file's numbers, not their float32 rounding
    assert len(seqs[0][1]) == 4 and seqs[0][2].shape == (5, 3, 4)
    for i, sample in enumerate(pairs.samples):                       # pair i = frames (i, i + 1), unshuffled
        assert [os.path.basename(p) for p in sample["imgs"]] == [f"{i:06d}.png", f"{i + 1:06d}.png"]
    data, pose = pairs[2]                                            # validate()'s layout: later frame first, 4x4 relative pose
    assert tuple(data.shape) == (6, 16, 48) and tuple(pose.shape) == (4, 4)
    assert np.allclose(pose.numpy(), np.linalg.inv(gt[2]) @ gt[3], atol=1e-5)
    assert dataset.odometry_sequences(str(tmp_path), ["09"], 16, 48) == []


def test_val_odometry_without_val_root_is_refused():
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--val-odometry"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 2 and "--val-odometry needs --val-root" in r.stderr, r.stderr[-2000:]


def test_importing_odometry_eval_stays_free_of_torch():
    code = "import sys, odometry_eval; assert 'torch' not in sys.modules and callable(odometry_eval.main)"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, PYTHONPATH=PKG))
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("name", R.ERROR_CASES + ("end_to_end",))
def test_input_conditions_of_the_gpu_comparisons(name):
    """A path length summed in another order differs by ~1e-12 relative at most; that must not be able to move a segment's end.
    Either every step is a whole number (sums exact in any order, ties included) or no frame lies within 1e-6 * length of a
    threshold.  The cases compared at a relative tolerance have a rotation error >= 1e-3 rad in every reference row, where the
    arccos of the definition is well conditioned."""
    gt, res = (R.end_to_end_gt(),) * 2 if name == "end_to_end" else R.error_case(name)
    assert R.exact_distances(gt) or R.threshold_margin(gt) > 1e-6, R.threshold_margin(gt)
    if name in R.RELATIVE_CASES:
        rows = np.array(oe.sequence_errors(R.as_dict(gt), R.as_dict(res)))
        assert len(rows) > 100
        assert float((rows[:, 1] * rows[:, 3]).min()) >= 1e-3
    if name == "end_to_end":
        rows = oe.sequence_errors(R.as_dict(gt), R.as_dict(gt))
        assert len(rows) == 1 and rows[0][0] == 9 and rows[0][3] == 100      # the one segment the tree is built to have


def test_chain_generator_catches_an_operand_swap():
    for n in (255, 1000, 4541):
        rel = R.chain_input(n)
        assert rel_err(R.world_reversed(rel), R.world_of(rel)) > 1e-2


def test_tree_order_product_agrees_with_the_sequential_chain():
    """Support for the 1e-9 tolerance of the GPU chain test: re-associating the fp64 product of 4541 rigid transforms moves it
    by ~N * 2^-53, orders of magnitude below 1e-9 (and an fp32 accumulation would sit orders of magnitude above)."""
    rel = R.chain_input(4541).astype(np.float64)
    want = R.world_of(rel)[1:]
    err = rel_err(R.tree_prefix(rel), want)
    print("tree-order vs sequential, n = 4541: rel_err", err)
    assert err < 1e-9
