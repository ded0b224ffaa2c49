"""dvf.validation.validate_odometry(align=...), odometry_eval.py --align and train.py --val-odometry-align end to end on the small
KITTI-odometry-shaped tree of tests/test_gpu_odometry.py (64x208, 20 frames), its ground truth a chained walk of 12 m steps with
a slow turn (align_ref.end_to_end_gt: positions that are not collinear; the straight line of odometry_ref.end_to_end_gt has no
unique alignment rotation, its sv[1] and sv[2] are exactly 0).
Every new field is the numpy definition (odometry_eval.py) applied to the returned chain, to 1e-9."""
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import align_ref as A
import odometry_eval as oe
import odometry_ref as R
from conftest import PKG, ROOT, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-9
H, W, N = 64, 208, 20


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import dataset
    gt = A.end_to_end_gt(N)
    root = R.make_tree(tmp_path_factory.mktemp("odo_align"), gt, h=H, w=W)
    return gt, root, dataset.odometry_sequences(root, ["00"], H, W)


@pytest.fixture(scope="module")
def net():
    from PoseExpNet_sfm import PoseExpNet
    torch.manual_seed(0)
    net = PoseExpNet(nb_ref_imgs=2, output_exp=True)
    net.init_weights()
    return net.to(DEV).eval()


def _close(name, got, want):
    err = abs(got - want) / abs(want) if want != 0.0 else abs(got)
    print(f"end to end: {name} {got!r} rel_err {err:.3e}")
    assert err < TOL, (name, got, want)


def test_validate_odometry_aligned_fields_are_the_definition_of_the_returned_chain(tree, net, tmp_path):
    from dvf import validation
    gt, _, seqs = tree
    out = validation.validate_odometry(net, seqs, torch.device(DEV, 0), 4, align="7dof", keep=True, output_dir=str(tmp_path))
    world = out["world"].cpu().numpy()
    c, rot, t, sv = oe.trajectory_alignment(gt, world, "7dof")
    assert (sv[1] + sv[2]) / sv[0] >= A.CONDITION                        # the chain of a random network is not collinear
    want = oe.apply_alignment(world, c, rot, t)
    err = rel_err(out["aligned"], want)
    print(f"end to end: aligned rel_err {err:.3e}")
    assert out["aligned"].shape == out["world"].shape and err < TOL
    per = out["per_sequence"]["00"]
    assert per["align"] == out["align"] == "7dof"
    _close("scale", per["scale"], c)
    assert rel_err(np.array(per["singular_values"]), sv) < TOL
    ate, rpe_t, rpe_r = oe.trajectory_errors(gt, want)
    rows = oe.snippet_errors(gt, want)
    mean, std, re = A.snippet_stats(rows)
    deg = 180.0 / math.pi
    for name, w in (("ate", ate), ("rpe_trans", rpe_t), ("rpe_rot", rpe_r * deg), ("snippet_ate", mean), ("snippet_ate_std", std),
                    ("snippet_re", re * deg)):
        _close(name, per[name], w)
    assert per["snippets"] == out["snippets"] == len(rows) == N - 4
    for name in ("scale", "ate", "rpe_trans", "rpe_rot", "snippet_ate", "snippet_ate_std", "snippet_re"):
        assert out[name] == per[name]                                    # one sequence: the mean over sequences is its value
    seg = oe.sequence_errors(R.as_dict(gt), R.as_dict(oe._as44(want)))
    t_err, r_err = oe.overall_error(seg)
    assert out["segments"] == len(seg) == 1
    _close("t_err", out["t_err"], 100.0 * t_err)
    # (r_err through arccos at ~1e-2 rad: the bound of tests/test_gpu_odometry.py)
    _close("r_err", out["r_err"], r_err * deg * 100.0)
    line = validation.format_trajectory(out)
    assert line.startswith("Trajectory: align 7dof scale ") and line.endswith(f"snippets {N - 4}")
    assert validation.format_trajectory(per, "00").endswith(f"snippets {N - 4} seq 00")
    for name, key in (("00.txt", "world"), ("00_aligned.txt", "aligned")):
        back = oe.load_poses(os.path.join(tmp_path, name))
        assert np.array_equal(np.stack([back[i] for i in range(N)])[:, :3], out[key].cpu().numpy())
    raw = validation.validate_odometry(net, seqs, torch.device(DEV, 0), 4)
    assert raw["t_err"] != out["t_err"]                                  # the alignment changed the score


def test_validate_odometry_synchronises_once_before_the_file_writing():
    from dvf import validation
    body = inspect.getsource(validation.validate_odometry)
    head = (inspect.getsource(validation.relative_poses) + inspect.getsource(validation.score_trajectories) +
            body[:body.index("write_trajectories(")])
    assert head.count(".tolist()") == 1 and ".cpu()" not in head and ".item()" not in head and "synchronize" not in head


def test_without_align_the_dict_has_todays_keys_and_none_aligns_nothing(tree, net):
    from dvf import validation
    gt, _, seqs = tree
    out = validation.validate_odometry(net, seqs, torch.device(DEV, 0), 4, keep=True)
    assert sorted(out) == ["offsets", "per_sequence", "r_err", "rel", "segments", "t_err", "world"]
    assert sorted(out["per_sequence"]["00"]) == ["path_length", "r_err", "segments", "t_err"]
    same = validation.validate_odometry(net, seqs, torch.device(DEV, 0), 4, align="none", keep=True)
    assert same["t_err"] == out["t_err"] and same["r_err"] == out["r_err"] and same["per_sequence"]["00"]["scale"] == 1.0
    assert torch.equal(same["aligned"], same["world"]) and torch.equal(same["world"], out["world"])
    with pytest.raises(ValueError):
        validation.validate_odometry(net, seqs, torch.device(DEV, 0), 4, align="sim3")


def test_odometry_eval_prints_trajectory_lines_only_with_align(tree, net, tmp_path, capsys):
    gt, root, _ = tree
    ckpt = str(tmp_path / "pose.pth.tar")
    torch.save({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, ckpt)
    argv = ["--pretrained-pose", ckpt, "--val-root", root, "--sequences", "00", "--height", str(H), "--width", str(W), "-b", "4"]
    plain_dir, align_dir = str(tmp_path / "plain"), str(tmp_path / "aligned")
    oe.main(argv + ["--output-dir", plain_dir])
    plain = capsys.readouterr().out
    assert "Trajectory:" not in plain and len([l for l in plain.splitlines() if l.startswith("Odometry: ")]) == 2
    assert sorted(os.listdir(plain_dir)) == ["00.txt"]
    metrics = oe.main(argv + ["--output-dir", align_dir, "--align", "scale"])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith(("Odometry:", "Trajectory:"))]
    assert [l.split()[0] for l in lines] == ["Odometry:", "Trajectory:", "Odometry:", "Trajectory:"]
    assert lines[1].startswith("Trajectory: align scale scale ") and lines[1].endswith(" seq 00") and "seq" not in lines[3]
    assert lines[1] == f"{lines[3]} seq 00"
    assert sorted(os.listdir(align_dir)) == ["00.txt", "00_aligned.txt"]
    with open(os.path.join(plain_dir, "00.txt")) as f, open(os.path.join(align_dir, "00.txt")) as g:
        assert f.read() == g.read()                                      # <seq>.txt stays the raw chain
    back = oe.load_poses(os.path.join(align_dir, "00_aligned.txt"))
    world = np.stack([oe.load_poses(os.path.join(align_dir, "00.txt"))[i] for i in range(N)])
    c = metrics["per_sequence"]["00"]["scale"]
    assert rel_err(np.stack([back[i] for i in range(N)]), oe.apply_alignment(world, c, np.eye(3), np.zeros(3))) < TOL
    _close("scale", c, oe.trajectory_alignment(gt, world, "scale")[0])


def test_train_prints_the_trajectory_line_and_saves_on_the_aligned_t_err(tree, tmp_path):
    _, root, _ = tree
    out = tmp_path / "ckpt"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "-b", "2", "--epochs", "1", "--steps-per-epoch", "1", "--height", str(H),
           "--width", str(W), "--val-root", root, "--test-sequences", "00", "--output-dir", str(out), "--val-odometry",
           "--val-odometry-align", "scale"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith(("Odometry:", "Trajectory:"))]
    assert [l.split()[0] for l in lines] == ["Odometry:", "Trajectory:"] and "[BEST:True]" in lines[0]
    words = lines[1].split()
    assert words[1:3] == ["align", "scale"] and words[3] == "scale" and math.isfinite(float(words[4])) and words[-2:] == ["snippets", str(N - 4)]
    assert float(lines[0].split()[2]) > 0                                # the aligned t_err is a number, not NaN
    assert os.path.exists(out / "best_odometry_checkpoint.pth.tar")


def test_train_refuses_the_align_flag_without_val_odometry(tree, tmp_path):
    _, root, _ = tree
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "-b", "2", "--epochs", "1", "--steps-per-epoch", "1", "--height", str(H),
           "--width", str(W), "--val-root", root, "--test-sequences", "00", "--output-dir", str(tmp_path / "ckpt"),
           "--val-odometry-align", "7dof"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 2 and "--val-odometry-align needs --val-odometry" in res.stderr
    assert not os.path.exists(tmp_path / "ckpt")
