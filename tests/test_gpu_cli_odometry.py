"""train.py --val-odometry and odometry_eval.py's command line on a small KITTI-odometry-shaped tree (pattern of
test_gpu_cli_depth_val.py): the Odometry line per epoch, the checkpoint saved on the best t_err, and odometry_eval.py printing
the best epoch's numbers for that file."""
import os
import subprocess
import sys

import numpy as np
import pytest

import odometry_ref as R
from conftest import PKG, ROOT, rel_err

pytestmark = pytest.mark.gpu
H, W = 64, 208


def _odometry_lines(stdout):
    out = []
    for line in stdout.splitlines():
        if line.startswith("Odometry: "):
            w = line.split()
            out.append({"t_err": float(w[2]), "r_err": float(w[4]), "segments": int(w[6]), "seq": w[8] if "seq" in w else None,
                        "best": "[BEST:True]" in line})
    return out


def _train(root, out, *extra, epochs="2", steps="2"):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "-b", "2", "--epochs", epochs, "--steps-per-epoch", steps, "--height", str(H),
           "--width", str(W), "--val-root", root, "--test-sequences", "00", "--output-dir", str(out)] + list(extra)
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout, env


def test_train_validates_odometry_and_odometry_eval_agrees(tmp_path):
    root = R.make_tree(tmp_path / "odo", R.end_to_end_gt(), h=H, w=W)
    out = tmp_path / "ckpt"
    stdout, env = _train(root, out, "--val-odometry")
    lines = _odometry_lines(stdout)
    assert len(lines) == 2 and all(l["seq"] is None and l["segments"] == 1 for l in lines), stdout[-2000:]
    assert all(l["t_err"] == l["t_err"] and l["t_err"] > 0 and l["r_err"] > 0 for l in lines) and lines[0]["best"]
    assert len([l for l in stdout.splitlines() if l.startswith("Test set: Average loss:")]) == 2      # validate() still runs
    ckpt = os.path.join(out, "best_odometry_checkpoint.pth.tar")
    assert os.path.exists(ckpt)
    assert os.path.exists(os.path.join(out, "best_vo_checkpoint.pth.tar")) and os.path.exists(os.path.join(out, "best_depth_checkpoint.pth.tar"))
    best = lines[1] if lines[1]["best"] else lines[0]              # the checkpoint holds the epoch of the best t_err
    assert lines[1]["best"] == (lines[1]["t_err"] < lines[0]["t_err"])
    poses = tmp_path / "poses_out"
    ev = subprocess.run([sys.executable, os.path.join(PKG, "odometry_eval.py"), "--pretrained-pose", ckpt, "--val-root", root,
                         "--sequences", "00", "--height", str(H), "--width", str(W), "-b", "2", "--output-dir", str(poses)],
                        capture_output=True, text=True, timeout=600, env=env)
    assert ev.returncode == 0, ev.stderr[-2000:]
    again = _odometry_lines(ev.stdout)
    assert len(again) == 2 and again[0]["seq"] == "00" and again[1]["seq"] is None
    for line in again:
        assert line["segments"] == 1
        for k in ("t_err", "r_err"):
            assert rel_err(np.float64(line[k]), np.float64(best[k])) < 1e-6, (k, line[k], best[k])
    with open(poses / "00.txt") as f:
        assert len([l for l in f if len(l.split()) == 12]) == 20


def test_train_without_the_flag_prints_and_writes_nothing_new(tmp_path):
    root = R.make_tree(tmp_path / "odo", R.end_to_end_gt(), h=H, w=W)
    out = tmp_path / "ckpt"
    stdout, _ = _train(root, out, epochs="1", steps="1")
    assert "Odometry:" not in stdout and "Test set: Average loss:" in stdout
    assert sorted(os.listdir(out)) == ["best_depth_checkpoint.pth.tar", "best_vo_checkpoint.pth.tar"]
