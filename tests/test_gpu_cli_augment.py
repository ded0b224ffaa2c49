"""End-to-end runs of the entry scripts with --augment: on dataset files through the default HIP-graph path (the
augmentation replaces the copies into the static input tensors, outside the captured graph) and on the synthetic stream with
a five-frame window (the ``extra_refs`` path), eager."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, PKG
from test_un_dataset import _make_tree

pytestmark = pytest.mark.gpu


def _run(script, flags, out):
    cmd = [sys.executable, os.path.join(PKG, script), "-b", "2", "--height", "64", "--width", "128", "--output-dir", str(out)] + flags
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    return [l for l in res.stdout.splitlines() if l.startswith("Train epoch")]


def _check(lines, n, out):
    assert len(lines) == n and "samples/s" in lines[0]
    for l in lines:
        total = float(l.split("total:")[1].split()[0])
        assert total == total and 0 < total < 1e6          # finite, positive
    for name in ("best_vo_checkpoint.pth.tar", "best_depth_checkpoint.pth.tar"):
        sd = torch.load(os.path.join(out, name), map_location="cpu", weights_only=True)
        assert isinstance(sd, dict) and len(sd) > 10


def test_unsupervise_augment_on_dataset_files_graph_mode(tmp_path):
    root = _make_tree(tmp_path, n=5)
    out = tmp_path / "ckpt"
    _check(_run("unsupervise.py", ["--data-root", str(root), "--augment", "--epochs", "2"], out), 2, out)


def test_train_augment_five_frame_window_synthetic(tmp_path):
    out = tmp_path / "ckpt"
    _check(_run("train.py", ["--augment", "--nb-ref-imgs", "4", "--epochs", "1", "--steps-per-epoch", "3", "--no-graph"], out), 1, out)
