"""train.py --val-depth-root and depth_eval.py's command line on a small validation tree (pattern of
test_gpu_cli.py::test_train_with_validate_on_odometry_tree): the Depth line per epoch, the depth checkpoint saved on the best
abs_rel, and the printed numbers against the test-side definition applied to the saved network's predictions."""
import os
import subprocess
import sys

import pytest
import torch

import depth_metrics_ref as R
from conftest import PKG, ROOT, rel_err
from test_depth_metrics import _make_depth_tree

pytestmark = pytest.mark.gpu
NAMES = R.COLUMNS[:8]


def _depth_lines(stdout):
    out = []
    for line in stdout.splitlines():
        if line.startswith("Depth: "):
            w = line.split()
            out.append({w[i]: float(w[i + 1]) for i in range(1, 17, 2)})
    return out


def _restated(ckpt, root, h, w, batch):
    """Mean rows of the restatement over the tree, from the predictions of the network in the saved state."""
    from DispNetS import DispNetS
    from dataset import depth_validation_set
    from dvf import cli
    from dvf import lib as L
    net = DispNetS()
    cli.load_pretrained(net, ckpt)
    net.to("cuda").eval()
    total, count = torch.zeros(8, dtype=torch.float64), 0
    with torch.no_grad():
        for img, gt in depth_validation_set(root, h, w).loader(batch):
            disp = net(img.cuda())[0].contiguous()
            b, _, dh, dw = disp.shape
            hg, wg = gt.shape[1:]
            up = torch.empty(b, hg, wg, device="cuda")
            L.check(L.lib().dvf_resize_bilinear_fwd(L.dev(disp), L.dev(up), b, dh, dw, hg, wg, dh / hg, dw / wg, L.stream()), "resize")
            rows, _ = R.rows(gt, (1.0 / up).cpu(), crop=True)
            keep = rows[:, 8] > 0
            total += rows[keep, :8].sum(0)
            count += int(keep.sum())
    return total / max(count, 1)


def test_train_validates_depth_and_depth_eval_agrees(tmp_path):
    h, w = 64, 208
    root = _make_depth_tree(str(tmp_path / "val"), [(37, 122), (37, 122), (40, 130), (40, 130)], h=h, w=w)
    out = tmp_path / "ckpt"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "-b", "2", "--epochs", "2", "--steps-per-epoch", "2", "--height", str(h),
           "--width", str(w), "--val-depth-root", root, "--output-dir", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = _depth_lines(res.stdout)
    assert len(lines) == 2 and all(set(l) == set(NAMES) for l in lines), res.stdout[-2000:]
    assert all(l["abs_rel"] == l["abs_rel"] and l["abs_rel"] > 0 for l in lines)
    ckpt = os.path.join(out, "best_depth_checkpoint.pth.tar")
    assert os.path.exists(ckpt) and os.path.exists(os.path.join(out, "best_vo_checkpoint.pth.tar"))
    best = min(lines, key=lambda l: l["abs_rel"])          # the checkpoint holds the epoch of the best abs_rel
    want = _restated(ckpt, root, h, w, 2)
    for i, k in enumerate(NAMES):
        assert rel_err(best[k], want[i]) < 1e-4, (k, best[k], float(want[i]))
    ev = subprocess.run([sys.executable, os.path.join(PKG, "depth_eval.py"), "--pretrained-disp", ckpt, "--val-depth-root", root,
                         "--height", str(h), "--width", str(w), "-b", "2"], capture_output=True, text=True, timeout=600, env=env)
    assert ev.returncode == 0, ev.stderr[-2000:]
    again = _depth_lines(ev.stdout)
    assert len(again) == 1
    for k in NAMES:
        assert rel_err(again[0][k], best[k]) < 1e-6, (k, again[0][k], best[k])
