"""CPU checks around the device depth metrics: the test-side definition (tests/depth_metrics_ref.py) against the reference's
own vectors and against the existing compute_errors, the threshold margins of the GPU test's cases, the validation set's
batching by ground-truth size, and the --val-depth-root flag.  No GPU call is made."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_metrics_ref as R
from conftest import PKG, ROOT, load_golden, t


def test_restatement_reproduces_the_reference_vectors():
    """metrics_compute_errors.npz was written by the reference's compute_errors: crop and full to 1e-6 (measured 7e-8)."""
    g = load_golden("metrics_compute_errors")
    for key, crop in (("crop", True), ("full", False)):
        rows, _ = R.rows(t(g["gt"]), t(g["pred"]), crop=crop)
        got = np.array(R.reference_six(rows))
        err = np.abs(got - g[key]) / np.abs(g[key])
        print(key, "max relative deviation", err.max())
        assert err.max() < 1e-6, (key, got, g[key])


@pytest.mark.parametrize("crop", [True, False])
def test_restatement_agrees_with_compute_errors(crop):
    import loss_functions_sfm as LS
    gt, pred = R.gen_case(2, 17, 257)
    rows, _ = R.rows(gt, pred, crop=crop)
    assert np.allclose(R.reference_six(rows), LS.compute_errors(gt, pred, crop=crop), rtol=1e-5, atol=1e-7)


def test_restatement_columns():
    """Hand-checked rows: the lower median of two, a zero row for an image without a valid pixel, NaN handling."""
    gt = torch.tensor([[[2.0, 4.0, 0.0, 90.0]], [[0.0, 0.0, 0.0, 0.0]], [[1.0, 2.0, 3.0, 0.0]]])
    pred = torch.tensor([[[1.0, 4.0, 5.0, 5.0]], [[1.0, 1.0, 1.0, 1.0]], [[1.0, float("nan"), 3.0, float("nan")]]])
    rows, _ = R.rows(gt, pred, crop=False)
    assert rows[0, 8] == 2 and rows[0, 9] == 2.0 and rows[0, 10] == 1.0      # lower of the two
    # scale 2: p = (2, 8): abs_diff = (0 + 4) / 2, a1 = 1/2 (ratio 1 and 2), a3 = 1/2 (2 > 1.953125)
    assert rows[0, 0] == 2.0 and rows[0, 5] == 0.5 and rows[0, 7] == 0.5
    assert float(rows[1].abs().sum()) == 0.0
    assert rows[2, 8] == 3 and rows[2, 11] == 1 and torch.isnan(rows[2, :8]).all() and rows[2, 9] == 2.0


@pytest.mark.parametrize("shape,crop,quantum", R.SMALL_CASES)
def test_small_cases_have_no_pixel_near_a_threshold(shape, crop, quantum):
    """The GPU test demands EQUAL threshold counts at the small shapes: no valid pixel's fp64 ratio may lie within 1e-6 of
    1.25^e there."""
    gt, pred = R.gen_case(*shape, quantum=quantum)
    _, near = R.rows(gt, pred, crop=crop)
    assert int(near.sum()) == 0


def _make_depth_tree(root, sizes, h=64, w=208, seed=5):
    """A depth validation tree: len(sizes) frames of (h, w) PNGs, ground truth of the given (Hg, Wg) sizes."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "image"))
    os.makedirs(os.path.join(root, "depth"))
    stems = []
    for i, (hg, wg) in enumerate(sizes):
        stem = f"{i:06d}"
        stems.append(stem)
        Image.fromarray(rng.randint(0, 256, size=(h + 6, w + 10, 3), dtype=np.uint8)).save(
            os.path.join(root, "image", stem + (".png" if i % 2 == 0 else ".jpg")))
        d = rng.uniform(0.5, 95.0, size=(hg, wg)).astype(np.float32)
        d[rng.uniform(size=(hg, wg)) < 0.6] = 0.0
        np.save(os.path.join(root, "depth", stem + ".npy"), d)
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("\n".join(stems) + "\n")
    return root


def test_validation_set_batches_by_ground_truth_size(tmp_path):
    from dataset import depth_validation_set
    sizes = [(37, 122), (37, 122), (37, 122), (40, 130), (40, 130), (37, 122)]
    ds = depth_validation_set(_make_depth_tree(str(tmp_path / "val"), sizes), 64, 208)
    assert len(ds) == 6 and ds.shapes == sizes
    assert ds.batches(2) == [[0, 1], [2], [3, 4], [5]]
    assert ds.batches(4) == [[0, 1, 2], [3, 4], [5]]
    seen = []
    for img, depth in ds.loader(2):
        assert img.dtype == torch.float32 and img.shape[1:] == (3, 64, 208) and depth.dtype == torch.float32
        assert img.shape[0] == depth.shape[0] and float(img.max()) > 1.5 and float(img.min()) >= 0.0      # 0..255 range
        seen.append(tuple(depth.shape))
    assert seen == [(2, 37, 122), (1, 37, 122), (2, 40, 130), (1, 37, 122)]
    d0 = np.load(os.path.join(ds.root, "depth", "000000.npy"))
    assert np.array_equal(ds[0][1].numpy(), d0)


def test_val_depth_root_flag_parses():
    code = ("import sys, runpy\n"
            "sys.argv = ['train.py']\n"
            f"ns = runpy.run_path({os.path.join(PKG, 'train.py')!r}, run_name='not_main')\n"
            "a = ns['parser'].parse_args(['--val-depth-root', '/some/dir'])\n"
            "assert a.val_depth_root == '/some/dir'\n"
            "assert ns['parser'].parse_args([]).val_depth_root is None\n"
            "print('PARSED')\n")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "PARSED" in r.stdout, r.stderr[-2000:]


def test_binding_declares_the_entry():
    from dvf import lib as L
    assert "dvf_depth_metrics" in L.SIGNATURES and "dvf_depth_metrics_ws_floats" in L.SIGNATURES
    lib = L.lib()
    assert lib.dvf_depth_metrics_ws_floats(4, 375, 1242) > 4 * 3 * 2 * 2048
    assert lib.dvf_depth_metrics_ws_floats(0, 8, 8) == 0
