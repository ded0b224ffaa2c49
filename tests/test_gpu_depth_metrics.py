"""dvf_depth_metrics on the GPU against the test-side definition (tests/depth_metrics_ref.py).

Bounds: n_valid and both medians EQUAL the restatement (the select is exact); the three threshold counts equal it up to the
number of pixels within 1e-6 of a threshold (zero at the small shapes: tests/test_depth_metrics.py asserts that); the five
error means agree to the suite's 1e-4 (conftest.rel_err, per column); a second run is bit-identical.
Measured worst deviation of an error mean over every case of this file: 1.8e-6 (test_gt_bounds_are_strict, two valid
pixels); 2.7e-7 over the random cases."""
import ctypes
import math

import numpy as np
import pytest
import torch

import depth_metrics_ref as R
from conftest import load_golden, rel_err, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _run(gt, pred, **kw):
    from dvf.metrics import depth_metrics
    rows = depth_metrics(gt.to(DEV).contiguous(), pred.to(DEV).contiguous(), **kw)
    torch.cuda.synchronize()
    return rows.cpu()


def _check(gt, pred, tag="", **kw):
    ref, near = R.rows(gt, pred, **kw)
    got = _run(gt, pred, **kw)
    again = _run(gt, pred, **kw)
    assert got.view(torch.int32).equal(again.view(torch.int32)), "a second run differs"
    worst = 0.0
    for i in range(ref.shape[0]):
        r, g = ref[i], got[i].double()
        assert g[8] == r[8] and g[11] == r[11], (tag, i, "n_valid / n_nan", g, r)
        if r[8] == 0:
            assert float(g.abs().sum()) == 0.0, (tag, i, g)
            continue
        assert g[9] == r[9], (tag, i, "med_gt", float(g[9]), float(r[9]))
        if r[11] > 0:
            assert torch.isnan(g[:8]).all() and math.isnan(float(g[10])), (tag, i, g)
            continue
        assert g[10] == r[10], (tag, i, "med_pred", float(g[10]), float(r[10]))
        for e in range(3):
            cg, cr = round(float(g[5 + e] * g[8])), round(float(r[5 + e] * r[8]))
            assert abs(cg - cr) <= int(near[i, e]), (tag, i, f"a{e + 1}", cg, cr, int(near[i, e]))
        for c in range(5):
            err = rel_err(g[c], r[c])
            worst = max(worst, err)
            assert err < 1e-4, (tag, i, R.COLUMNS[c], float(g[c]), float(r[c]))
    print(f"{tag}: worst error-mean deviation {worst:.3g}")
    return got, ref


@pytest.mark.parametrize("shape,crop,quantum", R.SMALL_CASES)
def test_random_small(shape, crop, quantum):
    gt, pred = R.gen_case(*shape, quantum=quantum)
    _check(gt, pred, tag=f"{shape} crop={crop} q={quantum}", crop=crop)


@pytest.mark.parametrize("crop", [True, False])
def test_golden_fixture(crop):
    g = load_golden("metrics_compute_errors")
    _check(t(g["gt"]), t(g["pred"]), tag=f"golden crop={crop}", crop=crop)


@pytest.mark.parametrize("shape", [(1, 375, 1242), (1, 600, 1000)])
def test_large(shape):
    """KITTI's size (228 blocks of 2048 pixels per image) and one with more than 256 blocks per image, where the finishing
    block's threads add more than one partial each.  The closest pixel lies 1.6e-6 from a threshold at 375 x 1242: too close
    to demand equal counts, so the allowance of the restatement applies at these sizes."""
    gt, pred = R.gen_case(*shape)
    _check(gt, pred, tag=str(shape), crop=True)


# ------------------------------------------------------------------ constructed cases for the select

def _filled(b, h, w, value=0.0):
    return torch.full((b, h, w), value, dtype=torch.float32)


def test_all_valid_gt_equal():
    gt, pred = _filled(1, 8, 40, 12.5), torch.rand(1, 8, 40, generator=torch.Generator().manual_seed(3)) * 20 + 1
    got, _ = _check(gt, pred, crop=False)
    assert got[0, 8] == 320 and got[0, 9] == 12.5


def test_values_differing_in_the_lowest_ten_bits():
    """1024 ground-truth values that share their upper 22 bits: only the last digit pass separates them."""
    g = torch.Generator().manual_seed(7)
    bits = (torch.tensor(0x41A00000, dtype=torch.int32) + torch.arange(1024, dtype=torch.int32))[torch.randperm(1024, generator=g)]
    gt = bits.view(torch.float32).reshape(1, 16, 64).clone()
    pbits = (torch.tensor(0x40400000, dtype=torch.int32) + torch.arange(1024, dtype=torch.int32))[torch.randperm(1024, generator=g)]
    pred = pbits.view(torch.float32).reshape(1, 16, 64).clone()
    got, _ = _check(gt, pred, crop=False)
    assert got[0, 9].view(torch.int32) == 0x41A00000 + 511 and got[0, 10].view(torch.int32) == 0x40400000 + 511


@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_valid_counts(n):
    gt, pred = _filled(1, 5, 9), _filled(1, 5, 9, 2.0)
    vals, preds = [30.0, 10.0, 20.0], [6.0, 1.0, 3.0]
    for k in range(n):
        gt[0, 1 + k, 2 * k + 1] = vals[k]
        pred[0, 1 + k, 2 * k + 1] = preds[k]
    got, _ = _check(gt, pred, crop=False)
    assert got[0, 8] == n
    assert got[0, 9] == sorted(vals[:n])[(n - 1) // 2] and got[0, 10] == sorted(preds[:n])[(n - 1) // 2]   # n = 2: the lower


def test_empty_image_between_two_normal_ones():
    from dvf.metrics import reduce_rows
    gt, pred = R.gen_case(3, 9, 65)
    gt[1] = 0.0
    got, ref = _check(gt, pred, crop=False)
    assert float(got[1].abs().sum()) == 0.0 and got[0, 8] > 0 and got[2, 8] > 0
    mean = reduce_rows(got.to(DEV)).cpu().double()
    want = (ref[0, :8] + ref[2, :8]) / 2
    for c in range(8):
        assert rel_err(mean[c], want[c]) < 1e-4


def test_empty_crop_rectangle():
    gt, pred = R.gen_case(2, 8, 64)
    for rect in ((3, 3, 0, 64), (0, 8, 10, 10)):
        got, _ = _check(gt, pred, rect=rect)
        assert float(got.abs().sum()) == 0.0


def test_gt_bounds_are_strict():
    below = float(np.nextafter(np.float32(80.0), np.float32(0.0)))
    gt = torch.tensor([[[0.0, 80.0, below, 5.0, NAN, -1.0, float("inf"), 81.0]]])
    pred = torch.tensor([[[1.0, 1.0, 40.0, 2.0, 1.0, 1.0, 1.0, 1.0]]])
    got, _ = _check(gt, pred, crop=False)
    assert got[0, 8] == 2 and got[0, 9] == 5.0 and got[0, 10] == 2.0


# ------------------------------------------------------------------ constructed cases for the clamp

def test_every_prediction_below_the_clamp():
    gt, _ = R.gen_case(1, 8, 63)
    got, _ = _check(gt, _filled(1, 8, 63, 1e-5), crop=False)
    assert got[0, 10] == torch.tensor(1e-3, dtype=torch.float32)


def test_negative_zero_and_infinite_predictions():
    gt = torch.tensor([[[10.0, 20.0, 30.0, 40.0, 50.0]]])
    pred = torch.tensor([[[-1.0, -0.0, float("inf"), 7.0, float("-inf")]]])
    got, _ = _check(gt, pred, crop=False, median_scaling=False)
    assert got[0, 8] == 5 and got[0, 11] == 0 and got[0, 10] == torch.tensor(1e-3, dtype=torch.float32)
    _check(gt, pred, crop=False)


def test_nan_prediction_at_a_valid_pixel():
    gt, pred = R.gen_case(3, 9, 65)
    clean, _ = _check(gt, pred, crop=False)
    y, x = [int(v) for v in torch.nonzero((gt[1] > 0) & (gt[1] < 80))[0]]
    pred[1, y, x] = NAN
    got, _ = _check(gt, pred, crop=False)
    assert got[1, 11] == 1 and torch.isnan(got[1, :8]).all() and got[1, 8] == clean[1, 8] and got[1, 9] == clean[1, 9]
    assert got[0].view(torch.int32).equal(clean[0].view(torch.int32)) and got[2].view(torch.int32).equal(clean[2].view(torch.int32))


def test_nan_prediction_at_an_invalid_pixel():
    gt, pred = R.gen_case(2, 8, 64)
    clean, _ = _check(gt, pred, crop=False)
    y, x = [int(v) for v in torch.nonzero(gt[1] == 0)[0]]
    pred[1, y, x] = NAN
    got, _ = _check(gt, pred, crop=False)
    assert got.view(torch.int32).equal(clean.view(torch.int32))


# ------------------------------------------------------------------ flags

def test_median_scaling_off_still_reports_the_medians():
    gt, pred = R.gen_case(2, 17, 257)
    on, _ = _check(gt, pred, crop=True)
    off, _ = _check(gt, pred, crop=True, median_scaling=False)
    assert off[:, 9:11].equal(on[:, 9:11]) and not off[:, :5].equal(on[:, :5])


def test_reclamp_after_a_scale_that_passes_the_cap():
    """Predictions of a tenth of the ground truth: the scale is ~10 and the largest scaled values pass 80 m."""
    gt, pred = R.gen_case(2, 17, 257)
    pred = (gt * 0.1 * (1 + 0.5 * torch.rand(gt.shape, generator=torch.Generator().manual_seed(9)))).float()
    plain, ref_plain = _check(gt, pred, crop=False)
    re, ref_re = _check(gt, pred, crop=False, reclamp=True)
    assert not ref_plain[:, 0].equal(ref_re[:, 0]) and not plain[:, 0].equal(re[:, 0])     # the second clamp acted


def test_non_default_gt_lo():
    gt, pred = R.gen_case(2, 8, 64)
    gt[0, 0, :8] = torch.tensor([1e-3, 5e-4, 2e-3, 1e-3, 9e-4, 1.5e-3, 0.0, 1e-3])
    gt[0, 1:] = 0.0
    gt[0, 0, 8:] = 0.0
    got, _ = _check(gt, pred, crop=False, min_depth=1e-3)
    assert got[0, 8] == 2                       # 2e-3 and 1.5e-3; fl(1e-3) itself is excluded
    got0, _ = _check(gt, pred, crop=False)
    assert got0[0, 8] == 7


# ------------------------------------------------------------------ graph capture, argument checks, Python API

def test_graph_capture_and_replay():
    from dvf.metrics import depth_metrics
    gt_a, pred_a = R.gen_case(2, 17, 257)
    gt_b, pred_b = R.gen_case(2, 17, 257, seed=99)
    gt, pred = gt_a.to(DEV), pred_a.to(DEV)
    depth_metrics(gt, pred)                      # eager once
    torch.cuda.synchronize()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            rows = depth_metrics(gt, pred)
    torch.cuda.current_stream().wait_stream(stream)
    for g_new, p_new in ((gt_b, pred_b), (gt_a, pred_a)):
        gt.copy_(g_new)
        pred.copy_(p_new)
        graph.replay()
        torch.cuda.synchronize()
        ref, _ = R.rows(g_new, p_new)
        got = rows.cpu().double()
        assert got[:, 8:11].equal(ref[:, 8:11])
        for c in range(5):
            assert rel_err(got[:, c], ref[:, c]) < 1e-4


def test_invalid_arguments_are_rejected_on_the_host():
    from dvf import lib as L
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    B, H, W = 2, 8, 16
    n = lib.dvf_depth_metrics_ws_floats(B, H, W)
    good = dict(gt=fake, pred=fake, out=fake, ws=fake, n=n, B=B, H=H, W=W, y1=0, y2=H, x1=0, x2=W, gt_lo=0.0, gt_hi=80.0,
                c_lo=1e-3, c_hi=80.0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.dvf_depth_metrics(a["gt"], a["pred"], a["out"], a["ws"], a["n"], a["B"], a["H"], a["W"], a["y1"], a["y2"],
                                     a["x1"], a["x2"], a["gt_lo"], a["gt_hi"], a["c_lo"], a["c_hi"], 1, None)

    bad = [dict(gt=None), dict(pred=None), dict(out=None), dict(ws=None), dict(B=0), dict(H=0), dict(W=-1), dict(n=n - 1),
           dict(y1=-1), dict(y2=H + 1), dict(x1=-1), dict(x2=W + 1), dict(y1=5, y2=4), dict(x1=9, x2=8), dict(c_lo=0.0),
           dict(c_lo=-1.0), dict(c_lo=81.0), dict(gt_lo=-1e-3), dict(B=4, H=32768, W=16384, n=1 << 40)]
    for kw in bad:
        assert call(**kw) == -1, kw


def test_compute_errors_device_against_the_reference_vectors():
    import loss_functions_sfm as LS
    g = load_golden("metrics_compute_errors")
    for key, crop in (("crop", True), ("full", False)):
        got = LS.compute_errors_device(t(g["gt"], DEV), t(g["pred"], DEV), crop=crop)
        assert len(got) == 6
        for a, b in zip(got, g[key]):
            assert rel_err(a, b) < 1e-4, (key, got, g[key])


def test_depth_metrics_refuses_cpu_tensors():
    from dvf.metrics import depth_metrics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        depth_metrics(torch.rand(1, 8, 8), torch.rand(1, 8, 8))
