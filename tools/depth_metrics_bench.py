"""Measurements of the device depth metrics (GPU box).

  depth_metrics_bench.py [iters]   dvf_depth_metrics (dvf.metrics.depth_metrics: Garg crop, median scaling) at 4x375x1242 and
                                   4x256x832 on KITTI-like data -- ground truth ~30 % dense and quantised to 1/256 m, depth
                                   growing towards the horizon, a prediction off by a scale and 10 % noise -- against
                                   loss_functions_sfm.compute_errors on the SAME GPU tensors (the per-image boolean gather,
                                   two sorts and six .cpu() transfers it replaces; wall clock, it synchronises by itself).
                                   The device call is timed with HIP events around `reps` back-to-back calls (median of iters).
                                   Also printed: the traffic floor of the pass structure -- four passes (three digit
                                   histograms, one metrics pass) each read gt and pred once, 4 * 2 * 4 * B*H*W bytes over the
                                   8 TB/s HBM figure -- the share of it reached, and the launch count (6: zero, 3 x histogram,
                                   metrics, finish).  At these sizes both maps (15 MB at the larger shape) stay in the
                                   256 MB last-level cache between passes, so the floor is a yardstick, not a bound.
With DVF_LIB pointing at the -DDVF_TUNING build the histogram variants are timed as well (DVF_DM_HIST: 0 = one LDS add per
lane, 1 = aggregated within the wave (the product), 3 / 4 = the same with 2 / 8 rounds, 2 = per-wave sub-histograms) and their rows compared bit for bit.
Give the invocation its own `timeout`."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-vo-feat_amd"))
from dvf import lib as L  # noqa: E402

HBM_BYTES_PER_S = 8e12
LAUNCHES = 6


def kitti_like(b, h, w, seed, dropout=0.7):
    g = torch.Generator().manual_seed(seed)
    rows = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    horizon = 0.42 * h
    depth = (1.65 * 0.58 * w / (rows - horizon).clamp(min=1.0)).clamp(max=85.0).expand(b, h, w)     # ground plane, camera 1.65 m up
    depth = depth * (1 + 0.15 * torch.rand(b, h, w, generator=g, dtype=torch.float64))
    obstacles = torch.rand(b, h, w, generator=g, dtype=torch.float64) < 0.2
    depth = torch.where(obstacles, depth * 0.5, depth)
    gt = torch.where(torch.rand(b, h, w, generator=g, dtype=torch.float64) < dropout, torch.zeros_like(depth), depth)
    gt = (torch.round(gt * 256) / 256).float()
    pred = (depth * 0.37 * (1 + 0.1 * torch.randn(b, h, w, generator=g, dtype=torch.float64))).float()
    return gt.cuda(), pred.cuda()


def _events(fn, iters, reps):
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return statistics.median(ms), min(ms), max(ms)


def _wall(fn, iters):
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main(iters, reps=20):
    import loss_functions_sfm as LS
    from dvf.metrics import depth_metrics
    tuning = bool(L.lib().dvf_build_has_tuning())
    # (the third case, tuning build only: DENSE ground truth, as rendered or completed depth gives -- every lane of a wave
    # active and neighbouring pixels in one bin, the worst case for LDS atomics on one address)
    for b, h, w, dropout in ((4, 375, 1242, 0.7), (4, 256, 832, 0.7)) + (((4, 375, 1242, 0.0),) if tuning else ()):
        gt, pred = kitti_like(b, h, w, seed=h, dropout=dropout)
        dense = float((gt > 0).float().mean())
        floor_us = 4 * 2 * 4 * b * h * w / HBM_BYTES_PER_S * 1e6
        for _ in range(3):
            depth_metrics(gt, pred)
            LS.compute_errors(gt, pred)
        rows = depth_metrics(gt, pred)
        six = LS.compute_errors_device(gt, pred)
        base = LS.compute_errors(gt, pred)
        dev = max(abs(a - c) / abs(c) for a, c in zip(six, base))
        print(f"{b}x{h}x{w}: gt {dense * 100:.1f} % dense, n_valid {rows[:, 8].tolist()}, device vs compute_errors max rel {dev:.2e}")
        med, lo, hi = _events(lambda: depth_metrics(gt, pred), iters, reps)
        bmed, blo, bhi = _wall(lambda: LS.compute_errors(gt, pred), iters)
        print(f"{b}x{h}x{w} dvf_depth_metrics: {med * 1e3:8.1f} us per call (events, median of {iters} x {reps}; min "
              f"{lo * 1e3:.1f}, max {hi * 1e3:.1f}), {LAUNCHES} launches; traffic floor {floor_us:.1f} us = "
              f"{floor_us / (med * 1e3) * 100:.1f} % of the time", flush=True)
        print(f"{b}x{h}x{w} compute_errors   : {bmed * 1e3:8.1f} us per call (wall clock, median of {iters}; min {blo * 1e3:.1f}, "
              f"max {bhi * 1e3:.1f}); ratio {bmed / med:.1f}x", flush=True)
        if tuning:
            want = rows.view(torch.int32).clone()
            for mode, name in ((0, "one add per lane"), (1, "aggregated in the wave, 1 round: the product"),
                               (3, "aggregated, 2 rounds"), (4, "aggregated, 8 rounds"), (2, "per-wave sub-histograms")):
                os.environ["DVF_DM_HIST"] = str(mode)
                for _ in range(3):
                    got = depth_metrics(gt, pred)
                same = bool(got.view(torch.int32).equal(want))
                m, mlo, mhi = _events(lambda: depth_metrics(gt, pred), iters, reps)
                print(f"{b}x{h}x{w} DVF_DM_HIST={mode} ({name}): {m * 1e3:8.1f} us per call (min {mlo * 1e3:.1f}, max {mhi * 1e3:.1f}); "
                      f"rows bit-identical to the product's: {same}", flush=True)
            os.environ.pop("DVF_DM_HIST", None)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
