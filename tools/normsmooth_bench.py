"""Measurements of the edge-aware smoothness of the mean-normalised disparity (GPU box).

  normsmooth_bench.py [iters]   forward + backward of dvf.ops.NormSmoothLossFn at batch 4 on the four train.py scales of 256x832
                                (256x832 ... 32x104, three-channel image): per-call time from HIP events (median) of the
                                forward (tile pass + finishing launch) and of the backward (one launch), the algorithmic bytes
                                -- (1+C)*4*BHW read by the forward, the same plus 4*BHW written by the backward -- and their
                                share of the 8 TB/s HBM figure; then the whole four-scale call next to dvf.ops.SmoothLossFn
                                (the second-order term it replaces) on the same maps, events around forward + backward.
Run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/normsmooth_bench.py` for the durations of
norm_smooth_fwd_kernel / norm_smooth_finish_kernel / norm_smooth_bwd_kernel themselves.  Give the invocation its own `timeout`."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-vo-feat_amd"))
from dvf import lib as L  # noqa: E402

HBM_BYTES_PER_S = 8e12


def _events(fn, iters):
    """Median milliseconds of fn() between two HIP events on the current stream."""
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main(iters):
    from dvf.conv import area_downsample
    from dvf.ops import NormSmoothLossFn, SmoothLossFn
    g = torch.Generator().manual_seed(0)
    B, C, H, W = 4, 3, 256, 832
    img = (torch.rand(B, C, H, W, generator=g) * 2 - 1).cuda()
    disps = [(10 * torch.sigmoid(2 * torch.randn(B, 1, H >> s, W >> s, generator=g)) + 0.01).cuda().requires_grad_(True)
             for s in range(4)]
    imgs = [area_downsample(img, tuple(d.shape[2:])) for d in disps]
    cfg = (2.0, 1.0, 1e-7)

    def clear():
        for d in disps:
            d.grad = None

    for s, (d, i) in enumerate(zip(disps, imgs)):
        for _ in range(3):
            clear()
            NormSmoothLossFn.apply(cfg, d, i).backward()
        L.TIMER = L.KernelTimer()
        for _ in range(iters):
            clear()
            NormSmoothLossFn.apply(cfg, d, i).backward()
        torch.cuda.synchronize()
        rec, L.TIMER = L.TIMER.records, None
        for kind in ("normsmooth_fwd", "normsmooth_bwd"):
            ms = [r[1].elapsed_time(r[2]) for r in rec if r[0] == kind]
            nbytes = [r[4] for r in rec if r[0] == kind][0]
            med = statistics.median(ms)
            print(f"scale {s} {B}x{C}x{H >> s}x{W >> s} {kind}: {med * 1e3:7.1f} us per call (events, median of {len(ms)}), "
                  f"{nbytes / 1e6:6.2f} MB algorithmic, {nbytes / HBM_BYTES_PER_S / (med * 1e-3) * 100:5.1f} % of the HBM time",
                  flush=True)

    pairs = [t for d, i in zip(disps, imgs) for t in (d, i)]

    def norm():
        clear()
        NormSmoothLossFn.apply(cfg, *pairs).backward()

    def second_order():
        clear()
        SmoothLossFn.apply(2.0, *disps).backward()

    for fn in (norm, second_order):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {"NormSmoothLossFn": [], "SmoothLossFn": []}
    for _ in range(4):                                  # alternate: the box is shared
        times["NormSmoothLossFn"].append(_events(norm, iters))
        times["SmoothLossFn"].append(_events(second_order, iters))
    for name, ts in times.items():
        print(f"four scales, forward + backward, {name}: {statistics.median(ts) * 1e3:7.1f} us per call "
              f"(events around the call, median of {len(ts)} x {iters}; min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f})",
              flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 50)
