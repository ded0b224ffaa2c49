"""Measurements of full-resolution multi-scale sampling (GPU box).

  fullres_bench.py kernels [iters]  forward + backward of dvf.ops.UpsampleIntFn at the train.py shapes of batch 4, 256x832:
                                    the disparities (4 planes, fused reciprocal) and the masks (8 planes, plain) of the scales
                                    x2, x4, x8: per-call time from HIP events (median) and the share of the 8 TB/s HBM figure
                                    at the algorithmic bytes of dvf/ops.py.  Run it under
                                    `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/fullres_bench.py kernels` for the
                                    durations of upsample_int_fwd_kernel / upsample_int_bwd_kernel themselves.
  fullres_bench.py step [iters]     train.py-form step (DispNetS + PoseExpNet_sfm, batch 4, 256x832; forward + backward +
                                    FlatAdam, eager) with the flag off, on (masks, w2 = 0.2) and on with SSIM + minimum
                                    reprojection + auto-mask, next to the same two bodies without the flag; alternating.
Give each invocation its own `timeout`."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-vo-feat_amd"))
from dvf import lib as L  # noqa: E402

HBM_BYTES_PER_S = 8e12


def kernels(iters):
    from dvf.ops import UpsampleIntFn
    g = torch.Generator().manual_seed(0)
    H, W = 256, 832
    for planes, eps, what in ((4, 0.0, "disparity -> depth"), (8, None, "masks")):
        for f in (2, 4, 8):
            x = (torch.rand(planes, 1, H // f, W // f, generator=g) + 0.05).cuda().requires_grad_(True)
            gout = torch.randn(planes, 1, H, W, generator=g).cuda()
            for _ in range(3):
                x.grad = None
                UpsampleIntFn.apply(x, f, eps).backward(gout)
            L.TIMER = L.KernelTimer()
            for _ in range(iters):
                x.grad = None
                UpsampleIntFn.apply(x, f, eps).backward(gout)
            torch.cuda.synchronize()
            rec, L.TIMER = L.TIMER.records, None
            for kind in ("upsample_int_fwd", "upsample_int_bwd"):
                ms = [r[1].elapsed_time(r[2]) for r in rec if r[0] == kind]
                nbytes = [r[4] for r in rec if r[0] == kind][0]
                med = statistics.median(ms)
                print(f"{what:18s} x{f} {planes} planes {kind}: {med * 1e3:7.1f} us per call (events, median of {len(ms)}), "
                      f"{nbytes / 1e6:5.1f} MB algorithmic, {nbytes / HBM_BYTES_PER_S / (med * 1e-3) * 100:5.1f} % of the HBM time",
                      flush=True)


def step(iters):
    import DispNetS
    import PoseExpNet_sfm
    from dvf.engine import FlatAdam
    from dvf.steps import train_sfm_losses
    from dvf.synthetic import synthetic_batch
    torch.manual_seed(0)
    nets = [DispNetS.DispNetS(), PoseExpNet_sfm.PoseExpNet(nb_ref_imgs=2, output_exp=True)]
    for n in nets:
        n.init_weights()
        n.cuda().train()
    opt = FlatAdam([p for n in nets for p in n.parameters()], lr=2e-4, overlap=True)
    batch = synthetic_batch(4, 256, 832, seed=1234, device=torch.device("cuda"), n_views=2)
    appearance = {"ssim_weight": 0.85, "min_reprojection": True, "auto_mask": True}
    variants = [("flag off, masks", {"w2": 0.2}), ("flag on,  masks", {"w2": 0.2, "full_res_multiscale": True}),
                ("flag off, appearance", dict(appearance)), ("flag on,  appearance", dict(appearance, full_res_multiscale=True))]

    def run(kw, n):
        opt.relearn()                               # the variants differ in which parameters get a gradient
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss, terms = train_sfm_losses(nets[0], nets[1], batch, **kw)
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for _, kw in variants:
        run(kw, 3)
    times = [[] for _ in variants]
    for _ in range(4):                              # alternate: the box is shared
        for i, (_, kw) in enumerate(variants):
            times[i].append(run(kw, iters))
    for (name, _), ts in zip(variants, times):
        print(f"train.py-form eager step, batch 4 256x832, {name}: {statistics.median(ts):.2f} ms "
              f"(median of {len(ts)} x {iters} steps; min {min(ts):.2f}, max {max(ts):.2f})", flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    {"kernels": kernels, "step": step}[mode](n)
