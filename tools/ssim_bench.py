"""Measurements of the SSIM + L1 appearance term (GPU box).

  ssim_bench.py kernels [iters]   forward + backward of dvf.ops.SsimL1LossFn at 4x3x256x832 (image term, with mask) and
                                  2x32x128x416 (feature-map width, no mask): per-call time from HIP events (median) and the
                                  share of the 8 TB/s HBM figure at the algorithmic bytes of dvf/ops.py.  Run it under
                                  `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ssim_bench.py kernels` for the
                                  per-kernel durations of ssim_fwd_kernel / ssim_bwd_kernel.
  ssim_bench.py step [iters]      eager step time (forward + backward + FlatAdam) of the cfg-4 body (batch 4, 256x832,
                                  DispNetS + PoseExpNet_sfm + FeatExtractor) with ssim_weight 0 and 0.85, alternating.
  ssim_bench.py minreproj [iters] forward + backward of dvf.ops.MinReprojLossFn at 4x3x256x832 (V = 2, auto-mask: K = 4) and
                                  2x32x128x416 (V = 2, K = 2), and at the same shapes the composition it replaces: K forward
                                  and V forward + backward calls of SsimL1LossFn.  Under rocprofv3 (as above) the trace holds
                                  minreproj_fwd/bwd_kernel next to ssim_fwd/bwd_kernel; the two shapes differ in grid size.
  ssim_bench.py minreproj-step [iters]  the eager cfg-4-body step with ssim_weight 0.85, min_reprojection + auto_mask off
                                  and on, alternating.
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
    from dvf.ops import SsimL1LossFn
    g = torch.Generator().manual_seed(0)
    for name, B, C, H, W, masked in (("image 4x3x256x832 mask", 4, 3, 256, 832, True), ("feat 2x32x128x416", 2, 32, 128, 416, False)):
        x = torch.rand(B, C, H, W, generator=g).cuda().requires_grad_(True)
        y = (torch.rand(B, C, H, W, generator=g) * (torch.rand(B, 1, H, W, generator=g) >= 0.1)).cuda().requires_grad_(True)
        m = (torch.rand(B, 1, H, W, generator=g) * 0.9 + 0.05).cuda().requires_grad_(True) if masked else None
        L.TIMER = L.KernelTimer()
        for _ in range(iters + 3):
            for t in (x, y, m):
                if t is not None:
                    t.grad = None
            loss = SsimL1LossFn.apply(x, y, m, (1.0, 0.85, 1e-4, 9e-4, None))
            loss.backward()
        torch.cuda.synchronize()
        rec, L.TIMER = L.TIMER.records, None
        for kind in ("ssim_fwd", "ssim_bwd"):
            ms = [r[1].elapsed_time(r[2]) for r in rec if r[0] == kind][3:]
            nbytes = [r[4] for r in rec if r[0] == kind][0]
            med = statistics.median(ms)
            print(f"{name:24s} {kind}: {med * 1e3:8.1f} us per call (events, median of {len(ms)}), {nbytes / 1e6:6.1f} MB algorithmic, "
                  f"{nbytes / HBM_BYTES_PER_S / (med * 1e-3) * 100:5.1f} % of the HBM time", flush=True)
        print(f"{name:24s} loss {float(loss):.6f}", flush=True)


def _report(name, rec, kinds):
    for kind in kinds:
        ms = [r[1].elapsed_time(r[2]) for r in rec if r[0] == kind]
        nbytes = [r[4] for r in rec if r[0] == kind][0]
        med = statistics.median(ms)
        print(f"{name:28s} {kind}: {med * 1e3:8.1f} us per call (events, median of {len(ms)}), {nbytes / 1e6:6.1f} MB algorithmic, "
              f"{nbytes / HBM_BYTES_PER_S / (med * 1e-3) * 100:5.1f} % of the HBM time", flush=True)


def minreproj(iters):
    from dvf.ops import MinReprojLossFn, SsimL1LossFn
    g = torch.Generator().manual_seed(0)
    for name, B, C, H, W, auto in (("image 4x3x256x832 V=2 auto", 4, 3, 256, 832, True), ("feat 2x32x128x416 V=2", 2, 32, 128, 416, False)):
        V = 2
        x = torch.rand(B, C, H, W, generator=g).cuda().requires_grad_(True)
        warped = [(torch.rand(B, C, H, W, generator=g) * (torch.rand(B, 1, H, W, generator=g) >= 0.1)).cuda().requires_grad_(True)
                  for _ in range(V)]
        identity = [torch.rand(B, C, H, W, generator=g).cuda() for _ in range(V if auto else 0)]
        cfg = (1.0, 0.85, 1e-4, 9e-4, auto)

        def clear():
            for t in [x] + warped:
                t.grad = None

        for _ in range(3):                                                  # warm both paths
            clear()
            MinReprojLossFn.apply(x, cfg, V, *warped, *identity)[0].backward()
            SsimL1LossFn.apply(x, warped[0], None, cfg[:4] + (None,)).backward()
        L.TIMER = L.KernelTimer()
        for _ in range(iters):
            clear()
            loss, _, counts = MinReprojLossFn.apply(x, cfg, V, *warped, *identity)
            loss.backward()
        torch.cuda.synchronize()
        rec = L.TIMER.records
        L.TIMER = L.KernelTimer()
        for _ in range(iters):                                              # the composition: K forwards, V of them with a backward
            clear()
            with torch.no_grad():
                for y in identity:
                    SsimL1LossFn.apply(x, y, None, cfg[:4] + (None,))
            sum(SsimL1LossFn.apply(x, y, None, cfg[:4] + (None,)) for y in warped).backward()
        torch.cuda.synchronize()
        rec2, L.TIMER = L.TIMER.records, None
        _report(name, rec, ("minreproj_fwd", "minreproj_bwd"))
        _report(name + " (one view)", rec2, ("ssim_fwd", "ssim_bwd"))
        print(f"{name:28s} loss {float(loss):.6f} counts {counts.tolist()}", flush=True)


def step(iters, variants=((0.0, {}), (0.85, {}))):
    import DispNetS
    import PoseExpNet_sfm
    import feat_extractor
    from dvf.engine import FlatAdam
    from dvf.steps import train_sfm_losses
    from dvf.synthetic import synthetic_batch
    torch.manual_seed(0)
    nets = [DispNetS.DispNetS(), PoseExpNet_sfm.PoseExpNet(nb_ref_imgs=2, output_exp=True), feat_extractor.FeatExtractor()]
    for n in nets:
        n.init_weights()
        n.cuda().train()
    opt = FlatAdam([p for n in nets for p in n.parameters()], lr=2e-4, overlap=True)
    batch = synthetic_batch(4, 256, 832, seed=1234, device=torch.device("cuda"), n_views=2)

    def run(w, kw, n):
        opt.relearn()                               # the variants differ in which parameters get a gradient
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss, terms = train_sfm_losses(nets[0], nets[1], batch, feat_extractor=nets[2], ssim_weight=w, **kw)
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(terms["photo"])

    for w, kw in variants:
        run(w, kw, 3)                               # warm both paths
    times = [[] for _ in variants]
    for _ in range(4):                              # alternate: the box is shared
        for i, (w, kw) in enumerate(variants):
            ms, photo = run(w, kw, iters)
            times[i].append(ms)
    for (w, kw), ts in zip(variants, times):
        print(f"cfg-4 body eager step, ssim_weight={w}{''.join(f', {k}' for k in kw)}: {statistics.median(ts):.2f} ms "
              f"(median of {len(ts)} x {iters} steps; min {min(ts):.2f}, max {max(ts):.2f})", flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    on = {"min_reprojection": True, "auto_mask": True}
    {"kernels": kernels, "step": step, "minreproj": minreproj,
     "minreproj-step": lambda k: step(k, ((0.85, {}), (0.85, on)))}[mode](n)
