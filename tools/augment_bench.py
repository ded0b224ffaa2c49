"""Measurements of the training augmentation (GPU box).

  augment_bench.py [iters]   dvf_augment_frames at the cfg-2 batch (F = 3 frames, B = 4, 3x256x832): HIP-event time per launch
                             with all ops on, with colour off and with the identity record, next to the three copy_ calls it
                             replaces (loader tensor -> static input tensor), in the same process, alternating.  A sample is
                             the time between two events around REPS back-to-back launches, divided by REPS; the figure is
                             the median of `iters` samples after a warm-up.  Source / destination sets rotate over more memory
                             than the 256 MiB Infinity Cache holds, so the bytes come from HBM.  Algorithmic bytes:
                             2 F B 3 H W 4 (every frame read once, written once); share = their time at 8 TB/s over the
                             measured time.  Then augment_batch (frames + geometry launch, host side included).
The clocks the driver reports are printed before and after.  Give the invocation its own `timeout`."""
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-vo-feat_amd"))
from dvf import augment  # noqa: E402
from dvf import lib as L  # noqa: E402

HBM_BYTES_PER_S = 8e12
REPS = 10


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        rows = [l.strip() for l in out.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l or "fclk" in l)]
        return "; ".join(rows) if rows else "clock state: not reported"
    except (OSError, subprocess.SubprocessError):
        return "clock state: rocm-smi not available"


def sample(fn, sets):
    """Milliseconds per call of fn(set) over REPS back-to-back calls on rotating buffer sets."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(REPS):
        fn(sets[i % len(sets)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS


def main(iters):
    F, B, C, H, W = 3, 4, 3, 256, 832
    nbytes = 2 * F * B * C * H * W * 4
    n_sets = 6                                            # 6 x 61.3 MB of sources + destinations > the Infinity Cache
    g = torch.Generator().manual_seed(0)
    sets = []
    for _ in range(n_sets):
        src = [(torch.rand(B, C, H, W, generator=g) * 255).cuda() for _ in range(F)]
        dst = [torch.empty_like(s) for s in src]
        sets.append((src, dst, L.ptr_array(src), L.ptr_array(dst)))
    sw, sh = int(1.15 * W), int(1.15 * H)
    ident = augment.identity_params(B, H, W)
    geo = ident.clone()
    for b in range(B):                                    # every sample differs: flip, zoom size and crop offset
        geo[b, :5] = torch.tensor([b % 2, sw - 7 * b, sh - 3 * b, (sw - 7 * b - W) // (b + 1), (sh - 3 * b - H) // (b + 1)])
    full = geo.clone()
    full[:, 5] = 1
    full[:, 6:11] = torch.tensor([[0.8, 2.0, 0.8, 1.0, 1.2], [1.2, 0.5, 1.2, 0.9, 0.8], [1.1, 1.3, 1.0, 1.1, 0.9],
                                  [0.9, 0.7, 1.1, 0.8, 1.0]])
    lib = L.lib()
    rows = {}
    for name, rec in (("all ops", full), ("colour off", geo), ("identity", ident)):
        augment.validate_params(rec, H, W)
        dev = rec.cuda()

        def launch(s, dev=dev):
            L.check(lib.dvf_augment_frames(s[2], s[3], F, dev.data_ptr(), B, C, H, W, 255.0, L.stream()), "dvf_augment_frames")
        rows["dvf_augment_frames, " + name] = launch

    def copies(s):
        for a, b in zip(s[0], s[1]):
            b.copy_(a, non_blocking=True)
    rows["3 x copy_ (what it replaces)"] = copies

    print(clocks(), flush=True)
    for fn in rows.values():
        for _ in range(3):
            sample(fn, sets)
    torch.cuda.synchronize()
    times = {k: [] for k in rows}
    for _ in range(iters):                                # alternate: the box is shared
        for k, fn in rows.items():
            times[k].append(sample(fn, sets))
    copy_ms = statistics.median(times["3 x copy_ (what it replaces)"])
    for k, ts in times.items():
        med = statistics.median(ts)
        print(f"{k:40s} {med * 1e3:7.1f} us (median of {len(ts)} x {REPS} launches; min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f}), "
              f"{nbytes / 1e6:.1f} MB algorithmic, {nbytes / HBM_BYTES_PER_S / (med * 1e-3) * 100:5.1f} % of 8 TB/s, "
              f"{med / copy_ms:4.2f} x the copy_ time", flush=True)

    # the whole wrapper: frame launch + geometry launch + the host side of both
    from dvf.synthetic import synthetic_batch
    src = synthetic_batch(B, H, W, device="cuda")
    dst = {k: ([torch.empty_like(t) for t in v] if isinstance(v, list) else torch.empty_like(v)) for k, v in src.items()}
    dev = full.cuda()
    for _ in range(3):
        augment.augment_batch(src, dst, dev)
    ts = [sample(lambda _s: augment.augment_batch(src, dst, dev), [None]) for _ in range(iters)]
    print(f"{'augment_batch (frames + geometry)':40s} {statistics.median(ts) * 1e3:7.1f} us per call (same buffers every call)", flush=True)
    print(clocks(), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
