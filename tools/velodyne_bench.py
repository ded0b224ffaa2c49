"""Measurement of the LiDAR depth maps (GPU box).

  velodyne_bench.py [iters]   one dvf.velodyne.depth_maps call for 4 frames of ~120 k points at 375 x 1242 (a KITTI raw batch):
                              points spread like a sweep (forward half kept by the kernel's own test, depths 2..80 m), a
                              KITTI-like camera.  HIP events around `reps` back-to-back calls, median of iters after a
                              warm-up; the sweeps rotate over enough sets to exceed the 256 MB last-level cache (the map is
                              a fresh allocation per call, as in a validation pass).  Printed next to the time: the host's
                              own time to enqueue a call (wall clock around the same loop, before the synchronise: when it
                              equals the event time the figure is the host's submission rate, not the kernels'), the bytes
                              the call needs -- 16 B per point read once, the map written by the fill pass, read and written
                              by the finish pass, 4 B of atomic per kept point -- as a time at the 8 TB/s HBM figure, and
                              the launch count (3).  The kernels' own durations come from a separate
                              `rocprofv3 --kernel-trace --stats -- python tools/velodyne_bench.py 3` run.
Give the invocation its own `timeout`."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-vo-feat_amd"))
from dvf.velodyne import depth_maps  # noqa: E402

HBM_BYTES_PER_S = 8e12
LAUNCHES = 3
# A KITTI-like pinhole camera (focal length 721.5 px, principal point (609.6, 172.9)) looking along the sensor's forward
# axis from 0.27 m behind and 0.08 m above it: camera x = -left, y = -up, z = forward.
PROJ = np.array([[721.5, 0.0, 609.6], [0.0, 721.5, 172.9], [0.0, 0.0, 1.0]]) @ np.array(
    [[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, -0.08], [1.0, 0.0, 0.0, -0.27]])


def sweep(n, seed):
    """n points on 64 rings over the full circle: range 2..80 m, elevation -24.8..+2 degrees, as the sensor spins."""
    rng = np.random.RandomState(seed)
    az = rng.uniform(-np.pi, np.pi, size=n)
    el = np.deg2rad(rng.uniform(-24.8, 2.0, size=n))
    r = np.minimum(rng.uniform(2.0, 80.0, size=n), 1.73 / np.maximum(np.sin(-el), 1e-3))      # the ground, sensor 1.73 m up
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.uniform(size=n)], 1).astype(np.float32)


def main(iters, reps=10, B=4, n=120000, H=375, W=1242):
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    set_bytes = B * n * 16                                              # (only the sweeps rotate)
    nsets = int(300e6 // set_bytes) + 2
    P = torch.from_numpy(np.stack([PROJ] * B)).cuda()
    counts = [n - 1000 * b for b in range(B)]
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).cuda()
    sets = [torch.from_numpy(np.concatenate([sweep(c, seed=17 * s + b) for b, c in enumerate(counts)])).cuda() for s in range(nsets)]
    total = sets[0].shape[0]
    for s in range(nsets):                                              # warm-up, every set once
        out = depth_maps(sets[s], offsets, P, H, W)
    torch.cuda.synchronize()
    kept = int((out > 0).sum())
    front = int((sets[-1][:, 0] >= 0).sum())
    again = depth_maps(sets[-1], offsets, P, H, W)
    print(f"{B} frames, {total} points ({front} forward), {H}x{W}: {kept} pixels measured ({kept / (B * H * W) * 100:.1f} %), "
          f"second run bit-identical: {bool(out.view(torch.int32).equal(again.view(torch.int32)))}; {nsets} rotating sets of "
          f"{set_bytes / 1e6:.1f} MB")
    ms, host, k = [], [], 0
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        t0 = time.perf_counter()
        for _ in range(reps):
            depth_maps(sets[k % nsets], offsets, P, H, W)
            k += 1
        host.append((time.perf_counter() - t0) * 1e3 / reps)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    med, lo, hi = statistics.median(ms), min(ms), max(ms)
    needed = total * 16 + 3 * B * H * W * 4 + kept * 4                   # points, fill write, finish read + write, atomics (>= kept)
    floor_us = needed / HBM_BYTES_PER_S * 1e6
    print(f"depth_maps: {med * 1e3:.1f} us per call (events, median of {iters} x {reps}; min {lo * 1e3:.1f}, max {hi * 1e3:.1f}), "
          f"host enqueue {statistics.median(host) * 1e3:.1f} us per call (wall clock, same loop), {LAUNCHES} launches; bytes needed "
          f"{needed / 1e6:.1f} MB = {floor_us:.1f} us at 8 TB/s = {floor_us / (med * 1e3) * 100:.1f} % of the time", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
