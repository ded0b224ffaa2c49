"""Measurement of the device odometry evaluation (GPU box).

  odometry_eval_bench.py [iters]   one sequence of n = 4541 poses (KITTI's longest): a seeded walk of 0.5-1.5 m steps with yaw /
                                   pitch / roll increments, ground truth = the same walk without the drift.
    device path   dvf.odometry.chain_poses + sequence_errors on the [n-1,4,4] fp32 matrices already on the device (4 launches:
                  chain, path length, rows, summary), HIP events around `reps` back-to-back passes, median of iters; the
                  chain and the errors are also timed alone (the "kernel summary": one launch and three launches).
    host path     what it stands in for: the device-to-host copy of the matrices, odometry_eval.se3_cam2world,
                  sequence_errors and overall_error in numpy; wall clock, median of iters (at most 5: it takes seconds).
Both on the same machine in the same run; the two results are compared before anything is timed.
Give the invocation its own `timeout`."""
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-vo-feat_amd"))
import odometry_eval as oe  # noqa: E402
from dvf.odometry import chain_poses, overall, sequence_errors  # noqa: E402

N = 4541


def walk(n, seed, yaw_bias=0.0, scale=1.0):
    rng = np.random.default_rng(seed)
    out = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        y, p, r = rng.uniform(-0.05, 0.05) + yaw_bias, rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)
        Ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]])
        Rx = np.array([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]])
        Rz = np.array([[math.cos(r), -math.sin(r), 0], [math.sin(r), math.cos(r), 0], [0, 0, 1]])
        out[i, :3, :3] = Ry @ Rx @ Rz
        out[i, :3, 3] = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05), rng.uniform(0.5, 1.5)]) * scale
    return out


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
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main(iters, reps=20):
    gt_world = np.stack(oe.se3_cam2world(list(walk(N - 1, 1))))
    rel = torch.from_numpy(walk(N - 1, 1, yaw_bias=3e-4, scale=1.03).astype(np.float32)).cuda()
    gt = torch.from_numpy(np.ascontiguousarray(gt_world[:, :3])).cuda()
    gt_dict = {i: p for i, p in enumerate(gt_world)}

    def device():
        world = chain_poses(rel)
        return world, sequence_errors(gt, world)

    def host():
        world = oe.se3_cam2world(list(rel.cpu().numpy()))
        rows = oe.sequence_errors(gt_dict, {i: p for i, p in enumerate(world)})
        return world, rows, oe.overall_error(rows)

    for _ in range(3):
        world, (rows, summary) = device()
    hworld, hrows, (ht, hr) = host()
    dt, dr = (float(v) for v in overall(summary))
    werr = float(np.abs(world.cpu().numpy() - np.stack(hworld)[:, :3]).max() / np.abs(np.stack(hworld)).max())
    print(f"n = {N}: {int(summary[2])} segments (host {len(hrows)}), path {float(summary[3]):.1f} m; device vs host: world rel "
          f"{werr:.2e}, t_err/len {abs(dt - ht) / ht:.2e}, r_err/len {abs(dr - hr) / hr:.2e}", flush=True)
    med, lo, hi = _events(device, iters, reps)
    cmed, clo, chi = _events(lambda: chain_poses(rel), iters, reps)
    emed, elo, ehi = _events(lambda: sequence_errors(gt, world), iters, reps)
    hmed, hlo, hhi = _wall(host, min(iters, 5))
    print(f"device chain_poses + sequence_errors: {med * 1e3:9.1f} us per pass (events, median of {iters} x {reps}; min {lo * 1e3:.1f}, "
          f"max {hi * 1e3:.1f}), 4 launches", flush=True)
    print(f"  chain_poses alone (1 launch: 256-thread block, chunk products + LDS scan + second pass): {cmed * 1e3:9.1f} us "
          f"(min {clo * 1e3:.1f}, max {chi * 1e3:.1f})", flush=True)
    print(f"  sequence_errors alone (3 launches: path length, {rows.shape[0]} rows, summary):               {emed * 1e3:9.1f} us "
          f"(min {elo * 1e3:.1f}, max {ehi * 1e3:.1f})", flush=True)
    print(f"host copy + se3_cam2world + sequence_errors + overall_error: {hmed * 1e3:9.1f} us per pass (wall clock, median of "
          f"{min(iters, 5)}; min {hlo * 1e3:.1f}, max {hhi * 1e3:.1f}); ratio {hmed / med:.0f}x", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
