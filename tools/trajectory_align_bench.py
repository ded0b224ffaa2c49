"""Measurement of the device trajectory alignment and its errors (GPU box).

  trajectory_align_bench.py [iters]   one sequence of n = 4541 poses (KITTI's longest): the walk of odometry_eval_bench.py, the
                                      prediction with a yaw drift and a 3 % scale error, already chained on the device.
    device path   dvf.odometry.align (7dof: sums, centred sums, solve, apply) + sequence_errors + trajectory_errors +
                  snippet_errors on the [n,3,4] fp64 chain (11 launches), HIP events around `reps` back-to-back passes,
                  median of iters; each of the four is also timed alone.
    host path     what it stands in for: the device-to-host copy of the chain, then odometry_eval.trajectory_alignment,
                  apply_alignment, sequence_errors + overall_error, trajectory_errors and snippet_errors in numpy; wall clock,
                  median of iters (at most 5: it takes seconds).
Both on the same machine in the same run; the two results are compared before anything is timed.
Give the invocation its own `timeout`."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-vo-feat_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odometry_eval as oe  # noqa: E402
from dvf.odometry import align, chain_poses, overall, sequence_errors, snippet_errors, trajectory_errors  # noqa: E402
from odometry_eval_bench import N, _events, _wall, walk  # noqa: E402

MODE = "7dof"


def main(iters, reps=20):
    gt_world = np.stack(oe.se3_cam2world(list(walk(N - 1, 1))))
    rel = torch.from_numpy(walk(N - 1, 1, yaw_bias=3e-4, scale=1.03).astype(np.float32)).cuda()
    gt = torch.from_numpy(np.ascontiguousarray(gt_world[:, :3])).cuda()
    gt_dict = {i: p for i, p in enumerate(gt_world)}
    world = chain_poses(rel)

    def device():
        aligned, transform = align(gt, world, MODE)
        return aligned, transform, sequence_errors(gt, aligned), trajectory_errors(gt, aligned), snippet_errors(gt, aligned)

    def host():
        res = world.cpu().numpy()
        c, rot, t, sv = oe.trajectory_alignment(gt_world, res, MODE)
        aligned = oe.apply_alignment(res, c, rot, t)
        rows = oe.sequence_errors(gt_dict, {i: p for i, p in enumerate(oe._as44(aligned))})
        return c, aligned, oe.overall_error(rows), oe.trajectory_errors(gt_world, aligned), oe.snippet_errors(gt_world, aligned)

    for _ in range(3):
        aligned, transform, (rows, summary), errors, (srows, ssum) = device()
    hc, haligned, (ht, hr), (hate, hrt, hrr), hsrows = host()
    dt, dr = (float(v) for v in overall(summary))
    e = errors.tolist()
    ssum = ssum.tolist()

    def rel_of(a, b):
        return abs(a - b) / abs(b)

    aerr = float(np.abs(aligned.cpu().numpy() - haligned).max() / np.abs(haligned).max())
    print(f"n = {N}, align {MODE}: scale {float(transform[0]):.9f}, ATE {e[0]:.4f} m, {int(ssum[3])} snippets (host {len(hsrows)}); "
          f"device vs host: c {rel_of(float(transform[0]), hc):.2e}, aligned rel {aerr:.2e}, t_err/len {rel_of(dt, ht):.2e}, "
          f"r_err/len {rel_of(dr, hr):.2e}, ATE {rel_of(e[0], hate):.2e}, RPE_t {rel_of(e[1], hrt):.2e}, RPE_r {rel_of(e[2], hrr):.2e}, "
          f"snippet ATE {rel_of(ssum[0] / ssum[3], float(hsrows[:, 0].mean())):.2e}, "
          f"snippet re {rel_of(ssum[2] / ssum[3], float(hsrows[:, 1].mean())):.2e}", flush=True)
    med, lo, hi = _events(device, iters, reps)
    parts = (("align (4 launches: sums, centred sums, solve, apply)", lambda: align(gt, world, MODE)),
             ("sequence_errors (3 launches)", lambda: sequence_errors(gt, aligned)),
             ("trajectory_errors (2 launches: pairs, finish)", lambda: trajectory_errors(gt, aligned)),
             (f"snippet_errors (2 launches: {srows.shape[0]} rows, finish)", lambda: snippet_errors(gt, aligned)))
    alone = [(name,) + _events(fn, iters, reps) for name, fn in parts]
    hmed, hlo, hhi = _wall(host, min(iters, 5))
    print(f"device align + sequence_errors + trajectory_errors + snippet_errors: {med * 1e3:9.1f} us per pass (events, median of "
          f"{iters} x {reps}; min {lo * 1e3:.1f}, max {hi * 1e3:.1f}), 11 launches", flush=True)
    for name, m, l, h in alone:
        print(f"  {name + ' alone:':66s}{m * 1e3:9.1f} us (min {l * 1e3:.1f}, max {h * 1e3:.1f})", flush=True)
    print(f"host copy + trajectory_alignment + apply_alignment + sequence_errors + trajectory_errors + snippet_errors: "
          f"{hmed * 1e3:9.1f} us per pass (wall clock, median of {min(iters, 5)}; min {hlo * 1e3:.1f}, max {hhi * 1e3:.1f}); "
          f"ratio {hmed / med:.0f}x", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
