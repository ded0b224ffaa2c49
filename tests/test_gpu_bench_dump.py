"""bench.py --dump-outputs: two runs with the same arguments write the same loss terms, weight gradients and updated
weights, and those are the arrays of one training step from the seeded initial state.  Bound between the runs: 1e-4
relative (max-abs error / max-abs reference) per array, fp32 -- a gradient whose sign differs between the runs moves its
weight by 2 * lr, far above it."""
import argparse
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu

B, H, W, LR = 1, 64, 128, 1e-3          # cfg 2 body at a small size; lr of bench.build's cfg-2 optimizer


def _dump(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
           "--height", str(H), "--width", str(W), "--no-graph", "--no-cpu-baseline", "--no-kernel-timing",
           "--dump-outputs", str(out_dir)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def _seeded_nets():
    """The networks as bench.build() initialises them (seeded, on the CPU: nothing has stepped them)."""
    spec = importlib.util.spec_from_file_location("dvf_bench_for_dump_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    args = argparse.Namespace(batch=B, height=H, width=W, seed=0, force_ddp=False, no_graph=True)
    with torch.random.fork_rng():            # build() seeds torch: leave the later tests' random inputs as they were
        return bench.build(args, bench.CONFIGS[2], torch.device("cpu"), 1, 0)[4]


def test_dump_outputs_repeat_across_runs_and_describe_one_step(tmp_path):
    a, b = _dump(tmp_path / "a"), _dump(tmp_path / "b")
    assert a.keys() == b.keys()
    assert {"loss_total", "loss_img", "loss_smooth", "grad_disp.conv1.0.weight", "param_disp.conv1.0.weight"} <= a.keys()
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype == np.float32 and a[k].shape == b[k].shape, k
        assert np.isfinite(a[k]).all(), k
        assert rel_err(a[k], b[k]) <= 1e-4, (k, rel_err(a[k], b[k]))

    # the losses are those of the seeded weights on the seeded batch (CPU oracle).  The image term gets 5e-3: with the
    # xavier-initialised networks many pixels project onto sampler tap or out-of-view boundaries, where fp32 coordinate
    # rounding may fall either way (conftest.safe_pixel_mask); one Adam step moves the losses by ~20 %.
    from oracle import steps as osteps
    nets = _seeded_nets()
    dsd = {k: v.detach().clone() for k, v in nets["disp"].state_dict().items()}
    psd = {k: v.detach().clone() for k, v in nets["pose"].state_dict().items()}
    ref, _, _ = osteps.step_unsupervise(dsd, psd, osteps.synthetic_batch(B, H, W, seed=1234), do_update=False)
    for k, tol in (("img", 5e-3), ("smooth", 1e-4), ("total", 1e-4)):
        assert abs(float(a["loss_" + k]) - float(ref[k])) <= tol * abs(float(ref[k])), (k, float(a["loss_" + k]), float(ref[k]))

    # the weights are the seeded ones after ONE Adam step (from zero moments every weight moves by lr against its gradient)
    checked = 0
    for net_name, net in nets.items():
        for k, p0 in net.state_dict().items():
            p, g = a[f"param_{net_name}.{k}"], a[f"grad_{net_name}.{k}"]
            if p.shape != tuple(p0.shape):
                continue                                                  # sampled: compared between the runs only
            step = p.astype(np.float64) - p0.numpy().astype(np.float64)
            if not g.any():                                               # no gradient (the unused mask decoder): not moved
                assert not step.any(), (net_name, k)
                continue
            assert np.abs(step).max() <= LR * 1.001, (net_name, k, np.abs(step).max())
            big = np.abs(g) > 1e-6                                        # well above Adam's eps: the step is ~lr
            if big.any():
                assert (np.sign(step[big]) == -np.sign(g[big])).all(), (net_name, k)
                assert np.median(np.abs(step[big])) > 0.5 * LR, (net_name, k)
                checked += 1
    assert checked >= 10
