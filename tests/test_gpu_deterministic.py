"""Deterministic mode (dvf.conv.set_deterministic) beyond the per-layer and per-step parity of test_gpu_bench_shapes.py:
 * the side-stream scratch of the ordered weight-gradient flush: a buffer replaced by a larger one must not be handed to
   the compute stream while side-stream kernels that were not joined yet may still write their slabs into it;
 * a HIP-graph replay of the cfg-2 forward + backward leaves the same gradient arena, bit for bit, as the eager step;
 * the one documented exception -- the photometric backward's source-gradient scatter -- says so when it runs."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_side_stream_scratch_is_not_reused_by_the_compute_stream():
    """A layer whose flush fits the 1<<20-float floor of the side stream's scratch, then one that grows it.  Before the
    streams join, compute-stream allocations of the old buffer's size must not get any of its memory: the caching allocator
    would hand it out at once if the buffer had been allocated under the compute stream (a dgrad output could then be
    written while a side-stream wgrad_pipe still flushes slabs into it).  No timing is involved: the allocator's reuse of a
    freed block is decided on the host."""
    from dvf import conv as C
    from dvf.engine import FlatAdam
    torch.manual_seed(0)
    small = C.FusedConv2d(16, 16, 3, 1, 1).to(DEV)
    large = C.FusedConv2d(64, 64, 3, 1, 1).to(DEV)
    opt = FlatAdam(list(small.parameters()) + list(large.parameters()), lr=1e-3)
    xs = torch.randn(1, 16, 32, 32, device=DEV)
    xl = torch.randn(2, 64, 128, 416, device=DEV)
    held = []
    C.set_deterministic(True)
    try:
        ys, yl = small(xs), large(xl)
        gs, gl = torch.randn_like(ys), torch.randn_like(yl)
        opt.zero_grad()
        torch.cuda.synchronize()
        key = (xs.device, opt.side.cuda_stream)
        C._WS.pop(key, None)                  # (a side stream handle of an earlier test may have left a larger buffer)
        torch.cuda.empty_cache()              # nothing but live tensors left in the pools
        ys.backward(gs)
        old = C._WS[key]
        lo, n = old.data_ptr(), old.numel()
        del old
        assert n == 1 << 20, n
        yl.backward(gl)
        assert C._WS[key].numel() > n, "the larger layer did not grow the side-stream scratch"
        hi = lo + 4 * n
        for i in range(64):
            t = torch.empty(n, device=DEV)
            held.append(t)
            p = t.data_ptr()
            assert p + 4 * n <= lo or p >= hi, (i, hex(p), hex(lo))
    finally:
        opt.join_wgrad()
        torch.cuda.synchronize()
        C.set_deterministic(False)
    assert float(small.weight.grad.abs().max()) > 0 and float(large.weight.grad.abs().max()) > 0


def test_graph_replay_matches_eager_step_bit_for_bit():
    """cfg-2 body at batch 2, 128x416 (the training scripts' default: --deterministic under HIP-graph replay): one replay of
    forward + backward (no optimizer step) leaves the gradient arena of an eager deterministic pass from the same weights,
    bit for bit."""
    import DispNetS
    import PoseExpNet
    from dvf import conv as C
    from dvf import lib as L
    from dvf.engine import FlatAdam, GraphedStep
    from dvf.steps import unsupervise_losses
    from dvf.synthetic import synthetic_batch
    torch.manual_seed(0)
    disp, pose = DispNetS.DispNetS(), PoseExpNet.PoseExpNet(output_exp=True)
    disp.init_weights(); pose.init_weights()
    disp.to(DEV).train(); pose.to(DEV).train()
    # overlap=False: the optimizer mode of the graphed step (bench.py, dvf/cli.py)
    opt = FlatAdam(list(pose.parameters()) + list(disp.parameters()), lr=1e-3, weight_decay=1e-8, overlap=False)
    batch = synthetic_batch(2, 128, 416, seed=1234, device=DEV)

    def fwd_bwd():
        loss, terms = unsupervise_losses(disp, pose, batch)
        opt.zero_grad()
        loss.backward()
        opt.join_wgrad()
        L.join_aux_streams()
        return (terms["total"],)

    C.set_deterministic(True)
    try:
        fwd_bwd()
        torch.cuda.synchronize()
        eager = opt.flat_g.clone()
        graphed = GraphedStep(fwd_bwd, [], warmup=1)
        torch.cuda.synchronize()
        opt.flat_g.fill_(float("nan"))       # the replay's zero_grad and backward must write every slice again
        graphed()
        torch.cuda.synchronize()
        replayed = opt.flat_g.clone()
    finally:
        C.set_deterministic(False)
    assert float(eager.abs().max()) > 0
    assert torch.equal(eager, replayed), float((eager - replayed).abs().max())


def test_source_gradient_scatter_warns_once_in_deterministic_mode():
    """Source-image gradients (the feature term's feature maps) are scattered with float atomics across blocks: the
    first such backward in deterministic mode warns, later ones and the default mode do not."""
    from dvf import conv as C
    from dvf import ops
    b, c, h, w = 1, 4, 16, 32
    gen = torch.Generator().manual_seed(3)
    K = torch.tensor([[w / 2.0, 0.0, w / 2.0], [0.0, h / 2.0, h / 2.0], [0.0, 0.0, 1.0]]).expand(b, 3, 3).contiguous()
    K, Kinv = K.to(DEV), torch.linalg.inv(K).to(DEV)
    depth = (torch.rand(b, h, w, generator=gen) * 5 + 2).to(DEV)
    pose = (torch.randn(2, b, 6, generator=gen) * 0.02).to(DEV)
    tgt = torch.rand(b, c, h, w, generator=gen).to(DEV)

    def backward(src_grad):
        srcs = [torch.rand(b, c, h, w, generator=gen).to(DEV).requires_grad_(src_grad) for _ in range(2)]
        d = depth.clone().requires_grad_(True)
        ops.PhotoLossFn.apply(tgt, d, pose, K, Kinv, None, 0, *srcs).backward()
        torch.cuda.synchronize()
        return srcs

    ops._WARNED_SRC_ATOMICS = False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        backward(True)                       # default mode: silent
    C.set_deterministic(True)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            backward(False)                  # no source gradients: silent
        with pytest.warns(RuntimeWarning, match="float atomics"):
            srcs = backward(True)
        assert all(float(s.grad.abs().max()) > 0 for s in srcs)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            backward(True)                   # once per process
    finally:
        C.set_deterministic(False)
