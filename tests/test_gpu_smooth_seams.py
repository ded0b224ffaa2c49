"""Second-order smoothness (smooth_fwd_kernel, smooth_reduce_kernel, smooth_bwd_kernel of csrc/warp_loss.hip, through
dvf.ops.SmoothLossFn as loss_functions.smooth_loss and loss_functions_sfm.smooth_loss call it) against
oracle.losses.smooth_loss in fp64: the loss and EVERY element of the gradient, at shapes that put each guard of the
gather-form backward on a tile seam or inside a partial tile (tests/smooth_seams.py::SHAPES names the guards per shape; the
case ids carry the shape), with seeded floats and with integer maps whose second differences are exact and often exactly 0.

Bounds: rel_err < 1e-5 for the loss and the gradient (the bound of test_gpu_losses.py::test_smooth_golden); where the fp64
gradient of an integer map is exactly 0 the kernel's is exactly 0 (tests/test_smooth_seams_inputs.py shows that such an
element is zero term by term); a second run gives the same bits (no atomics).
Measured worst deviations over every case of this file: loss 8.9e-8 (131x3, floats), gradient 7.5e-8 (3x200,
integers)."""
import pytest
import torch

import smooth_seams as S
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
IDS = ["%dx%dx%dx%d" % s for s in S.SHAPES]


def _apis():
    import loss_functions as lf
    import loss_functions_sfm as ls
    return (("loss_functions", lambda maps, f: lf.smooth_loss(maps if len(maps) > 1 else maps[0], f)),
            ("loss_functions_sfm", lambda maps, f: ls.smooth_loss(maps if len(maps) > 1 else maps[0], f)))


def _run(fn, maps, factor):
    leaves = [m.to(DEV).requires_grad_(True) for m in maps]
    loss = fn(leaves, factor)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), [x.grad.cpu() for x in leaves]


def _check(maps, factor, family, tag):
    ref_loss, ref_grads = S.oracle(maps, factor)
    for name, fn in _apis():
        loss, grads = _run(fn, maps, factor)
        loss2, grads2 = _run(fn, maps, factor)
        assert loss.view(torch.int32).equal(loss2.view(torch.int32)), (tag, name, "a second run differs")
        e_loss = rel_err(loss, ref_loss)
        e_grad = max(rel_err(g, r) for g, r in zip(grads, ref_grads))
        print(f"{tag} {family} {name}: loss {float(loss):.6g} rel_err {e_loss:.3g}, gradient rel_err {e_grad:.3g}")
        assert e_loss < TOL, (tag, name, float(loss), float(ref_loss))
        for s, (g, g2, r) in enumerate(zip(grads, grads2, ref_grads)):
            assert g.view(torch.int32).equal(g2.view(torch.int32)), (tag, name, s, "a second run differs")
            assert g.shape == r.shape and rel_err(g, r) < TOL, (tag, name, s, rel_err(g, r))
            if family == "int":
                zero = r == 0
                assert bool((g[zero] == 0).all()), (tag, name, s, "non-zero where the fp64 gradient is exactly 0",
                                                    int((g[zero] != 0).sum()))


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("shape", list(S.SHAPES), ids=IDS)
def test_smooth_at_seams(shape, family):
    """One map of `shape`; S.SHAPES[shape] states the guards of smooth_bwd_kernel / smooth_fwd_kernel it stands for."""
    _check([S.make(shape, family)], 1, family, "%dx%dx%dx%d" % shape)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_smooth_multi_scale_across_a_seam(family):
    """[(5,65), (3,33)] with scale_factor 2: smooth_reduce_kernel's accumulate path on top of a seam-shape result (guards
    x + 1 < W at column 63|64 and y + 1 < H at row 3|4 in the first map, every stencil clipped in y in the second)."""
    _check(S.make_multi(family), 2, family, "multi")
