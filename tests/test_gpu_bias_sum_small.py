"""The bias-only path of dvf_act_bwd (y = dpre = NULL: bias_sum_kernel, the pass behind the weight gradient of every
transposed layer): per-channel sums of one tensor against a float64 CPU sum (max-abs error / max-abs of the reference
<= 1e-4).  Shapes: one element per thread and fewer (1, 1, 7); the 16-byte path (4, 16, 1024); HW % 4 != 0 (2, 37, 8196);
several chunks per plane (3, 2, 24577); one channel with many blocks on one address (4, 1, 212992).  Every shape also
runs from a base pointer misaligned by one float (the scalar-load variant), with accumulate_dbias 0 and 1; the ordered
mode (scratch of dvf_act_bwd_ws_floats) is bit-identical across two runs.  One case goes through dvf_conv2d_wgrad of a
transposed 3x3 stride-2 layer, whose weight-gradient kernel leaves the bias to this pass."""
import ctypes

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
SHAPES = ((1, 1, 7), (4, 16, 1024), (2, 37, 8196), (3, 2, 24577), (4, 1, 212992))


def _dev_at_offset(x, offset):
    """x on the device; offset = 1: a contiguous view one float into its storage (not 16-byte aligned)."""
    if offset:
        return torch.empty(x.numel() + 1, device=DEV)[1:].view(x.shape).copy_(x)
    return x.to(DEV)


@pytest.mark.parametrize("offset", (0, 1), ids=("aligned", "offset1"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bias_sum(shape, offset):
    from dvf import lib as L
    lib = L.lib()
    n, c, hw = shape
    gen = torch.Generator().manual_seed(n * 1000003 + c * 1009 + hw)
    dy = torch.randn(n, c, hw, generator=gen) + 0.25
    db0 = torch.randn(c, generator=gen)
    ref = dy.double().sum(dim=(0, 2))
    gdy = _dev_at_offset(dy, offset)
    assert (gdy.data_ptr() % 16 == 0) == (offset == 0)
    need = int(lib.dvf_act_bwd_ws_floats(n, c, hw))
    assert need >= c, need
    ws = torch.empty(need, device=DEV)

    def run(acc, ordered):
        db = db0.to(DEV) if acc else torch.full((c,), 7.0, device=DEV)
        L.check(lib.dvf_act_bwd(gdy.data_ptr(), None, None, db.data_ptr(), n, c, hw, L.ACT_NONE, 1.0, 0.0, acc,
                                ws.data_ptr() if ordered else None, need if ordered else 0, L.stream_raw()), "dvf_act_bwd")
        torch.cuda.synchronize()
        return db.cpu()

    for acc in (0, 1):
        want = ref + db0.double() if acc else ref
        atomic = run(acc, False)
        e = rel_err(atomic, want)
        print(f"bias_sum {shape} offset {offset} acc {acc}: atomic rel err {e:.2e}")
        assert e <= TOL, (shape, offset, acc, e)
        o1, o2 = run(acc, True), run(acc, True)
        assert torch.equal(o1, o2), (shape, offset, acc, float((o1 - o2).abs().max()))
        assert rel_err(o1, want) <= TOL, (shape, offset, acc, rel_err(o1, want))


def test_transposed_layer_bias_through_wgrad():
    """ConvTranspose2d(8, 4, 3, stride 2, pad 1, output_padding 1), 5x9 -> 10x18, N = 2: dvf_conv2d_wgrad returns dbias (and
    dw) of torch's float64 CPU autograd."""
    from dvf import lib as L
    lib = L.lib()
    n, cin, cout, h, w = 2, 8, 4, 5, 9
    oh, ow = 2 * h, 2 * w
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(n, cin, h, w, generator=gen)
    dpre = torch.randn(n, cout, oh, ow, generator=gen) + 0.25
    wt = torch.randn(cin, cout, 3, 3, generator=gen, dtype=torch.float64).requires_grad_(True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv_transpose2d(x.double(), wt, b, stride=2, padding=1, output_padding=1)
    assert tuple(y.shape) == (n, cout, oh, ow)
    y.backward(dpre.double())
    desc = L.ConvDesc(n, cin, h, w, cout, oh, ow, 3, 3, 2, 1, 1, L.ACT_NONE, 1.0, 0.0)
    segarr = L.int_array([cin])
    gx, gd = x.to(DEV), dpre.to(DEV)
    inarr = (ctypes.c_void_p * 1)(gx.data_ptr())
    need = max(int(lib.dvf_conv2d_wgrad_ws_floats(ctypes.byref(desc), segarr, 1)), 1)
    ws = torch.empty(need, device=DEV)
    for ordered in (False, True):
        dw = torch.full((cin, cout, 3, 3), 7.0, device=DEV)
        db = torch.full((cout,), 7.0, device=DEV)
        L.check(lib.dvf_conv2d_wgrad(ctypes.byref(desc), inarr, segarr, 1, gd.data_ptr(), dw.data_ptr(), 0, db.data_ptr(), 0,
                                     ws.data_ptr() if ordered else None, need if ordered else 0, L.stream_raw()),
                "dvf_conv2d_wgrad")
        torch.cuda.synchronize()
        eb, ew = rel_err(db, b.grad), rel_err(dw, wt.grad)
        print(f"transposed 3x3 s2 8->4 ordered {ordered}: dbias rel err {eb:.2e}, dw rel err {ew:.2e}")
        assert eb <= TOL, (ordered, eb)
        assert ew <= TOL, (ordered, ew)
