"""head_wgrad_kernel (the weight gradient of the 1-4 channel 3x3 heads) at small shapes, through dvf_conv2d_wgrad:
C_out in {1, 2, 4} x C_in in {4, 5, 16, 33, 128} (below, at and off the per-thread channel chunk, many chunks) x N in {1, 3}
x H x W in {3x5, 9x37, 16x64, 33x130} (smaller than one unit, no multiple of it in either direction, an exact multiple, and
W % 4 != 0: the scalar-load variant), each with accumulate 0 and 1 onto a non-zero dw, against a float64 CPU sum
(max-abs error / max-abs of the reference <= 1e-4).  With the scratch of dvf_conv2d_wgrad_ws_floats the ordered path runs
(plan note), two runs are bit-identical and within 1e-5 of the atomic path; a scratch one float too small falls back to
the atomics and stays correct."""
import ctypes

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
TOL_DET_VS_ATOMIC = 1e-5

C_OUTS = (1, 2, 4)
C_INS = (4, 5, 16, 33, 128)
NS = (1, 3)
SIZES = ((3, 5), (9, 37), (16, 64), (33, 130))


def _reference(x, dy):
    """dw[m][c][ta][tb] = sum_{n,y,x} dy[n][m][y][x] * x[n][c][y+ta-1][x+tb-1] in float64."""
    n, c, h, w = x.shape
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))
    dyd = dy.double()
    dw = torch.empty(dy.shape[1], c, 3, 3, dtype=torch.float64)
    for ta in range(3):
        for tb in range(3):
            dw[:, :, ta, tb] = torch.einsum("nmyx,ncyx->mc", dyd, xp[:, :, ta:ta + h, tb:tb + w])
    return dw


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cout", C_OUTS)
def test_head_wgrad_small(cout, hw):
    from dvf import lib as L
    lib = L.lib()
    h, w = hw
    gen = torch.Generator().manual_seed(1000 * cout + 10 * h + w)
    for cin in C_INS:
        for n in NS:
            x = torch.randn(n, cin, h, w, generator=gen)
            dy = torch.randn(n, cout, h, w, generator=gen)
            dw0 = torch.randn(cout, cin, 3, 3, generator=gen)
            ref = _reference(x, dy)
            gx, gdy = x.to(DEV), dy.to(DEV)
            desc = L.ConvDesc(n, cin, h, w, cout, h, w, 3, 3, 1, 1, 0, L.ACT_NONE, 1.0, 0.0)
            segarr, inarr = L.int_array([cin]), (ctypes.c_void_p * 1)(gx.data_ptr())
            need = int(lib.dvf_conv2d_wgrad_ws_floats(ctypes.byref(desc), segarr, 1))
            assert need >= cout * cin * 9, need
            ws = torch.empty(need, device=DEV)

            def run(acc, ws_floats):
                dw = dw0.to(DEV) if acc else torch.full((cout, cin, 3, 3), 7.0, device=DEV)
                L.check(lib.dvf_conv2d_wgrad(ctypes.byref(desc), inarr, segarr, 1, gdy.data_ptr(), dw.data_ptr(), acc, None, 0,
                                             ws.data_ptr() if ws_floats else None, ws_floats, L.stream_raw()), "dvf_conv2d_wgrad")
                plans = [(r.kernel, r.C_out, r.ordered) for r in L.last_plans()[0][:1]]
                torch.cuda.synchronize()
                return dw.cpu(), plans

            for acc in (0, 1):
                tag = (cout, cin, n, h, w, acc)
                want = ref + dw0.double() if acc else ref
                atomic, plans = run(acc, 0)
                assert plans and plans[0] == (L.K_HEAD_WGRAD, cout, 0), (tag, plans)
                e = rel_err(atomic, want)
                print(f"head_wgrad {tag}: atomic rel err {e:.2e}")
                assert e <= TOL, (tag, e)
                det1, plans = run(acc, need)
                assert plans and plans[0] == (L.K_HEAD_WGRAD, cout, 1), (tag, plans)
                det2, _ = run(acc, need)
                assert torch.equal(det1, det2), (tag, float((det1 - det2).abs().max()))
                assert rel_err(det1, want) <= TOL, (tag, rel_err(det1, want))
                assert rel_err(det1, atomic) <= TOL_DET_VS_ATOMIC, (tag, rel_err(det1, atomic))
                short, plans = run(acc, need - 1)          # a scratch one float too small: the atomic path, still correct
                assert plans and plans[0] == (L.K_HEAD_WGRAD, cout, 0), (tag, plans)
                assert rel_err(short, want) <= TOL, (tag, rel_err(short, want))
