"""The two-stage loss sums past one trip of the finishing block.  Every loss kernel with one float per block ends in the same
one-block launch (csrc/elementwise.hip: sum_partials_kernel; minreproj_reduce_kernel and smooth_reduce_kernel run the same
device helper, csrc/dvf_common.h: block_sum_strided), whose 256 threads stride over the per-block partials.  The parity cases
of the kernels' own test files finish over 1 to 12 blocks, so each caller gets one shape here with 257 to about 320 blocks -- a
second trip for some threads only -- and a ragged last tile on both axes with W % 4 != 0.  Per caller: the loss against the
fp64 restatement its own test file uses, at that file's tolerance and with no pixel excluded; a repeated call is
bit-identical; and a call with accumulate=1 into the same loss_out leaves exactly fl(first + second)."""
import pytest
import torch

import minreproj_ref as MR
import ssim_ref
from conftest import rel_err
from oracle import losses as ol

pytestmark = pytest.mark.gpu
DEV = "cuda"
SSIM_SHAPE = (1, 1, 272, 1025)      # 64x16 tiles: 17 x 17 = 289 blocks
ROW_SHAPE = (70, 1025)              # 64x4 tiles: 17 x 18 = 306 blocks
BCE_SHAPE = (1, 1, 77, 997)         # 76769 elements = 299 blocks of 256 and one of 225 (the launch is capped at 1024 blocks)
MINREPROJ_SEED = 3                  # see test_minreproj
TOL = 1e-4                          # test_gpu_ssim.TOL, test_gpu_minreproj.TOL


def _rand_image(gen, shape, in_scale, zero_share=0.0):
    """Uniform image as the kernels read it (in_scale * value in [0, 1]); zero_share of its pixels are exactly zero in all
    channels (a warped reference's out-of-view pixels)."""
    b, c, h, w = shape
    img = torch.rand(b, c, h, w, generator=gen) / in_scale
    return img * (torch.rand(b, 1, h, w, generator=gen) >= zero_share) if zero_share else img


def _check(call, nblk, ref, tol):
    """call(loss_out, accumulate) launches the forward under test on the current stream."""
    assert 257 <= nblk <= 320
    out, fresh = torch.empty(1, device=DEV), torch.empty(1, device=DEV)
    call(out, 0)
    first = out.cpu()
    call(out, 1)
    call(fresh, 0)
    torch.cuda.synchronize()
    print("blocks", nblk, "loss", float(first), "rel err", rel_err(first, ref))
    assert float(ref) > 0 and rel_err(first, ref) < tol
    assert torch.equal(fresh.cpu(), first)
    assert torch.equal(out.cpu(), first + first)


@pytest.mark.parametrize("in_scale,alpha", [(1.0, 0.85), (0.004, 0.0)])
def test_ssim_l1(in_scale, alpha):
    from dvf import lib as L
    b, c, h, w = SSIM_SHAPE
    gen = torch.Generator().manual_seed(1)
    x, y = _rand_image(gen, SSIM_SHAPE, in_scale), _rand_image(gen, SSIM_SHAPE, in_scale, 0.1)
    ref = ssim_ref.ssim_l1_loss(x.double(), y.double(), None, alpha, 1e-4, 9e-4, in_scale)
    lib, xg, yg = L.lib(), x.to(DEV), y.to(DEV)
    nblk = int(lib.dvf_ssim_partials_floats(b, h, w))
    partials = torch.empty(nblk, device=DEV)
    _check(lambda out, acc: L.check(lib.dvf_ssim_loss_fwd(L.dev(xg), L.dev(yg), None, 0, L.dev(out), L.dev(partials), b, c, h, w,
                                                          in_scale, alpha, 1e-4, 9e-4, acc, L.stream()), "dvf_ssim_loss_fwd"),
           nblk, ref, TOL)


def test_minreproj():
    """Two views with the auto-mask (K = 4 candidates).  Only the loss is compared, and every pixel counts: at a near-tie the
    two candidates' errors differ by less than the tolerance.  With MINREPROJ_SEED the set that test_gpu_minreproj excludes
    from its gradient comparison (dilated near-ties + L1 kink band, cap 5 %) is 0.92 % of these elements (CPU, fp64):
    an input that file's tests would accept."""
    from dvf import lib as L
    b, c, h, w = SSIM_SHAPE
    in_scale, alpha, v = 1.0, 0.85, 2
    gen = torch.Generator().manual_seed(MINREPROJ_SEED)
    x = _rand_image(gen, SSIM_SHAPE, in_scale)
    warped = [_rand_image(gen, SSIM_SHAPE, in_scale, 0.1) for _ in range(v)]
    identity = [_rand_image(gen, SSIM_SHAPE, in_scale) for _ in range(v)]
    ref, _ = MR.minreproj_loss(x.double(), [t.double() for t in warped], [t.double() for t in identity], alpha, 1e-4, 9e-4,
                               in_scale)
    lib, xg, cands = L.lib(), x.to(DEV), [t.to(DEV) for t in warped + identity]
    k = len(cands)
    floats = int(lib.dvf_minreproj_partials_floats(b, h, w, k))
    partials = torch.empty(floats, device=DEV)
    select = torch.empty((b, h, w), device=DEV, dtype=torch.uint8)
    counts = torch.empty(k + 1, device=DEV, dtype=torch.int32)
    _check(lambda out, acc: L.check(lib.dvf_minreproj_fwd(L.dev(xg), L.ptr_array(cands), v, 1, L.dev(out), select.data_ptr(),
                                                          counts.data_ptr(), L.dev(partials), b, c, h, w, in_scale, alpha, 1e-4,
                                                          9e-4, acc, L.stream()), "dvf_minreproj_fwd"),
           floats // (k + 2), ref, TOL)
    # the integer half of the same finishing block
    assert counts.tolist() == [int((select == i).sum()) for i in range(k)] + [0] and int(counts.sum()) == b * h * w


def test_edge_aware_smoothness():
    from dvf import lib as L
    h, w = ROW_SHAPE
    g = torch.Generator().manual_seed(h)
    D = torch.rand(1, 1, h, w, generator=g) * 3 + 0.01
    I = torch.rand(1, 3, h, w, generator=g) * 255
    ref = ol.edge_aware_smooth_caffe(D.double(), 0.004 * I.double())
    lib, dg, ig = L.lib(), D.to(DEV), I.to(DEV)
    nblk = int(lib.dvf_edge_smooth_partials_floats(1, h, w))
    partials = torch.empty(nblk, device=DEV)
    _check(lambda out, acc: L.check(lib.dvf_edge_smooth_fwd(L.dev(dg), L.dev(ig), L.dev(out), L.dev(partials), 1, 3, h, w, 0.004,
                                                            0.33, 1.0, acc, L.stream()), "dvf_edge_smooth_fwd"),
           nblk, ref, 1e-4)                                   # test_paper_losses.test_edge_smooth_kernel_vs_oracle


def test_second_order_smoothness():
    from dvf import lib as L
    h, w = ROW_SHAPE
    d = torch.rand(1, 1, h, w, generator=torch.Generator().manual_seed(5)) * 10
    ref = ol.smooth_loss(d.double())
    lib, dg = L.lib(), d.to(DEV)
    floats = int(lib.dvf_smooth_partials_floats(1, h, w))
    partials = torch.empty(floats, device=DEV)
    _check(lambda out, acc: L.check(lib.dvf_smooth_loss_fwd(L.dev(dg), L.dev(out), L.dev(partials), 1, h, w, 1.0, acc, L.stream()),
                                    "dvf_smooth_loss_fwd"),
           floats // 4, ref, 1e-5)                            # test_gpu_losses.test_smooth_full_size_properties


def test_explainability_bce():
    from dvf import lib as L
    m = torch.rand(*BCE_SHAPE, generator=torch.Generator().manual_seed(9)) * 0.98 + 0.01
    ref = ol.explainability_loss(m.double())
    n = m.numel()
    assert n % 256 != 0
    lib, mg = L.lib(), m.to(DEV)
    partials = torch.empty(1024, device=DEV)
    _check(lambda out, acc: L.check(lib.dvf_bce_ones_fwd(L.dev(mg), L.dev(out), L.dev(partials), n, acc, L.stream()),
                                    "dvf_bce_ones_fwd"),
           min((n + 255) // 256, 1024), ref, 1e-5)            # test_gpu_losses.test_photometric_sfm_golden
