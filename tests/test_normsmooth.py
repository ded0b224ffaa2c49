"""Edge-aware smoothness of the mean-normalised disparity, CPU side: the torch restatement (tests/normsmooth_ref.py, the
definition of the term) against a hand-computed case and its own invariants, the host checks of the C ABI, and the keyword of
the step bodies.  No GPU is touched."""
import ctypes
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

import normsmooth_ref as NR


def _disp(shape, gen, scales=(1.0, 3.0, 0.2), dt=torch.float64):
    d = 10 * torch.sigmoid(2 * torch.randn(*shape, generator=gen, dtype=dt)) + 0.01
    return d * torch.tensor(scales[:shape[0]], dtype=dt).view(-1, 1, 1, 1)


def test_hand_computed_case():
    """1x1x2x3, mean disparity 2, eps = 0, in_scale 0.5 on an image stored at twice its value:
    n = [[.5, 1, 1.5], [1.5, 1, .5]]; every |dx n| = .5 with wx = e^-1, 1 / 1, e^-2; |dy n| = 1, 0, 1 with wy = 1, e^-1, e^-1."""
    disp = torch.tensor([[[[1.0, 2.0, 3.0], [3.0, 2.0, 1.0]]]], dtype=torch.float64)
    img = torch.tensor([[[[0.0, 2.0, 2.0], [0.0, 0.0, 4.0]]]], dtype=torch.float64)
    e1, e2 = math.exp(-1.0), math.exp(-2.0)
    want = 0.5 * (e1 + 1 + 1 + e2) / 4 + (1 + 0 * e1 + e1) / 3
    got = NR.normalized_smooth_loss(disp, img, in_scale=0.5, eps=0.0)
    assert abs(float(got) - want) < 1e-15
    # the gradient of the same case: A_p / m - T / (m^2 H W) with m = 2, T = want * m
    d = disp.clone().requires_grad_(True)
    NR.normalized_smooth_loss(d, img, in_scale=0.5, eps=0.0).backward()
    cx, cy = 1 / 4, 1 / 3
    A = torch.tensor([[-e1 * cx - 1 * cy, (e1 - 1) * cx + 0 * cy, 1 * cx + e1 * cy],
                      [1 * cx + 1 * cy, (-1 + e2) * cx - 0 * cy, -e2 * cx - e1 * cy]], dtype=torch.float64)
    g = A / 2 - (want * 2) / (4 * 6)
    assert float((d.grad[0, 0] - g).abs().max()) < 1e-15


def test_gradcheck_fp64():
    gen = torch.Generator().manual_seed(1)
    disp = _disp((2, 1, 4, 5), gen, (1.0, 3.0)).requires_grad_(True)
    img = torch.rand(2, 3, 4, 5, generator=gen, dtype=torch.float64) * 2 - 1
    assert torch.autograd.gradcheck(lambda d: NR.normalized_smooth_loss(d, img, 1.0, 1e-7), (disp,))
    assert torch.autograd.gradcheck(lambda d: NR.normalized_smooth_loss(d, img, 0.004 * 127, 0.0), (disp,))


def test_degree_zero_homogeneity():
    """eps = 0: loss(k disp) == loss(disp), and by Euler's theorem sum_p disp_p g_p == 0 for every image on its own."""
    gen = torch.Generator().manual_seed(2)
    disp = _disp((3, 1, 5, 7), gen).requires_grad_(True)
    img = torch.rand(3, 3, 5, 7, generator=gen, dtype=torch.float64) * 2 - 1
    loss = NR.normalized_smooth_loss(disp, img, eps=0.0)
    loss.backward()
    for k in (0.25, 3.0, 1e3):
        assert abs(float(NR.normalized_smooth_loss(k * disp.detach(), img, eps=0.0)) - float(loss)) <= 1e-12 * float(loss)
    dg = (disp.detach() * disp.grad).flatten(1)
    assert float(disp.grad.abs().max()) > 0
    for b in range(3):
        assert abs(float(dg[b].sum())) <= 1e-12 * float(dg[b].abs().sum())


def test_constant_disparity_is_exactly_zero():
    gen = torch.Generator().manual_seed(3)
    img = torch.rand(3, 3, 5, 7, generator=gen) * 2 - 1
    for dt in (torch.float32, torch.float64):
        disp = (torch.tensor([0.5, 7.0, 0.01], dtype=dt).view(3, 1, 1, 1) * torch.ones(3, 1, 5, 7, dtype=dt)).requires_grad_(True)
        loss = NR.normalized_smooth_loss(disp, img.to(dt))
        loss.backward()
        assert float(loss) == 0.0 and float(disp.grad.abs().max()) == 0.0


def test_multiscale_form_is_the_weighted_sum_over_the_area_pyramid():
    gen = torch.Generator().manual_seed(4)
    img = torch.rand(2, 3, 16, 24, generator=gen, dtype=torch.float64)
    disps = [_disp((2, 1, 16 >> s, 24 >> s), gen, (1.0, 3.0)) for s in range(3)]
    want = sum(NR.normalized_smooth_loss(d, img if s == 0 else F.interpolate(img, d.shape[2:], mode="area")) * 0.5 / 2 ** s
               for s, d in enumerate(disps))
    got = NR.multiscale_normalized_smooth_loss(disps, img, scale_factor=2.0, weight=0.5)
    assert abs(float(got) - float(want)) <= 1e-15


def test_host_checks_run_before_any_launch():
    """dvf_norm_smooth_fwd / _bwd return DVF_ERR_INVALID_ARG for null pointers, H = 1, W = 1 (the means over H-1 / W-1 elements
    would be empty) and B = 65536; pointers are not dereferenced (fake non-null ones, as tests/test_abi.py does)."""
    from dvf import lib as L
    lib = L.lib()
    f = ctypes.c_void_p(0x1000)

    def fwd(ptrs, B, C, H, W):
        return lib.dvf_norm_smooth_fwd(*ptrs, B, C, H, W, 1.0, 1e-7, 1.0, 0, None)

    def bwd(ptrs, B, C, H, W):
        return lib.dvf_norm_smooth_bwd(*ptrs, B, C, H, W, 1.0, 1e-7, 1.0, None)

    for call in (fwd, bwd):
        for k in range(5):
            ptrs = [f] * 5
            ptrs[k] = None
            assert call(ptrs, 1, 3, 8, 8) == -1, (call.__name__, k)
        assert call([f] * 5, 1, 3, 1, 8) == -1
        assert call([f] * 5, 1, 3, 8, 1) == -1
        assert call([f] * 5, 65536, 3, 8, 8) == -1
        assert call([f] * 5, 0, 3, 8, 8) == -1
        assert call([f] * 5, 1, 0, 8, 8) == -1
        assert call([f] * 5, 1, 3, 1 << 15, 1 << 15) == -1          # C*H*W >= 2^31
    assert lib.dvf_norm_smooth_partials_floats(2, 17, 65) == 2 * 2 * 2 * 3      # 64x16 tiles, three sums each


def test_step_bodies_take_the_keyword_and_default_to_off():
    from dvf import steps
    for fn in (steps.train_sfm_losses, steps.unsupervise_losses, steps.unsupervise_dvo_losses):
        p = inspect.signature(fn).parameters
        assert "normalized_smoothness" in p and p["normalized_smoothness"].default is False, fn.__name__
    from dvf import cli
    import argparse
    parser = argparse.ArgumentParser()
    cli.add_common_flags(parser)
    assert cli.normsmooth_kwargs(parser.parse_args([])) == {"normalized_smoothness": False}
    assert cli.normsmooth_kwargs(parser.parse_args(["--normalized-smoothness"])) == {"normalized_smoothness": True}


def test_product_refuses_cpu_tensors():
    import loss_functions
    import loss_functions_sfm
    d, img = torch.rand(1, 1, 8, 8) + 0.1, torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_functions.normalized_smooth_loss(d, img)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_functions_sfm.normalized_smooth_loss([d], img)
