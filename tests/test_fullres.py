"""CPU-side checks of full-resolution multi-scale sampling: the properties of the torch restatement (tests/fullres_ref.py)
that the kernel design of csrc/upsample.hip relies on, and the C ABI / host plumbing as far as it goes without a GPU."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import fullres_ref as FR
from conftest import PKG
from dvf import lib as L

FACTORS = (2, 4, 8)
COARSE = [(1, 1), (2, 3), (5, 7), (9, 33)]


def test_abi_has_the_upsample_entries_and_rejects_bad_arguments_without_touching_the_gpu():
    lib = L.lib()
    for name in ("dvf_upsample_int_fwd", "dvf_upsample_int_bwd"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    fake = ctypes.c_void_p(0x1000)          # recorded, never dereferenced: every call below returns before a launch
    fwd = lambda i, o, p, h, w, f, r=0: lib.dvf_upsample_int_fwd(i, o, p, h, w, f, r, 0.0, None)      # noqa: E731
    bwd = lambda g, o, gi, p, h, w, f, r=0: lib.dvf_upsample_int_bwd(g, o, gi, p, h, w, f, r, None)   # noqa: E731
    assert fwd(None, fake, 1, 4, 4, 2) == -1 and fwd(fake, None, 1, 4, 4, 2) == -1
    assert bwd(None, fake, fake, 1, 4, 4, 2) == -1 and bwd(fake, fake, None, 1, 4, 4, 2) == -1
    assert bwd(fake, None, fake, 1, 4, 4, 2, 1) == -1           # the reciprocal's backward needs the saved output
    for f in (0, 1, 3, 16, -2):
        assert fwd(fake, fake, 1, 4, 4, f) == L.ERR_UNSUPPORTED and bwd(fake, fake, fake, 1, 4, 4, f) == L.ERR_UNSUPPORTED
    for p, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4)):
        assert fwd(fake, fake, p, h, w, 2) == -1 and bwd(fake, fake, fake, p, h, w, 2) == -1
    # fine pixels are indexed in 32 bits: 2^31 of them are refused (8 * 1024 * 1024 coarse pixels x 64 x 4 planes)
    assert fwd(fake, fake, 4, 8192, 1024, 8) == -1 and bwd(fake, fake, fake, 4, 8192, 1024, 8) == -1
    assert fwd(fake, fake, 1 << 20, 1 << 10, 1 << 10, 2) == -1


def test_abi_has_the_ordered_inverse_warp_backward():
    """Host side of the deterministic pose reduction: the scratch size is one 12-float record per 64x4 block plus the B
    sums, and a pose gradient without a scratch is refused before anything is launched."""
    lib = L.lib()
    for name in ("dvf_inverse_warp_ordered_ws_floats", "dvf_inverse_warp_bwd_ordered"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.dvf_inverse_warp_ordered_ws_floats(4, 256, 832) == (13 * 64 * 4 + 4) * 12
    assert lib.dvf_inverse_warp_ordered_ws_floats(0, 256, 832) == 0
    fake = ctypes.c_void_p(0x1000)
    assert lib.dvf_inverse_warp_bwd_ordered(fake, fake, fake, fake, fake, fake, None, fake, fake, None, 1, 3, 8, 8, 0, None) == -1
    assert lib.dvf_inverse_warp_bwd_ordered(None, fake, fake, fake, fake, fake, None, fake, fake, fake, 1, 3, 8, 8, 0, None) == -1


def test_full_resolution_refuses_other_ratios_before_any_device_call():
    """3x, unequal ratios in H and W, 16x and a size that does not divide raise ValueError naming the sizes -- on CPU tensors,
    so nothing was launched; a supported ratio then gets as far as the device check (no CPU fallback)."""
    import loss_functions_sfm as LS
    ok = torch.rand(1, 1, 8, 16)
    cases = [((2, 4), (6, 12)),          # 3x
             ((4, 4), (8, 16)),          # 2x in H, 4x in W
             ((1, 2), (16, 32)),         # 16x
             ((5, 10), (8, 16)),         # does not divide
             ((16, 32), (8, 16))]        # larger than the target
    for (h, w), out_hw in cases:
        bad = torch.rand(1, 1, h, w)
        for maps in (bad, [bad], [torch.rand(1, 1, *out_hw), bad]):
            with pytest.raises(ValueError) as e:
                LS.full_resolution(maps, out_hw)
            assert str((1, 1, h, w)) in str(e.value) and str(out_hw) in str(e.value)
    assert LS.full_resolution([ok], (8, 16))[0] is ok                                         # factor 1, plain: as it is
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LS.full_resolution([torch.rand(1, 1, 4, 8)], (8, 16))


@pytest.mark.parametrize("factor", FACTORS)
def test_restatement_preserves_constants_and_is_a_partition_of_unity(factor):
    """Every fine pixel's four weights sum to 1 (constants are preserved, exactly: the weights are multiples of 1/(2 factor)
    per axis) and so the transpose of a constant gout sums to factor^2 per coarse pixel on average: sum(gin) = sum(gout)."""
    for h, w in COARSE:
        x = torch.full((2, 3, h, w), 3.25, dtype=torch.float64, requires_grad=True)
        up = FR.upsample(x, (factor * h, factor * w))
        assert tuple(up.shape) == (2, 3, factor * h, factor * w) and torch.equal(up.detach(), torch.full_like(up, 3.25))
        up.backward(torch.full_like(up, 2.0))
        per_plane = x.grad.sum((2, 3))
        assert torch.equal(per_plane, torch.full_like(per_plane, 2.0 * factor * factor * h * w))
        # interior coarse pixels get exactly factor^2; the borders collect the clamped taps on top of that
        if h > 2 and w > 2:
            inner = x.grad[:, :, 1:-1, 1:-1]
            assert torch.equal(inner, torch.full_like(inner, 2.0 * factor * factor))


def test_restatement_factor_one_is_the_identity_and_depth_is_taken_at_the_fine_resolution():
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(2, 1, 5, 7, generator=gen, dtype=torch.float64) + 0.1
    assert torch.equal(FR.upsample(x, (5, 7)), x)
    assert torch.equal(FR.upsample_depth(x, (5, 7), 0.0), 1.0 / x)
    d = FR.upsample_depth(x, (20, 28), 1e-4)
    assert torch.equal(d, 1.0 / (FR.upsample(x, (20, 28)) + 1e-4))
    assert not torch.allclose(d, FR.upsample(1.0 / (x + 1e-4), (20, 28)))       # not the upsampled coarse depth


@pytest.mark.parametrize("factor", FACTORS)
def test_integer_operands_make_fp32_exact(factor):
    """The premise of the GPU suite's bit-exact pin: with integer inputs in [-64, 64] and integer output gradients in [-8, 8]
    torch's own fp32 path equals fp64, forward and backward, at the shapes that test uses."""
    gen = torch.Generator().manual_seed(factor)
    for h, w in COARSE:
        x = torch.randint(-64, 65, (6, 1, h, w), generator=gen).double()
        g = torch.randint(-8, 9, (6, 1, factor * h, factor * w), generator=gen).double()
        res = []
        for dt in (torch.float32, torch.float64):
            xr = x.to(dt).requires_grad_(True)
            up = FR.upsample(xr, (factor * h, factor * w))
            up.backward(g.to(dt))
            res.append((up.detach().double(), xr.grad.double()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_entry_scripts_list_the_flag_and_single_scale_ones_refuse_it():
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--full-res-multiscale" in r.stdout, r.stderr[-2000:]
    for script in ("unsupervise.py", "unsupervise_dvo.py"):
        r = subprocess.run([sys.executable, os.path.join(PKG, script), "--full-res-multiscale"], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode != 0 and "--full-res-multiscale needs a multi-scale loss" in r.stderr, (script, r.stderr[-2000:])


def test_step_keyword_and_cli_helper_exist():
    import inspect
    from argparse import Namespace
    from dvf import cli
    from dvf.steps import train_sfm_losses
    assert inspect.signature(train_sfm_losses).parameters["full_res_multiscale"].default is False
    assert cli.fullres_kwargs(Namespace(full_res_multiscale=True)) == {"full_res_multiscale": True}
    assert cli.fullres_kwargs(Namespace(full_res_multiscale=False), multiscale=False) == {}
    with pytest.raises(ValueError, match="single scale"):
        cli.fullres_kwargs(Namespace(full_res_multiscale=True), multiscale=False)
