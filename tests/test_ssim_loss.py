"""CPU-side checks of the opt-in SSIM + L1 appearance term: the torch restatement the HIP kernels are tested against
(tests/ssim_ref.py) is itself checked against finite differences, and the C ABI / host plumbing is checked as far as it
goes without a GPU."""
import os
import subprocess
import sys

import pytest
import torch

import ssim_ref
from conftest import PKG
from dvf import lib as L


def _case(b, c, h, w, seed, zero_pixels):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(b, c, h, w, generator=gen, dtype=torch.float64)
    y = torch.rand(b, c, h, w, generator=gen, dtype=torch.float64)
    m = torch.rand(b, 1, h, w, generator=gen, dtype=torch.float64) * 0.9 + 0.05
    keep = torch.ones(b, 1, h, w, dtype=torch.float64)
    for (bi, yi, xi) in zero_pixels:
        keep[bi, 0, yi, xi] = 0
    return x, y, m, keep


@pytest.mark.parametrize("b,c,h,w,zero_pixels", [
    (1, 1, 3, 3, [(0, 1, 1)]),                      # every window touches all four borders
    (1, 2, 3, 7, [(0, 0, 0), (0, 1, 3)]),           # every window touches top and bottom
    (2, 3, 6, 7, [(0, 2, 3), (1, 0, 6), (1, 5, 0)]),  # interior windows as well
])
def test_restatement_passes_gradcheck(b, c, h, w, zero_pixels):
    """fp64 autograd of the restatement against finite differences, for x, y and the mask.  The warped image has pixels
    that are exactly zero in all channels (validity 0).  Validity is a step function of y, so y enters as y_free * keep
    with a fixed 0/1 `keep`: the zeroed pixels stay zero under the finite-difference perturbation, while the gradient
    reaching every other pixel -- through windows that contain zeroed neighbours too -- is checked."""
    x, y, m, keep = _case(b, c, h, w, seed=h * 10 + w, zero_pixels=zero_pixels)
    assert float((ssim_ref.valid_mask(y * keep) == 0).sum()) == len(zero_pixels)
    # random images: no |x - y| kink within the step, no active clamp
    d = ssim_ref.dssim(x, y * keep)
    assert float(d.min()) > 1e-3 and float(d.max()) < 1 - 1e-3 and float((x - y * keep).abs().min()) > 1e-5
    for alpha in (0.85, 1.0, 0.0):
        fn = lambda xx, yy, mm: ssim_ref.ssim_l1_loss(xx, yy * keep, mm, alpha=alpha)     # noqa: E731
        assert torch.autograd.gradcheck(fn, [t.clone().requires_grad_(True) for t in (x, y, m)], eps=1e-7, atol=1e-7,
                                        rtol=1e-5)
    fn = lambda xx, yy: ssim_ref.ssim_l1_loss(xx, yy * keep, None, in_scale=0.5, c1=3e-4, c2=2e-3)       # noqa: E731
    assert torch.autograd.gradcheck(fn, [t.clone().requires_grad_(True) for t in (x, y)], eps=1e-7, atol=1e-7, rtol=1e-5)


def test_identical_images_have_no_structural_loss():
    gen = torch.Generator().manual_seed(3)
    for dt in (torch.float32, torch.float64):
        x = (torch.rand(2, 3, 9, 11, generator=gen, dtype=dt) + 0.01)
        assert float(ssim_ref.ssim_l1_loss(x, x.clone(), None, alpha=1.0)) <= 1e-6
        assert float(ssim_ref.ssim_l1_loss(x, x.clone(), None, alpha=0.85)) <= 1e-6


def test_reflection_border_is_index_minus_one_to_one():
    x = torch.arange(12.0).reshape(1, 1, 3, 4)
    w = ssim_ref.windows(x)
    assert w[0, 0, 0, 0].tolist() == [5, 4, 5, 1, 0, 1, 5, 4, 5]
    assert w[0, 0, 2, 3].tolist() == [6, 7, 6, 10, 11, 10, 6, 7, 6]


def test_abi_has_the_ssim_entries():
    lib = L.lib()
    for name in ("dvf_ssim_partials_floats", "dvf_ssim_loss_fwd", "dvf_ssim_loss_bwd"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.dvf_ssim_partials_floats(4, 256, 832) > 0


def test_abi_rejects_bad_arguments_without_touching_the_gpu():
    import ctypes
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)          # recorded, never dereferenced: every call below returns before a launch
    assert lib.dvf_ssim_loss_fwd(None, None, None, 0, None, None, 1, 3, 8, 8, 1.0, 0.85, 1e-4, 9e-4, 0, None) == -1
    assert lib.dvf_ssim_loss_bwd(None, None, None, 0, None, None, None, None, 1, 3, 8, 8, 1.0, 0.85, 1e-4, 9e-4, None) == -1
    assert lib.dvf_ssim_loss_fwd(fake, fake, None, 0, fake, fake, 1, 3, 2, 8, 1.0, 0.85, 1e-4, 9e-4, 0, None) == -1      # H = 2
    assert lib.dvf_ssim_loss_fwd(fake, fake, None, 0, fake, fake, 1, 3, 8, 2, 1.0, 0.85, 1e-4, 9e-4, 0, None) == -1      # W = 2
    assert lib.dvf_ssim_loss_bwd(fake, fake, None, 0, fake, fake, fake, None, 1, 3, 2, 8, 1.0, 0.85, 1e-4, 9e-4, None) == -1
    assert lib.dvf_ssim_loss_fwd(fake, fake, None, 0, fake, fake, 65536, 3, 8, 8, 1.0, 0.85, 1e-4, 9e-4, 0, None) == -1  # B
    assert lib.dvf_ssim_loss_fwd(fake, fake, None, 0, fake, fake, 1, 2048, 1024, 1024, 1.0, 0.85, 1e-4, 9e-4, 0, None) == -1
    assert lib.dvf_ssim_loss_fwd(fake, fake, fake, 63, fake, fake, 1, 3, 8, 8, 1.0, 0.85, 1e-4, 9e-4, 0, None) == -1     # mask stride < H*W


def test_ssim_path_refuses_cpu_tensors():
    """ssim_weight > 0 on CPU tensors must raise like every other product path: there is no eager fallback."""
    import loss_functions
    import loss_functions_sfm
    b, h, w = 1, 16, 32
    img = [torch.rand(b, 3, h, w) for _ in range(3)]
    K = torch.eye(3).expand(b, 3, 3).contiguous()
    depth = torch.rand(b, 1, h, w) + 1
    pose = torch.zeros(b, 2, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_functions_sfm.photometric_reconstruction_loss(img[0], img[1:], K, K, [depth], [None], pose, ssim_weight=0.85)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_functions.photometric_reconstruction_loss(img[0], img[1], img[2], depth[:, 0], pose[:, 0], pose[:, 1], K, K,
                                                       ssim_weight=0.85)
    from dvf.ops import SsimL1LossFn
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SsimL1LossFn.apply(img[0], img[1], None, (1.0, 0.85, 1e-4, 9e-4, None))


@pytest.mark.parametrize("script", ["train.py", "unsupervise.py"])
def test_entry_scripts_list_the_ssim_flags(script):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--ssim-weight", "--ssim-c1", "--ssim-c2"):
        assert flag in r.stdout, flag
