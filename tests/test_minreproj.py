"""CPU-side checks of the per-pixel minimum-reprojection term: the torch restatement the HIP kernels are tested against
(tests/minreproj_ref.py) is itself checked against finite differences and against its defining properties, and the C ABI /
host plumbing is checked as far as it goes without a GPU."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import minreproj_ref as MR
import ssim_ref
from conftest import PKG
from dvf import lib as L


def _case(b, c, h, w, v, auto, seed, zero_pixels=()):
    """fp64 target, v warped references with the given pixels exactly zero in all channels (via a fixed 0/1 ``keep``, so
    they stay zero under a finite-difference perturbation), and v identity references when ``auto``."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(b, c, h, w, generator=gen, dtype=torch.float64)
    warped = [torch.rand(b, c, h, w, generator=gen, dtype=torch.float64) for _ in range(v)]
    identity = [torch.rand(b, c, h, w, generator=gen, dtype=torch.float64) for _ in range(v if auto else 0)]
    keep = torch.ones(v, b, 1, h, w, dtype=torch.float64)
    for (k, bi, yi, xi) in zero_pixels:
        keep[k, bi, 0, yi, xi] = 0
    return x, warped, identity, keep


def _margin(e, usable):
    """fp64 gap between the best and the second-best usable candidate per pixel (inf where fewer than two are usable)."""
    s = torch.where(usable, e, torch.full_like(e, float("inf"))).sort(0).values
    if s.shape[0] < 2:
        return torch.full_like(s[0], float("inf"))
    return torch.nan_to_num(s[1] - s[0], nan=float("inf"))


@pytest.mark.parametrize("b,c,h,w,v,auto,zero_pixels", [
    (1, 1, 3, 3, 1, True, [(0, 0, 1, 1)]),                               # every window touches all four borders
    (1, 2, 3, 7, 2, False, [(0, 0, 0, 0), (1, 0, 0, 0), (1, 0, 1, 3)]),   # pixel (0, 0) has no usable candidate
    (2, 3, 6, 7, 2, True, [(0, 0, 2, 3), (1, 1, 0, 6), (0, 1, 5, 0)]),    # interior windows, four candidates
])
def test_restatement_passes_gradcheck(b, c, h, w, v, auto, zero_pixels):
    """fp64 autograd of the restatement against finite differences, for the target and every warped reference.  The selection
    is piecewise constant, so the case must sit inside one piece: every pixel's margin between its best and second-best
    usable candidate is far above what the finite-difference step (1e-7) can move, as is every |x - y| from its kink, and
    the clamp is inactive."""
    x, warped, identity, keep = _case(b, c, h, w, v, auto, seed=7 * h + w, zero_pixels=zero_pixels)
    ws = [y * keep[k] for k, y in enumerate(warped)]
    for alpha in (0.85, 1.0, 0.0):
        e, usable = MR.candidate_errors(x, ws, identity, alpha)
        assert float(_margin(e, usable).min()) > 1e-5
    for y in ws + identity:
        d = ssim_ref.dssim(x, y)
        assert float(d.min()) > 1e-3 and float(d.max()) < 1 - 1e-3
    for k, y in enumerate(warped):
        assert float(((x - y).abs() + (1 - keep[k])).min()) > 1e-5
    select = MR.minreproj_loss(x, ws, identity)[1]
    assert int((select == MR.NONE).sum()) == (1 if not auto and len(zero_pixels) == 3 else 0)
    for alpha in (0.85, 1.0, 0.0):
        fn = lambda xx, *yy: MR.minreproj_loss(xx, [y * keep[k] for k, y in enumerate(yy)], identity, alpha)[0]   # noqa: E731
        assert torch.autograd.gradcheck(fn, [t.clone().requires_grad_(True) for t in [x] + warped], eps=1e-7, atol=1e-7,
                                        rtol=1e-5)
    fn = lambda xx, *yy: MR.minreproj_loss(xx, [y * keep[k] for k, y in enumerate(yy)], identity, 0.85, 3e-4, 2e-3, 0.5)[0]  # noqa: E731
    assert torch.autograd.gradcheck(fn, [t.clone().requires_grad_(True) for t in [x] + warped], eps=1e-7, atol=1e-7, rtol=1e-5)


def test_one_view_without_auto_mask_is_the_ssim_l1_loss():
    x, warped, _, keep = _case(2, 3, 6, 7, 1, False, seed=3, zero_pixels=[(0, 0, 2, 3), (0, 1, 0, 0)])
    y = warped[0] * keep[0]
    for alpha in (0.0, 0.85, 1.0):
        for in_scale in (1.0, 0.5):
            got, select = MR.minreproj_loss(x, [y], (), alpha, in_scale=in_scale)
            ref = ssim_ref.ssim_l1_loss(x, y, None, alpha, in_scale=in_scale)
            assert abs(float(got) - float(ref)) <= 1e-15 * abs(float(ref)) + 1e-18
            assert int((select == MR.NONE).sum()) == 2 and int((select == 0).sum()) == 2 * 6 * 7 - 2


def test_tie_goes_to_the_lowest_index_and_to_a_warped_view_before_an_identity_one():
    x, warped, _, keep = _case(2, 3, 6, 7, 1, False, seed=4, zero_pixels=[(0, 1, 4, 2)])
    y = warped[0] * keep[0]
    # two identical warped candidates: candidate 0 wins every usable pixel
    select = MR.minreproj_loss(x, [y, y.clone()])[1]
    assert int((select == 0).sum()) == 2 * 6 * 7 - 1 and int((select == MR.NONE).sum()) == 1 and int((select == 1).sum()) == 0
    # the identity candidate equals the warped one: the warped one wins wherever it is usable, the identity one (always
    # usable) only where the warped pixel is exactly zero
    loss, select = MR.minreproj_loss(x, [y], [y.clone()])
    assert int((select == 0).sum()) == 2 * 6 * 7 - 1 and int(select[1, 4, 2]) == 1
    # ... and that pixel's identity value is part of the loss
    assert float(loss) > float(MR.minreproj_loss(x, [y])[0])


def test_pixel_without_usable_candidate_adds_nothing_and_stays_in_the_denominator():
    x, warped, _, keep = _case(1, 2, 5, 6, 2, False, seed=5, zero_pixels=[(0, 0, 2, 3), (1, 0, 2, 3)])
    ws = [y * keep[k] for k, y in enumerate(warped)]
    loss, select = MR.minreproj_loss(x, ws)
    assert int(select[0, 2, 3]) == MR.NONE and int((select == MR.NONE).sum()) == 1
    e, _ = MR.candidate_errors(x, ws)
    best = e.min(0).values                       # (every other pixel has both candidates usable)
    best[0, 2, 3] = 0
    assert abs(float(loss) - float(best.sum()) / 30) < 1e-15
    # nothing usable anywhere: the loss is exactly zero
    zero = [torch.zeros_like(y) for y in ws]
    loss, select = MR.minreproj_loss(x, zero)
    assert float(loss) == 0 and bool((select == MR.NONE).all())


def test_abi_has_the_minreproj_entries():
    lib = L.lib()
    for name in ("dvf_minreproj_partials_floats", "dvf_minreproj_fwd", "dvf_minreproj_bwd"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    # 13 x 16 tiles x 4 images, one loss partial and K + 1 counts each
    assert lib.dvf_minreproj_partials_floats(4, 256, 832, 4) == 4 * 16 * 13 * 6
    assert lib.dvf_minreproj_partials_floats(4, 256, 832, 0) == 0 and lib.dvf_minreproj_partials_floats(4, 256, 832, 9) == 0


def test_abi_rejects_bad_arguments_without_touching_the_gpu():
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)          # recorded, never dereferenced: every call below returns before a launch
    ptrs = lambda n: (ctypes.c_void_p * 8)(*([0x1000] * n))     # noqa: E731  (host array; entries past n are null)
    f = (1.0, 0.85, 1e-4, 9e-4)
    fwd = lambda tgt, cands, v, auto, b, c, h, w: lib.dvf_minreproj_fwd(tgt, cands, v, auto, fake, fake, fake, fake, b, c, h, w,  # noqa: E731
                                                                         *f, 0, None)
    bwd = lambda tgt, cands, v, auto, b, c, h, w: lib.dvf_minreproj_bwd(tgt, cands, v, auto, fake, fake, fake, ptrs(4), b, c, h,  # noqa: E731
                                                                         w, *f, None)
    assert lib.dvf_minreproj_fwd(None, None, 1, 0, None, None, None, None, 1, 3, 8, 8, *f, 0, None) == -1
    assert lib.dvf_minreproj_bwd(None, None, 1, 0, None, None, None, None, 1, 3, 8, 8, *f, None) == -1
    for call in (fwd, bwd):
        assert call(None, ptrs(2), 2, 0, 1, 3, 8, 8) == -1          # null target
        assert call(fake, None, 2, 0, 1, 3, 8, 8) == -1             # null candidate array
        assert call(fake, ptrs(1), 2, 0, 1, 3, 8, 8) == -1          # second view missing
        assert call(fake, ptrs(2), 2, 1, 1, 3, 8, 8) == -1          # auto-mask: the identity candidates are missing
        assert call(fake, ptrs(8), 0, 0, 1, 3, 8, 8) == -1          # V = 0
        assert call(fake, ptrs(8), 5, 0, 1, 3, 8, 8) == -1          # V = 5
        assert call(fake, ptrs(2), 2, 0, 1, 3, 2, 8) == -1          # H = 2
        assert call(fake, ptrs(2), 2, 0, 1, 3, 8, 2) == -1          # W = 2
        assert call(fake, ptrs(2), 2, 0, 65536, 3, 8, 8) == -1      # B
        assert call(fake, ptrs(2), 2, 0, 1, 2048, 1024, 1024) == -1  # C*H*W >= 2^31
    assert lib.dvf_minreproj_fwd(fake, ptrs(2), 2, 0, fake, None, fake, fake, 1, 3, 8, 8, *f, 0, None) == -1   # no selection map
    assert lib.dvf_minreproj_fwd(fake, ptrs(2), 2, 0, fake, fake, None, fake, 1, 3, 8, 8, *f, 0, None) == -1   # no counts
    assert lib.dvf_minreproj_bwd(fake, ptrs(2), 2, 0, None, fake, fake, ptrs(2), 1, 3, 8, 8, *f, None) == -1   # no selection map
    # nothing to write: returns before any launch
    assert lib.dvf_minreproj_bwd(fake, ptrs(2), 2, 0, fake, fake, None, None, 1, 3, 8, 8, *f, None) == 0


def test_wrapper_refuses_cpu_tensors_and_bad_candidates():
    """There is no eager fallback: CPU tensors raise like on every other product path; shape mismatches, more than four views
    and an identity source that wants a gradient raise before anything is launched."""
    import loss_functions
    import loss_functions_sfm
    from dvf.ops import MinReprojLossFn
    b, h, w = 1, 16, 32
    img = [torch.rand(b, 3, h, w) for _ in range(6)]
    cfg = (1.0, 0.85, 1e-4, 9e-4, False)
    auto = cfg[:4] + (True,)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MinReprojLossFn.apply(img[0], cfg, 2, img[1], img[2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MinReprojLossFn.apply(img[0], auto, 1, img[1], img[2])
    with pytest.raises(ValueError, match="n_views"):
        MinReprojLossFn.apply(img[0], cfg, 5, *img[1:6])
    with pytest.raises(ValueError, match="candidates"):
        MinReprojLossFn.apply(img[0], auto, 2, img[1], img[2])             # auto-mask without the identity candidates
    with pytest.raises(ValueError, match="does not match"):
        MinReprojLossFn.apply(img[0], cfg, 2, img[1], torch.rand(b, 3, h, w + 1))
    with pytest.raises(ValueError, match="identity"):
        MinReprojLossFn.apply(img[0], auto, 1, img[1], img[2].clone().requires_grad_(True))
    K = torch.eye(3).expand(b, 3, 3).contiguous()
    depth = torch.rand(b, 1, h, w) + 1
    pose = torch.zeros(b, 2, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_functions_sfm.photometric_reconstruction_loss(img[0], img[1:3], K, K, [depth], [None], pose, ssim_weight=0.85,
                                                           min_reprojection=True, auto_mask=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_functions.photometric_reconstruction_loss(img[0], img[1], img[2], depth[:, 0], pose[:, 0], pose[:, 1], K, K,
                                                       min_reprojection=True)


def test_mode_keywords_are_checked():
    """auto_mask needs min_reprojection; the explainability mask is not part of the mode (neither a mask tensor in the
    photometric loss nor w2 > 0 in the step)."""
    import loss_functions
    import loss_functions_sfm
    from dvf.steps import train_sfm_losses
    b, h, w = 1, 16, 32
    img = [torch.rand(b, 3, h, w) for _ in range(3)]
    K = torch.eye(3).expand(b, 3, 3).contiguous()
    depth = torch.rand(b, 1, h, w) + 1
    pose = torch.zeros(b, 2, 6)
    with pytest.raises(ValueError, match="auto_mask"):
        loss_functions_sfm.photometric_reconstruction_loss(img[0], img[1:], K, K, [depth], [None], pose, auto_mask=True)
    with pytest.raises(ValueError, match="auto_mask"):
        loss_functions.photometric_reconstruction_loss(img[0], img[1], img[2], depth[:, 0], pose[:, 0], pose[:, 1], K, K,
                                                       auto_mask=True)
    with pytest.raises(ValueError, match="explainability mask"):
        loss_functions_sfm.photometric_reconstruction_loss(img[0], img[1:], K, K, [depth, depth], [None, torch.rand(b, 2, h, w)],
                                                           pose, min_reprojection=True)
    with pytest.raises(ValueError, match="w2 must be 0"):
        train_sfm_losses(None, None, {}, w2=0.2, min_reprojection=True)


@pytest.mark.parametrize("script", ["train.py", "unsupervise.py"])
def test_entry_scripts_list_the_minreproj_flags(script):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--min-reprojection", "--auto-mask"):
        assert flag in r.stdout, flag
