"""GPU: the bilinear sampler's decisions (csrc/warp_common.h: project, tap_addr / tap_pos, gather / taps_*, blend, blend_grad)
pinned with the exactly representable warps of tests/warp_exact.py.  Every comparison is against the fp64 oracle, unmasked,
with no outlier allowed.  Exact family: warped images and image gradients must EQUAL the oracle (every product and sum is
an fp32 number, so neither the kernel's operation order nor the order of its float atomics can matter); depth and pose
gradients, whose chain divides, within 1e-5.  Mid-cell family (16-byte staging, also at a one-float storage offset) and the
pixel-coordinate front end (whose 1e-12 term has no exact fp64 twin, see tests/test_warp_exact_inputs.py): the suite's 1e-4.

Measured on the MI355X against fp64 (max-abs error / max-abs reference, maximum over all cases of a test):
  test_inverse_warp_exact          depth gradient 6.9e-06   pose gradient 4.4e-07
  test_inverse_warp_tolerance      depth gradient 1.4e-05   pose gradient 2.5e-06
  test_photo_loss_exact            depth gradient 5.2e-07   pose gradient 3.1e-07   loss 9.4e-08
  test_photo_loss_tolerance        depth gradient 1.2e-05   pose gradient 3.8e-07
Source-gradient elements whose terms cancel to an exact 0 in the oracle keep a residue of at most 3.8e-07 of the maximum."""
import functools

import pytest
import torch

import warp_exact as wx
from conftest import outliers, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the suite's bound (tests/test_gpu_losses.py)
EXACT = 1e-5        # depth / pose gradients of the exact family (the fp32 oracle's own distance from fp64: up to 3.5e-6)
DEV = "cuda"
_ids = lambda s: "%dx%d" % s if isinstance(s, tuple) and len(s) == 2 and isinstance(s[0], int) else None


@functools.lru_cache(maxsize=None)
def _case(h, w, family, c):
    return wx.make(h, w, family, c)


@functools.lru_cache(maxsize=None)
def _ref_warp(h, w, family, c, v, pad, align, rot, pix):
    return wx.oracle_warp(_case(h, w, family, c), v, pad, align, rot, torch.float64, pix)


def _flags(rot, pad, align, pix):
    from dvf import lib as L
    return (L.POSE_SE3 | L.PIXEL_COORDS) if pix else L.geom_flags(rot, pad, align)


def _leaf(x, grad=True, offset=False):
    """x on the GPU as a leaf; offset: a contiguous view one float into its storage (not 16-byte aligned)."""
    x = x.detach().float()
    g = torch.empty(x.numel() + 1, device=DEV)[1:].view(x.shape).copy_(x) if offset else x.clone().to(DEV)
    return g.requires_grad_(grad)


def _gpu_warp(case, v, pad, align, rot, pix=False, deterministic=False):
    from dvf import conv as C
    from dvf.ops import InverseWarpFn
    img, depth = _leaf(case.srcs[v]), _leaf(case.depth)
    pose = _leaf((case.pose_se3 if pix else case.pose)[v])
    C.set_deterministic(deterministic)
    try:
        out = InverseWarpFn.apply(img, depth, pose, case.K.to(DEV), case.Kinv.to(DEV), _flags(rot, pad, align, pix))
        out.backward(case.gouts[v].to(DEV))
        torch.cuda.synchronize()
    finally:
        C.set_deterministic(False)
    return out.detach().cpu(), img.grad.cpu(), depth.grad.cpu(), pose.grad.cpu()


def _report(test, **figures):
    print("measured %s: %s" % (test, "  ".join("%s %.1e" % kv for kv in figures.items())))


def _warp_runs(c):
    return [(v, rot) for v in range(4) for rot in (("euler", "quat") if c == 3 else ("euler",))]


@pytest.mark.parametrize("c", [1, 3, 32])
@pytest.mark.parametrize("pad,align", wx.MODES)
@pytest.mark.parametrize("size", wx.EXACT_SIZES, ids=_ids)
def test_inverse_warp_exact(size, pad, align, c):
    """dvf_inverse_warp_fwd / _bwd and _bwd_ordered on the exact family, every view, Euler and quaternion at C = 3."""
    case = _case(*size, "exact", c)
    worst_d = worst_p = 0.0
    for v, rot in _warp_runs(c):
        ref = _ref_warp(*size, "exact", c, v, pad, align, rot, False)
        got = _gpu_warp(case, v, pad, align, rot)
        assert torch.equal(got[0], ref[0].float()), (v, rot, "warped", int((got[0] != ref[0].float()).sum()))
        assert torch.equal(got[1], ref[1].float()), (v, rot, "image gradient", int((got[1] != ref[1].float()).sum()))
        for k, name in ((2, "depth"), (3, "pose")):
            assert rel_err(got[k], ref[k]) < EXACT and outliers(got[k], ref[k], EXACT) == 0, (v, rot, name, rel_err(got[k], ref[k]))
        worst_d, worst_p = max(worst_d, rel_err(got[2], ref[2])), max(worst_p, rel_err(got[3], ref[3]))
        if rot == "euler":
            det = _gpu_warp(case, v, pad, align, rot, deterministic=True)
            again = _gpu_warp(case, v, pad, align, rot, deterministic=True)
            assert torch.equal(det[3], again[3]), (v, "ordered pose gradient differs between two runs")
            assert rel_err(det[3], ref[3]) < EXACT and outliers(det[3], ref[3], EXACT) == 0, (v, "ordered pose")
            assert torch.equal(det[0], got[0]) and torch.equal(det[1], got[1]) and torch.equal(det[2], got[2]), (v, "ordered")
    _report("test_inverse_warp_exact", depth=worst_d, pose=worst_p)


_TOL_WARP = [(s, "mid", p, a, False) for s in wx.MID_SIZES for p, a in wx.MODES] + \
            [(s, "mid", "zeros", False, True) for s in wx.PIX_SIZES]


@pytest.mark.parametrize("c", [1, 3, 32])
@pytest.mark.parametrize("size,family,pad,align,pix", _TOL_WARP, ids=_ids)
def test_inverse_warp_tolerance(size, family, pad, align, pix, c):
    """Mid-cell family (x_n rounds) and the pixel-coordinate front end: 1e-4, unmasked, no outlier; identical zero pattern."""
    case = _case(*size, family, c)
    worst_d = worst_p = 0.0
    for v, rot in ([(v, "euler") for v in range(4)] if pix else _warp_runs(c)):
        ref = _ref_warp(*size, family, c, v, pad, align, rot, pix)
        got = _gpu_warp(case, v, pad, align, rot, pix)
        assert rel_err(got[0], ref[0]) < TOL and rel_err(got[1], ref[1]) < TOL, (v, rot)
        for k, name in ((2, "depth"), (3, "pose")):
            assert rel_err(got[k], ref[k]) < TOL and outliers(got[k], ref[k], TOL) == 0, (v, rot, name, rel_err(got[k], ref[k]))
        if pad == "zeros" and not align:
            assert torch.equal((got[0] == 0).all(1), (ref[0] == 0).all(1)), (v, rot, "zero pattern")
        worst_d, worst_p = max(worst_d, rel_err(got[2], ref[2])), max(worst_p, rel_err(got[3], ref[3]))
        if rot == "euler":
            det = _gpu_warp(case, v, pad, align, rot, pix, deterministic=True)
            again = _gpu_warp(case, v, pad, align, rot, pix, deterministic=True)
            assert torch.equal(det[3], again[3])
            assert rel_err(det[3], ref[3]) < TOL and outliers(det[3], ref[3], TOL) == 0
            assert torch.equal(det[0], got[0]) and torch.equal(det[2], got[2]) and rel_err(det[1], got[1]) < 1e-6
    _report("test_inverse_warp_tolerance", depth=worst_d, pose=worst_p)


# ------------------------------------------------------------------------------------------------- fused photometric loss
def _gpu_photo(case, nv, pad, align, tgt, mask, in_scale, pix=False, offset=False):
    from dvf.ops import PhotoLossFn
    lv = {"depth": _leaf(case.depth), "pose": _leaf((case.pose_se3 if pix else case.pose)[:nv]), "tgt": _leaf(tgt)}
    if mask is not None:
        lv["mask"] = _leaf(mask[:, :nv])
    for v in range(nv):
        lv[f"s{v}"] = _leaf(case.srcs[v], offset=offset)
    flags = (_flags("euler", pad, align, pix), in_scale)
    loss = PhotoLossFn.apply(lv["tgt"], lv["depth"], lv["pose"], case.K.to(DEV), case.Kinv.to(DEV), lv.get("mask"), flags,
                             *[lv[f"s{v}"] for v in range(nv)])
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), {k: x.grad.cpu() for k, x in lv.items()}


_PHOTO = [(s, nv, m, sc, c) for s in wx.EXACT_SIZES for nv in (1, 2, 4) for m in (False, True) for sc in (1.0, 0.25)
          for c in (3, 32)]
# NV = 3 has kernel instantiations of its own: one case per size, appended so that the indices (and modes) above do not move
_PHOTO += [(s, 3, True, 0.25, 3) for s in wx.EXACT_SIZES]


@pytest.mark.parametrize("n,size,nv,with_mask,in_scale,c", [(i,) + p for i, p in enumerate(_PHOTO)], ids=_ids)
def test_photo_loss_exact(n, size, nv, with_mask, in_scale, c):
    """PhotoLossFn on the exact family (padding / align_corners cycle over the cases).  Loss within 5e-7 (four fp32 ulps:
    one rounding in the reference's mean, up to two in partial * (1/N)); depth, pose, mask and target gradients within 1e-5;
    source gradients (22-bit fixed-point LDS accumulation) within 1e-4 and exactly 0 wherever the oracle's are.  On 5x257 the
    third batch element's first view spans more than 256 columns: the direct fallback, by the RS <= 256 rule."""
    pad, align = wx.MODES[(n + n // 4) % 4]
    case = _case(*size, "exact", c)
    if size == (5, 257):
        assert wx.max_span(case, 0, 2, pad, align)[0] > 256
    tgt, ties = wx.tie_target(case, nv, pad, align)
    assert ties > 0
    mask = case.mask if with_mask else None
    ref_loss, ref = wx.oracle_photo(case, nv, pad, align, tgt, mask, in_scale)
    loss, got = _gpu_photo(case, nv, pad, align, tgt, mask, in_scale)
    assert abs(float(loss) - float(ref_loss)) <= 5e-7 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    for k in ("depth", "pose", "tgt") + (("mask",) if with_mask else ()):
        assert rel_err(got[k], ref[k]) < EXACT and outliers(got[k], ref[k], EXACT) == 0, (k, rel_err(got[k], ref[k]))
    for v in range(nv):
        g, r = got[f"s{v}"], ref[f"s{v}"]
        assert rel_err(g, r) < TOL and outliers(g, r, TOL) == 0, (v, rel_err(g, r))
        # exactly 0 wherever no term reaches the element.  (Where terms reach it and cancel, the oracle's fp64 sum can be
        # exactly 0 while fp32 products of the same terms leave a residue: that is held to the 1e-4 above, not to 0.)
        assert int((g[ref[f"reach{v}"] == 0] != 0).sum()) == 0, (v, "gradient where no term reaches the element")
        cancel = (r == 0) & (ref[f"reach{v}"] != 0)
        if bool((g[cancel] != 0).any()):
            print("cancelling terms: view %d, %d elements, largest residue %.1e of the maximum" %
                  (v, int((g[cancel] != 0).sum()), float(g[cancel].abs().max()) / float(r.abs().max())))
    if pad == "zeros" and nv == 4:
        assert float(got["s2"][0].abs().max()) == 0.0              # view 2 of batch element 0 is wholly out of the image
    again_loss, again = _gpu_photo(case, nv, pad, align, tgt, mask, in_scale)
    assert torch.equal(loss, again_loss) and torch.equal(got["depth"], again["depth"]) and torch.equal(got["pose"], again["pose"])
    _report("test_photo_loss_exact", depth=rel_err(got["depth"], ref["depth"]), pose=rel_err(got["pose"], ref["pose"]),
            loss=abs(float(loss) - float(ref_loss)) / abs(float(ref_loss)))


_PHOTO_TOL = [(s, "mid", nv, m, c, False) for s in wx.MID_SIZES for nv, m, c in ((4, True, 3), (2, False, 32), (1, True, 32))] + \
             [(s, "mid", nv, m, 3, True) for s in wx.PIX_SIZES for nv, m in ((2, False), (4, True))]


@pytest.mark.parametrize("n,size,family,nv,with_mask,c,pix", [(i,) + p for i, p in enumerate(_PHOTO_TOL)], ids=_ids)
def test_photo_loss_tolerance(n, size, family, nv, with_mask, c, pix):
    """Mid-cell family (W % 4 == 0: 16-byte staging) and the pixel-coordinate front end, aligned and with the sources at a
    one-float storage offset (scalar staging): 1e-4 with no outlier; the two runs agree to 1e-6."""
    pad, align = ("zeros", False) if pix else wx.MODES[n % 4]
    in_scale = (1.0, 0.25)[n % 2]
    case = _case(*size, family, c)
    mask = case.mask if with_mask else None
    # off the values a bilinear blend of integers takes (weights are multiples of 1/16 times n/(n-1): 0.3 is one at H = 6):
    # no |tgt - warped| sits at its kink, where fp32 decides the sign
    tgt = case.tgt + 0.3183
    ref_loss, ref = wx.oracle_photo(case, nv, pad, align, tgt, mask, in_scale, pix=pix)
    runs = []
    for offset in (False, True):
        loss, got = _gpu_photo(case, nv, pad, align, tgt, mask, in_scale, pix, offset)
        assert abs(float(loss) - float(ref_loss)) <= TOL * abs(float(ref_loss)), (offset, float(loss), float(ref_loss))
        for k in got:
            assert rel_err(got[k], ref[k]) < TOL and outliers(got[k], ref[k], TOL) == 0, (offset, k, rel_err(got[k], ref[k]))
        runs.append((loss, got))
    assert abs(float(runs[0][0]) - float(runs[1][0])) <= 1e-6 * abs(float(ref_loss))
    for k in got:
        assert rel_err(runs[1][1][k], runs[0][1][k]) < 1e-6, k
    again_loss, again = _gpu_photo(case, nv, pad, align, tgt, mask, in_scale, pix)
    loss, got = runs[0]
    assert torch.equal(loss, again_loss) and torch.equal(got["depth"], again["depth"]) and torch.equal(got["pose"], again["pose"])
    _report("test_photo_loss_tolerance", depth=rel_err(got["depth"], ref["depth"]), pose=rel_err(got["pose"], ref["pose"]))
