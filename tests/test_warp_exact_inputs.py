"""CPU: the inputs of tests/warp_exact.py are what they claim to be, so that tests/test_gpu_warp_exact.py compares the HIP
sampler with something determinate.  Exact family: the fp32 and the fp64 oracle give the same bits; every decision of the
sampler occurs; the image gradient's scatter-add is exact in any order.  Mid-cell family and pixel-coordinate front end:
every source coordinate is at least 1e-3 px from a tap-set crossing and from |x_n| = 1."""
import pytest
import torch

import warp_exact as wx
from conftest import rel_err


@pytest.fixture(scope="module")
def exact_cases():
    return {s: wx.make(*s, "exact") for s in wx.EXACT_SIZES}


@pytest.mark.parametrize("size", wx.EXACT_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pad,align", wx.MODES)
def test_exact_family_fp32_equals_fp64(exact_cases, size, pad, align):
    """Warped image and image gradient: torch.equal.  Depth and pose gradients: the fp32 oracle's own distance from fp64
    is within the 1e-5 that the GPU test asks of the kernel (largest: 3.5e-6, depth gradient of 5x257 view 3, where terms of the
    size of the 256 px coordinate cancel down to shifts of a pixel or less; pose gradients stay below 1e-6)."""
    case = exact_cases[size]
    for v in range(4):
        for rot in ("euler", "quat"):
            o32 = wx.oracle_warp(case, v, pad, align, rot, torch.float32)
            o64 = wx.oracle_warp(case, v, pad, align, rot, torch.float64)
            assert torch.equal(o32[0], o64[0].float()), (v, rot, "warped")
            assert torch.equal(o32[1], o64[1].float()), (v, rot, "image gradient")
            assert rel_err(o32[2], o64[2]) < 1e-5, (v, rot, "depth gradient")
            assert rel_err(o32[3], o64[3]) < 1e-5, (v, rot, "pose gradient")
        assert wx.atomic_order_margin(case, v, pad, align) < 1.0, v


@pytest.mark.parametrize("size", wx.EXACT_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pad,align", wx.MODES)
def test_exact_family_census(exact_cases, size, pad, align):
    """Every decision the mode can take at this size occurs at least once, in x and again in y."""
    case = exact_cases[size]
    assert case.b == 3 and wx.behind_is_determinate(case)
    poses = case.pose.reshape(-1, 6)
    assert len({tuple(p.tolist()) for p in poses}) == poses.shape[0]          # a different pose per (view, batch element)
    n = wx.census(case, pad, align)
    for name, count in n.items():
        size_a = case.h if name.startswith("y:") else case.w
        if name in wx.COMMON:                   # (needs the decision in both axes: reachable only if it is in the smaller)
            size_a = min(case.h, case.w)
        if wx.reachable(name, size_a, pad, align):
            assert count > 0, (name, n)
        elif name.split(":")[-1] != "sentinel_hi":
            assert count == 0, (name, n)
    # decisions no mode of the grid path reaches are reached by the pixel-coordinate front end's inputs (below)
    assert any(wx.reachable("x:first_m1", case.w, p, a) for p, a in wx.MODES)


def test_exact_family_span_forces_the_direct_fallback(exact_cases):
    """5x257, batch element 2, view 0: a 64-pixel tile whose valid taps span more than 256 columns (RS <= 256 is the LDS
    tile's rule in footprint(), whatever tile size the host picks), with taps inside the image."""
    case = exact_cases[(5, 257)]
    for pad, align in wx.MODES:
        rs, spans = wx.max_span(case, 0, 2, pad, align)
        assert rs > 256, (pad, align, spans)
        r = wx.coords(case, 0, pad, align)
        inside = (r.x0[2] >= 0) & (r.x0[2] + 1 <= case.w - 1) & (r.y0[2] >= 0) & (r.y0[2] + 1 <= case.h - 1)
        assert int(inside[:4, :64].sum()) > 0
    # every other (view, batch element) of every exact size stays within the LDS tile's width
    for size, c in exact_cases.items():
        for v in range(4):
            for i in range(c.b):
                if (size, v, i) != ((5, 257), 0, 2):
                    assert wx.max_span(c, v, i)[0] <= 256, (size, v, i)


@pytest.mark.parametrize("size", wx.MID_SIZES, ids=lambda s: "%dx%d" % s)
def test_mid_cell_family_keeps_its_distance(size):
    case = wx.make(*size, "mid")
    assert size[1] % 4 == 0 and wx.behind_is_determinate(case)
    for pad, align in wx.MODES:
        assert wx.min_crossing_distance(case, pad, align) >= 1e-3, (pad, align)
        n = wx.census(case, pad, align)
        assert n["behind"] > 0 and (pad == "border" or n["view_out"] > 0)
        for v in range(4):
            o32 = wx.oracle_warp(case, v, pad, align, "euler", torch.float32)
            o64 = wx.oracle_warp(case, v, pad, align, "euler", torch.float64)
            for k, a, r in zip(("warped", "image", "depth", "pose"), o32, o64):
                assert rel_err(a, r) < 1e-4, (pad, align, v, k)
            if pad == "zeros":
                assert torch.equal((o32[0] == 0).all(1), (o64[0] == 0).all(1))


@pytest.mark.parametrize("size", wx.PIX_SIZES, ids=lambda s: "%dx%d" % s)
def test_pixel_coordinate_front_end_inputs(size):
    """The pixel-coordinate front end is in the tolerance group: the fp64 oracle's u = fx px / (pz + 1e-12) + cx is NOT the
    fp32 value where pz + 1e-12 rounds to pz -- at an integer coordinate the two take different tap sets, and a weight
    that is exactly 0 in fp32 is 1e-12 in fp64, which flips the exact-zero validity mask.  So it runs on the mid-cell
    shifts (no integer coordinate anywhere), where fp32 and fp64 agree to 1e-4 with the same zero pattern."""
    case = wx.make(*size, "mid")
    assert wx.min_crossing_distance(case, "zeros", False, pix=True) >= 1e-3
    n = wx.census(case, "zeros", False, pix=True)
    for name, count in n.items():
        if wx.reachable(name, 0, "zeros", False, pix=True) and name.split(":")[-1] not in ("int_inside", "corner_lo", "corner_hi"):
            assert count > 0, (name, n)
    for v in range(4):
        o32 = wx.oracle_warp(case, v, "zeros", False, dtype=torch.float32, pix=True)
        o64 = wx.oracle_warp(case, v, "zeros", False, dtype=torch.float64, pix=True)
        for k, a, r in zip(("warped", "image", "depth", "pose"), o32, o64):
            assert rel_err(a, r) < 1e-4, (v, k)
        assert torch.equal((o32[0] == 0).all(1), (o64[0] == 0).all(1))


def test_tie_targets_exist(exact_cases):
    for size, case in exact_cases.items():
        for pad, align in wx.MODES:
            assert wx.tie_target(case, 2, pad, align)[1] > 0, (size, pad, align)
