"""Exactly representable warps for the bilinear sampler (tests/test_warp_exact_inputs.py, tests/test_gpu_warp_exact.py).

Rotation is zero (R = I exactly, Euler or quaternion), K = [[f,0,cx],[0,f,cy],[0,0,1]] with f = 4 and an integer, non-zero
principal point, Kinv is written by hand, depths are powers of two and translations multiples of 1/16.  With t_z = 0 the
source coordinate of target pixel u is x_q = u + S_x / d with S_x = f t_x a multiple of 1/4: a multiple of 1/16 for
d in {1/2, 1, 2, 4}.  "Shifts" below are (S_x, S_y, t_z): pixels at depth 1, and metres.

Exact family: H-1 and W-1 are powers of two, so x_n = 2 x_q / (W-1) - 1 and both un-normalisations are exact in fp32, the
bilinear weights carry at most 20 fractional bits, images and upstream gradients are small integers: every coordinate,
weight, product and sum is exact, fp32 and fp64 give the same bits, and no pixel is ambiguous.  The depth map and the
shifts are placed so that every decision of the sampler occurs (census()).

Mid-cell family: widths are multiples of 4 (16-byte staging in photo_loss.hip), W-1 is no power of two and x_n rounds; depths
are 1/2 and 1 and all shifts are ODD multiples of 1/4, chosen per size so that no x_q is an integer and every source
coordinate stays away from a tap-set crossing and from |x_n| = 1 (_clear_shift(), min_crossing_distance()).  The same shifts serve the pixel-coordinate front end.

Not placed on purpose: a pixel at p_z == 1e-3 exactly.  The fp64 oracle's constant 1e-3 differs from the kernel's 1e-3f, so
that tie has no fp64 truth.  Behind-camera pixels here have p_z <= 0, and their p_x, p_y are 0 or at least 1/4 in
magnitude, which the clamp Z = 1e-3 sends 250 px or more away: out of the image on the same side in fp32 and fp64."""
import types

import torch

from oracle import geometry as og

F = 4.0
DEPTHS = (0.5, 1.0, 2.0, 4.0)
MID_DEPTHS = (0.5, 1.0)                          # (depths 2 and 4 put x_q on odd eighths / sixteenths: see _clear_shift)
EXACT_SIZES = ((5, 9), (17, 65), (9, 129), (5, 257))
MID_SIZES = ((6, 8), (8, 64), (12, 132))
PIX_SIZES = ((8, 64), (5, 65))
MODES = (("zeros", False), ("zeros", True), ("border", False), ("border", True))
TX, TY = 64, 4                                  # the warp kernels' block tile (csrc/warp_common.h)
# 5x257, batch element 2: depths 1/2 and 128 alternate along x and view 0 shifts by 96 px at depth 1.  Pixel u = 0 (depth
# 128) samples column 0.75 and pixel u = 63 (depth 1/2) column 255: the first 64-pixel tile's valid taps span all 257
# columns.  (With depths 1/2 and 8 no translation does that: both shifts have the sign of S_x and their ratio is 16, so a
# tile that reaches column 255 starts at column 6 or later, a span of at most 251.)
SPAN_DEPTHS = (128.0, 0.5)
SPAN_SHIFT = 96.0


def intrinsics(b, h, w):
    cx, cy = (w - 1) // 2 + 1.0, max((h - 1) // 2 - 1.0, 1.0)
    K = torch.tensor([[F, 0, cx], [0, F, cy], [0, 0, 1.0]])
    Kinv = torch.tensor([[1 / F, 0, -cx / F], [0, 1 / F, -cy / F], [0, 0, 1.0]])        # by hand, not torch.inverse
    return K.expand(b, 3, 3).contiguous(), Kinv.expand(b, 3, 3).contiguous()


def shifts(h, w, family):
    """[V=4][B] -> (S_x, S_y, t_z); every (view, batch element) differs."""
    out = 4.0 * (w + 4)                                     # even at depth 4 the whole image lands right of column W+3
    if family == "exact":
        tab = [[(0.25, 0.25, 0), (-0.25, -0.25, 0)],        # +-1/16 .. +-1/2 px: x0 = -1 / W-1, one step beyond |x_n| = 1
               [(0, 0, 0), (-2, 1, 0)],                     # identity: integer coordinates, x_n = +-1 exactly, the far corner
               [(out, -0.5, 0), (1, -1, -2)],               # wholly out of the image | behind the camera where depth <= 2
               [(0.75, -0.5, 0), (-1.25, 0.75, 0)]]
        # third batch element: shifts of several pixels.  Its depth gradients (|S| / d^2) are the largest of each view: the
        # sub-pixel shifts above compute theirs as the difference of terms the size of the coordinate (u / d), and that
        # cancellation noise is then small against the tensor's maximum, which every bound here is relative to
        for v, s in enumerate([(8.5, -0.25, 0), (-6.25, 0.5, 0), (9, 2, 0), (-11, -0.5, 0)]):
            tab[v].append(s)
        if (h, w) == (5, 257):
            for row in tab:
                row.pop()
            for v, s in enumerate([(SPAN_SHIFT, 0, 0), (-32, 0, 0), (64, 0, 0), (32, -32, 0)]):
                tab[v].append(s)
        return tab
    tab = [[(0.25, 0.25, 0), (-0.25, -0.25, 0)],            # odd quarters only: no integer x_q at either depth
           [(0.75, -1.25, 0), (-2.25, 0.75, 0)],
           [(out + 0.25, -0.25, 0), (1.25, -0.75, -2)],
           [(1.75, 3.25, 0), (-12.25, -8.25, 0)]]           # +6.5 / -24.5 px at depth 1/2: floor(ix) > n+1 / < -2 in pixel-coordinate mode
    return [[(_clear_shift(w, sx), _clear_shift(h, sy), tz) for sx, sy, tz in row] for row in tab]


def _clear_shift(n, want):
    """The odd multiple of 1/4 nearest to `want` (ties: the larger magnitude) for which every u + S / d, u in [0, n),
    d in MID_DEPTHS, un-normalises at least 1/512 px from an integer with align_corners off and on.  A multiple of 1/16
    alone does not give that: ix = x_q n / (n - 1) - 1/2 is an integer at x_q = 1.25 for n = 6 or 3.0625 for n = 8."""
    def clear(s):
        for d in MID_DEPTHS:
            for u in range(n):
                q = u + s / d
                for raw in (q, q * n / (n - 1) - 0.5):
                    if -2 < raw < n + 1 and abs(raw - round(raw)) < 1 / 512:
                        return False
        return True
    cands = sorted((k / 4 for k in range(-63, 64, 2)), key=lambda c: (abs(c - want), -abs(c)))
    return next(c for c in cands if abs(c - want) < 4 and clear(c)) if abs(want) < 16 else want


def _blocky(gen, b, h, w, lo, hi):
    """Integers constant over 2x4 cells: many 2x2 neighbourhoods are constant, so the warped value is an integer there."""
    cells = torch.randint(lo, hi, (b, (h + 1) // 2, (w + 3) // 4), generator=gen)
    return cells.repeat_interleave(2, 1).repeat_interleave(4, 2)[:, :h, :w].float()


def make(h, w, family="exact", c=3, seed=0):
    """Inputs of one case (fp32, CPU).  pose is [V=4,B,6] = (tx,ty,tz,0,0,0); pose_se3 the same translations as (0,0,0,u).
    srcs / gouts: one [B,C,H,W] integer tensor per view; tgt integer; mask [B,4,H,W] multiples of 1/16 (zeros included)."""
    tab = shifts(h, w, family)
    b = len(tab[0])
    gen = torch.Generator().manual_seed(1000 * h + w + 7 * c + seed)
    K, Kinv = intrinsics(b, h, w)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    depth = torch.tensor(DEPTHS)[(xx + yy + 3) % 4].expand(b, h, w).contiguous()       # depth 4 at both far corners
    if family == "exact" and (h, w) == (5, 257):
        depth[2] = torch.tensor(SPAN_DEPTHS)[xx % 2]
    if family != "exact":
        depth = torch.tensor(MID_DEPTHS)[(xx + yy) % 2].expand(b, h, w).contiguous()
    pose = torch.zeros(4, b, 6)
    for v in range(4):
        for i in range(b):
            sx, sy, tz = tab[v][i]
            pose[v, i, :3] = torch.tensor([sx / F, sy / F, float(tz)])
    case = types.SimpleNamespace(h=h, w=w, b=b, c=c, family=family, K=K, Kinv=Kinv, depth=depth, pose=pose)
    case.pose_se3 = torch.cat((pose[..., 3:], pose[..., :3]), dim=-1).contiguous()
    case.srcs, case.gouts = [], []
    for v in range(4):
        s = torch.randint(-2, 4, (b, c, h, w), generator=gen).float()
        s[:, 0] = _blocky(gen, b, h, w, 1, 4)
        case.srcs.append(s)
        case.gouts.append(torch.randint(-2, 3, (b, c, h, w), generator=gen).float())
    case.tgt = torch.randint(-2, 4, (b, c, h, w), generator=gen).float()
    case.mask = torch.randint(0, 17, (b, 4, h, w), generator=gen).float() / 16
    return case


def coords(case, v, pad="zeros", align=False, pix=False):
    """fp64 source coordinates of view v as the sampler decides them: raw x_q, x_n, un-normalised ix after the zeros
    overwrite / border clip, x0 = floor(ix), `cut` (gradient cut), p_z.  Tensors are [B,H,W]."""
    b, h, w = case.depth.shape
    cam = og.pixel2cam(case.depth.double(), case.Kinv.double())
    proj = case.K.double() @ og.pose_vec2mat(case.pose[v].double(), "euler")
    p = (proj[:, :, :3] @ cam.reshape(b, 3, -1) + proj[:, :, 3:]).reshape(b, 3, h, w)
    r = types.SimpleNamespace(pz=p[:, 2])
    Z = p[:, 2] + 1e-12 if pix else p[:, 2].clamp(min=1e-3)
    for a, n, q in (("x", w, p[:, 0] / Z), ("y", h, p[:, 1] / Z)):
        xn = 2 * q / (n - 1) - 1
        cut = torch.zeros_like(q, dtype=torch.bool)
        if pix:
            ix = q
        else:
            xs = xn
            if pad == "zeros":
                cut = (xn > 1) | (xn < -1)
                xs = torch.where(cut, torch.full_like(xn, 2.0), xn)
            ix = (xs + 1) / 2 * (n - 1) if align else ((xs + 1) * n - 1) / 2
            if pad == "border":
                cut = (ix < 0) | (ix > n - 1)
                ix = ix.clamp(0, n - 1)
        setattr(r, a + "q", q)
        setattr(r, a + "n", xn)
        setattr(r, "i" + a, ix)
        setattr(r, a + "0", torch.floor(ix))
        setattr(r, "cut_" + a, cut)
    r.any_tap = ((r.x0 >= -1) & (r.x0 <= w - 1)) & ((r.y0 >= -1) & (r.y0 <= h - 1))
    return r


def foot_spans(x0, y0, h, w, vec):
    """Per 64x4 block of one image: (RS, rows) of the valid taps' bounding box as footprint() in csrc/photo_loss.hip
    computes them, or None for a block without a valid tap.  x0, y0: [H,W] floor coordinates."""
    x0, y0 = x0.long().clamp(-4, w + 4), y0.long().clamp(-4, h + 4)
    anyv = ((x0 >= -1) & (x0 <= w - 1)) & ((y0 >= -1) & (y0 <= h - 1))
    xb, ya, yb = x0.clamp(0, w - 2), y0.clamp(0, h - 1), (y0 + 1).clamp(0, h - 1)
    out = []
    for by in range(0, h, TY):
        for bx in range(0, w, TX):
            sl = (slice(by, by + TY), slice(bx, bx + TX))
            m = anyv[sl]
            if not bool(m.any()):
                out.append(None)
                continue
            lo, hi = int(xb[sl][m].min()), int(xb[sl][m].max()) + 1
            if vec:
                lo &= ~3
            rs = ((hi - lo + 1 + 3) & ~3) if vec else hi - lo + 1
            out.append((rs, int(yb[sl][m].max()) - int(ya[sl][m].min()) + 1))
    return out


def max_span(case, v, i, pad="zeros", align=False, pix=False):
    r = coords(case, v, pad, align, pix)
    spans = foot_spans(r.x0[i], r.y0[i], case.h, case.w, case.w % 4 == 0)
    return max((s[0] for s in spans if s is not None), default=0), spans


CASES = ("int_inside", "first_m1", "first_last", "xn_p1", "xn_m1", "beyond_p1", "beyond_m1", "sentinel_hi", "sentinel_lo")
COMMON = ("corner_lo", "corner_hi", "behind", "view_out")


def census(case, pad, align, pix=False):
    """{name: count}: per axis ("x:" / "y:") the decisions of CASES, and those of COMMON, over all views."""
    n = {a + ":" + k: 0 for a in "xy" for k in CASES}
    n.update({k: 0 for k in COMMON})
    for v in range(4):
        r = coords(case, v, pad, align, pix)
        for a, size in (("x", case.w), ("y", case.h)):
            q, xn, ix = getattr(r, a + "q"), getattr(r, a + "n"), getattr(r, "i" + a)
            f0, cut = getattr(r, a + "0"), getattr(r, "cut_" + a)
            cnt = lambda m: int(m.sum())
            n[a + ":int_inside"] += cnt(~cut & (ix == f0) & (ix > 0) & (ix < size - 1))
            n[a + ":first_m1"] += cnt(f0 == -1)
            n[a + ":first_last"] += cnt(f0 == size - 1)
            n[a + ":xn_p1"] += cnt(xn == 1)
            n[a + ":xn_m1"] += cnt(xn == -1)
            n[a + ":beyond_p1"] += cnt(q == size - 1 + 1 / 16)
            n[a + ":beyond_m1"] += cnt(q == -1 / 16)
            n[a + ":sentinel_hi"] += cnt(f0 > size + 1)
            n[a + ":sentinel_lo"] += cnt(f0 < -2)
        n["corner_lo"] += int(((r.x0 == -1) & (r.y0 == -1)).sum())
        n["corner_hi"] += int(((r.x0 == case.w - 1) & (r.y0 == case.h - 1)).sum())
        n["behind"] += int((r.pz < 1e-3).sum())
        n["view_out"] += sum(1 for i in range(case.b) if not bool(r.any_tap[i].any()))
    return n


def reachable(name, size, pad, align, pix=False):
    """Whether the sampler can take decision `name` along an axis of `size` samples in this mode at all."""
    key = name.split(":")[-1]
    if pix:                                     # coordinates are used as they come: every decision but the x_n ones matters
        return key not in ("xn_p1", "xn_m1", "beyond_p1", "beyond_m1")
    if pad == "border":                         # clipped to [0, size-1]: floor(ix) never leaves the image
        return key not in ("first_m1", "corner_lo", "sentinel_hi", "sentinel_lo", "view_out")
    if key in ("first_m1", "corner_lo"):        # zeros: x_n >= -1 gives ix >= -1/2 (align_corners off) or >= 0 (on)
        return not align
    if key == "sentinel_lo":                    # zeros: x_n < -1 is overwritten with +2
        return False
    if key == "sentinel_hi":                    # the overwritten coordinate x_n = 2 itself: floor(ix) > size + 1 ?
        ix2 = 1.5 * (size - 1) if align else (3 * size - 1) / 2
        return int(ix2) > size + 1
    return True


def min_crossing_distance(case, pad, align, pix=False):
    """Smallest distance in pixels, over all views and both axes, of a source coordinate that can reach a tap to an integer
    (tap-set crossing, border clip) and of a raw coordinate to the |x_n| = 1 overwrite boundary (x_q = 0, size-1)."""
    best = float("inf")
    for v in range(4):
        r = coords(case, v, "border" if pix else pad, align, pix)   # (unclipped distance: computed from x_n below)
        for a, size in (("x", case.w), ("y", case.h)):
            q, xn = getattr(r, a + "q"), getattr(r, a + "n")
            raw = q if pix else ((xn + 1) / 2 * (size - 1) if align else ((xn + 1) * size - 1) / 2)
            near = (raw > -2) & (raw < size + 1)
            if bool(near.any()):
                best = min(best, float((raw[near] - raw[near].round()).abs().min()))
            if not pix:
                best = min(best, float(torch.minimum(q.abs(), (q - (size - 1)).abs()).min()))
    return best


def behind_is_determinate(case):
    """Behind-camera pixels (p_z < 1e-3): p_x, p_y are 0 or at least 1/4 in magnitude (see the module docstring)."""
    b, h, w = case.depth.shape
    for v in range(4):
        cam = og.pixel2cam(case.depth.double(), case.Kinv.double())
        proj = case.K.double() @ og.pose_vec2mat(case.pose[v].double(), "euler")
        p = (proj[:, :, :3] @ cam.reshape(b, 3, -1) + proj[:, :, 3:]).reshape(b, 3, h, w)
        m = p[:, 2] < 1e-3
        for k in (0, 1):
            vals = p[:, k][m].abs()
            if bool(((vals != 0) & (vals < 0.25)).any()):
                return False
        if bool(((p[:, 2] > 0) & (p[:, 2] < 0.25)).any()):       # nothing near the 1e-3 clamp
            return False
    return True


# ---------------------------------------------------------------------------------------------------------- oracle runs
def _leaf(x, dtype, grad=True):
    return x.detach().clone().to(dtype).contiguous().requires_grad_(grad)


def oracle_warp(case, v, pad, align, rot="euler", dtype=torch.float64, pix=False):
    """Oracle inverse warp of view v and its backward with the case's upstream gradient: (out, g_img, g_depth, g_pose)."""
    img, depth = _leaf(case.srcs[v], dtype), _leaf(case.depth, dtype)
    pose = _leaf((case.pose_se3 if pix else case.pose)[v], dtype)
    if pix:
        out = og.inverse_warp_pixel(img, depth, og.se3_exp(pose), case.K.to(dtype))
    else:
        out = og.inverse_warp(img, depth, pose, case.K.to(dtype), case.Kinv.to(dtype), rot, pad, align)
    (out * case.gouts[v].to(dtype)).sum().backward()
    return out.detach(), img.grad, depth.grad, pose.grad


def tie_target(case, nv, pad, align, pix=False):
    """The case's integer target with, wherever the fp64 warp of one of the first nv views is an integer, that integer:
    |tgt - warped| is exactly zero there (sgn(0) = 0 is part of the contract).  Returns (tgt, number of such elements)."""
    tgt, ties = case.tgt.clone(), 0
    for v in reversed(range(nv)):
        w = oracle_warp(case, v, pad, align, pix=pix)[0]
        hit = (w == w.round()) & (w != 0)
        tgt = torch.where(hit, w.float(), tgt)
    for v in range(nv):
        w = oracle_warp(case, v, pad, align, pix=pix)[0]
        ties += int((tgt.double() == w).sum())
    return tgt, ties


def oracle_photo(case, nv, pad, align, tgt, mask=None, in_scale=1.0, rot="euler", dtype=torch.float64, pix=False,
                 src_grads=True):
    """Oracle photometric loss over the first nv views (explainability-mask form; in_scale multiplies every image value)
    and its backward.  Returns (loss, {name: gradient}) with names depth, pose [V,B,6], mask, tgt, s0 .. s{nv-1}."""
    lv = {"depth": _leaf(case.depth, dtype), "pose": _leaf((case.pose_se3 if pix else case.pose)[:nv], dtype),
          "tgt": _leaf(tgt, dtype)}
    if mask is not None:
        lv["mask"] = _leaf(mask[:, :nv], dtype)
    for v in range(nv):
        lv[f"s{v}"] = _leaf(case.srcs[v], dtype, src_grads)
    K, Kinv = case.K.to(dtype), case.Kinv.to(dtype)
    total = 0
    for v in range(nv):
        src = in_scale * lv[f"s{v}"]
        if pix:
            warped = og.inverse_warp_pixel(src, lv["depth"], og.se3_exp(lv["pose"][v]), K)
        else:
            warped = og.inverse_warp(src, lv["depth"], lv["pose"][v], K, Kinv, rot, pad, align)
        valid = 1 - (warped == 0).prod(1, keepdim=True).type_as(warped)
        diff = (in_scale * lv["tgt"] - warped) * valid
        if mask is not None:
            diff = diff * lv["mask"][:, v:v + 1]
        total = total + diff.abs().mean()
    total.backward()
    grads = {k: x.grad for k, x in lv.items() if x.grad is not None}
    # reach{v}: per source element the sum of the bilinear weights of the pixels whose term is not zero (sign, validity and
    # mask all non-zero).  Exactly 0 = no term reaches the element; an element whose terms merely cancel is > 0.
    for v in range(nv):
        src = _leaf(case.srcs[v], dtype)
        if pix:
            warped = og.inverse_warp_pixel(in_scale * src, lv["depth"].detach(), og.se3_exp(lv["pose"][v].detach()), K)
        else:
            warped = og.inverse_warp(in_scale * src, lv["depth"].detach(), lv["pose"][v].detach(), K, Kinv, rot, pad, align)
        valid = 1 - (warped == 0).prod(1, keepdim=True).type_as(warped)
        diff = (in_scale * lv["tgt"].detach() - warped.detach()) * valid
        if mask is not None:
            diff = diff * lv["mask"][:, v:v + 1].detach()
        (warped * (diff != 0).to(dtype)).sum().backward()
        grads[f"reach{v}"] = src.grad
    return total.detach(), grads


def atomic_order_margin(case, v, pad, align):
    """Certificate that the image gradient's scatter-add is exact in ANY order: per source element, every term
    g * weight is a multiple of 2^-q (q = the largest number of fractional bits among that element's terms) and the sum of
    the terms' magnitudes stays below 2^(24-q), so every partial sum is an fp32 number.  Returns the largest
    sum|terms| * 2^q / 2^24 over the elements (< 1 means certified)."""
    r = coords(case, v, pad, align)
    b, c, h, w = case.srcs[v].shape
    g = case.gouts[v].double()
    ex, ey = r.x0 + 1 - r.ix, r.y0 + 1 - r.iy
    dx, dy = r.ix - r.x0, r.iy - r.y0
    mag = torch.zeros(b, c, h * w, dtype=torch.float64)
    bits = torch.zeros(b, c, h * w, dtype=torch.float64)
    for xi, yi, wt in ((r.x0, r.y0, ex * ey), (r.x0 + 1, r.y0, dx * ey), (r.x0, r.y0 + 1, ex * dy), (r.x0 + 1, r.y0 + 1, dx * dy)):
        ok = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
        term = (g * (wt * ok).unsqueeze(1)).reshape(b, c, -1)
        q = torch.zeros_like(term)
        for k in range(1, 41):
            q = torch.where((term * 2.0 ** (k - 1)) != torch.floor(term * 2.0 ** (k - 1)), torch.full_like(q, float(k)), q)
        idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long().reshape(b, 1, -1).expand(b, c, -1)
        mag.scatter_add_(2, idx, term.abs())
        bits = bits.scatter_reduce(2, idx, q, reduce="amax")
    return float((mag * 2.0 ** bits).max()) / 2.0 ** 24
