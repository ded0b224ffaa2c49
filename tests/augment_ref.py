"""Torch restatement of the on-device training augmentation (test infrastructure; imports nothing from the product).

The reference's ``custom_transforms.py`` (RandomHorizontalFlip :46-61, RandomScaleCrop :64-84) cannot be imported any more
(``scipy.misc.imresize`` is gone), so this file IS the definition the HIP kernels (csrc/augment.hip) are tested against and
parity is unpinned: plain tensor code, fp64 or fp32, CPU.

One record of 12 numbers per sample applies to ALL frames of the sample (target, temporal references, stereo view):

  0      flip          0 or 1
  1, 2   sw, sh        size of the zoomed image before the crop, integers, W <= sw <= int(zoom_max W), same for sh
  3, 4   ox, oy        crop offset, integers, 0 <= ox <= sw - W, 0 <= oy <= sh - H
  5      colour_on     0 or 1
  6      gamma         U[0.8, 1.2]
  7      brightness    U[0.5, 2.0]
  8..10  gain r, g, b  U[0.8, 1.2] each
  11     reserved      0

Resample (zoom-crop first, flip last, half-pixel centres, edge clamp), for output pixel (y, x):
  xc = flip ? W-1-x : x;  u = (xc + ox + 0.5) (W / sw) - 0.5;  v = (y + oy + 0.5) (H / sh) - 0.5,  clamped to the image;
  x0 = floor(u), x1 = min(x0 + 1, W-1), fx = u - x0 (likewise y);  value = (1-fy)((1-fx) a + fx b) + fy((1-fx) c + fx d).
With sw = W, ox = 0 the fractions are exactly 0: a bit-exact copy (or mirror).

Colour, only where colour_on (else the value passes through bit for bit):
  n = value / value_max;  n = n^gamma (0 stays 0);  n = n brightness gain_c;  value = value_max clamp(n, 0, 1).

Intrinsics, with sx = sw/W, sy = sh/H, cxo = 0.5 (sx-1) - ox, cyo = 0.5 (sy-1) - oy:
  no flip  A = [[sx,0,cxo],[0,sy,cyo],[0,0,1]],       M = I
  flip     A = [[-sx,0,W-1-cxo],[0,sy,cyo],[0,0,1]],  M = diag(-1,1,1)
  K' = A K M,  Kinv' = M Kinv A^-1 (A^-1 in closed form).
A is the exact map from old to new pixel indices in the warp's own convention (an integer index is the pixel centre,
inverse_warp.py set_id_grid).  TWO DEPARTURES FROM THE REFERENCE: it scales K by the untruncated random factor and ignores the
half-pixel term (custom_transforms.py:73-74, 81-82), and it mirrors the principal point as w - cx (:55), one pixel off in this
convention.

Stereo pose, under flip only (conjugation by M, exact for Rx Ry Rz, for the exponential map and for the quaternion form):
  T_R2L     (t, r)  *= (-1, 1, 1, 1, -1, -1)
  T_R2L_se3 (w, u)  *= (1, -1, -1, -1, 1, 1)
Zoom-crop leaves poses alone.
"""
import torch

IDENTITY = (0.0, None, None, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0)      # sw, sh = W, H
TR_FLIP = (-1.0, 1.0, 1.0, 1.0, -1.0, -1.0)
SE3_FLIP = (1.0, -1.0, -1.0, -1.0, 1.0, 1.0)


def identity_record(H, W):
    r = list(IDENTITY)
    r[1], r[2] = float(W), float(H)
    return r


def resample_coords(params, H, W, dtype):
    """Clamped source coordinates (u [B,W], v [B,H]) and the masks of the output columns / rows whose taps were not clamped."""
    p = params.to(dtype)
    flip, sw, sh, ox, oy = (p[:, i:i + 1] for i in range(5))
    x = torch.arange(W, dtype=dtype)[None]
    y = torch.arange(H, dtype=dtype)[None]
    xc = torch.where(flip > 0.5, W - 1 - x, x)
    u = (xc + ox + 0.5) * (W / sw) - 0.5
    v = (y + oy + 0.5) * (H / sh) - 0.5
    free_x = (u >= 0) & (u <= W - 1)
    free_y = (v >= 0) & (v <= H - 1)
    return u.clamp(0, W - 1), v.clamp(0, H - 1), free_x, free_y


def resample(frame, params):
    B, C, H, W = frame.shape
    u, v, _, _ = resample_coords(params, H, W, frame.dtype)
    x0f, y0f = torch.floor(u), torch.floor(v)
    fx, fy = (u - x0f)[:, None, None, :], (v - y0f)[:, None, :, None]
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)

    def rows(yi):
        return torch.gather(frame, 2, yi[:, None, :, None].expand(B, C, H, W))

    def cols(t, xi):
        return torch.gather(t, 3, xi[:, None, None, :].expand(B, C, H, W))

    top, bot = rows(y0), rows(y1)
    a, b, c, d = cols(top, x0), cols(top, x1), cols(bot, x0), cols(bot, x1)
    return (1 - fy) * ((1 - fx) * a + fx * b) + fy * ((1 - fx) * c + fx * d)


def colour(frame, params, value_max=255.0):
    p = params.to(frame.dtype)
    on = (p[:, 5] > 0.5).view(-1, 1, 1, 1)
    gamma, bright = p[:, 6].view(-1, 1, 1, 1), p[:, 7].view(-1, 1, 1, 1)
    gain = p[:, 8:11].view(-1, 3, 1, 1)
    n = frame / value_max
    n = torch.where(n == 0, torch.zeros_like(n), n ** gamma)
    n = n * bright * gain
    return torch.where(on, value_max * n.clamp(0, 1), frame)


def pixel_map(params, H, W, dtype):
    """A [B,3,3] (old pixel index -> new pixel index) and its closed-form inverse."""
    p = params.to(dtype)
    flip, sw, sh, ox, oy = (p[:, i] for i in range(5))
    sx, sy = sw / W, sh / H
    cxo, cyo = 0.5 * (sx - 1) - ox, 0.5 * (sy - 1) - oy
    f = flip > 0.5
    a = torch.where(f, -sx, sx)
    c = torch.where(f, W - 1 - cxo, cxo)
    o, i = torch.zeros_like(a), torch.ones_like(a)
    A = torch.stack([a, o, c, o, sy, cyo, o, o, i], dim=1).view(-1, 3, 3)
    Ainv = torch.stack([1 / a, o, -c / a, o, 1 / sy, -cyo / sy, o, o, i], dim=1).view(-1, 3, 3)
    return A, Ainv


def apply_ref(frames, K, Kinv, T_tr, T_se3, params, value_max=255.0):
    """frames: list of [B,3,H,W]; K, Kinv [B,3,3]; T_tr, T_se3 [B,6]; params [B,12] ->
    (frames', K', Kinv', T_tr', T_se3') in the dtype of the inputs."""
    B, _, H, W = frames[0].shape
    dtype = K.dtype
    out = [colour(resample(f, params), params, value_max) for f in frames]
    A, Ainv = pixel_map(params, H, W, dtype)
    f = (params[:, 0] > 0.5)
    m = torch.where(f, -torch.ones(B, dtype=dtype), torch.ones(B, dtype=dtype))
    M = torch.diag_embed(torch.stack([m, torch.ones_like(m), torch.ones_like(m)], dim=1))
    K2 = A @ K @ M
    Kinv2 = M @ Kinv @ Ainv
    one = torch.ones(6, dtype=dtype)
    s_tr = torch.where(f[:, None], torch.tensor(TR_FLIP, dtype=dtype)[None], one[None])
    s_se3 = torch.where(f[:, None], torch.tensor(SE3_FLIP, dtype=dtype)[None], one[None])
    return out, K2, Kinv2, T_tr * s_tr, T_se3 * s_se3
