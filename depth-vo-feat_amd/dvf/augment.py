"""On-device training augmentation (build-side extension, opt-in through ``--augment``): random horizontal flip, random
zoom-and-crop and a colour perturbation of every frame of a sample, with the matching intrinsics and stereo pose, in one
streaming pass from the loader's batch into the step's static input tensors (csrc/augment.hip).

It stands where the reference applies ``custom_transforms.RandomHorizontalFlip`` / ``RandomScaleCrop`` on the host
(custom_transforms.py:46-84, train.py:89-101).  Those no longer import (``scipy.misc.imresize``), so parity is unpinned and
``tests/augment_ref.py`` is the definition.  TWO DELIBERATE DEPARTURES FROM THE REFERENCE, both because the intrinsics must be
the exact map of pixel indices in the warp's own convention (an integer index is the pixel centre, inverse_warp.py:8-15):

  * the reference scales fx, cx by the untruncated random factor and ignores the half-pixel term
    (custom_transforms.py:73-74, 81-82); here sx = sw / W with the integer zoomed size, cx' = sx cx + (sx - 1) / 2 - ox;
  * the reference mirrors the principal point as w - cx (custom_transforms.py:55); here cx' = W - 1 - cx, and the stereo
    baseline changes sign with the flip.  With w - cx the photometric loss of a mirrored batch differs from the original's
    by about 1 %; with W - 1 - cx it is equal to the last digit (tests/test_augment.py).

One record of 12 floats per sample, applied to all frames of the sample (the loss is taken on the augmented frames):
``(flip, sw, sh, ox, oy, colour_on, gamma, brightness, gain_r, gain_g, gain_b, 0)``."""
import ctypes

import torch

from . import lib as L

OPS = ("flip", "zoom", "colour")
REC = 12
FRAME_KEYS = ("img_R2", "img_R1", "img_L2")
MAX_FRAMES = 8          # frames per launch of dvf_augment_frames
GAMMA, BRIGHTNESS, GAIN = (0.8, 1.2), (0.5, 2.0), (0.8, 1.2)


def parse_ops(text):
    """``"flip,colour"`` -> ("flip", "colour") in canonical order; ValueError for an unknown or empty name."""
    names = [n.strip() for n in text.split(",")]
    bad = [n for n in names if n not in OPS]
    if bad or not names:
        raise ValueError(f"unknown augmentation op {bad[0]!r}: choose from {', '.join(OPS)}")
    return tuple(o for o in OPS if o in names)


def identity_params(B, H, W):
    rec = torch.tensor([0, W, H, 0, 0, 0, 1, 1, 1, 1, 1, 0], dtype=torch.float32)
    return rec.repeat(B, 1)


def sample_params(generator, B, H, W, ops=OPS, flip_prob=0.5, zoom_max=1.15, colour_prob=0.5):
    """float32 CPU tensor [B,12], deterministic in ``generator``.  Zoom: x_scaling, y_scaling ~ U[1, zoom_max] independently,
    sw = int(W x_scaling), sh = int(H y_scaling), offsets uniform integers in [0, sw - W] and [0, sh - H], as
    custom_transforms.py:70-78 draws them.  An op left out of ``ops`` keeps its identity fields (the same number of random
    draws is consumed whatever the ops, so switching one off does not change the others' stream)."""
    for o in ops:
        if o not in OPS:
            raise ValueError(f"unknown augmentation op {o!r}: choose from {', '.join(OPS)}")
    r = torch.rand(B, 11, generator=generator, dtype=torch.float64)
    p = identity_params(B, H, W).double()
    if "flip" in ops:
        p[:, 0] = (r[:, 0] < flip_prob).double()
    if "zoom" in ops:
        sw = torch.floor(W * (1 + r[:, 1] * (zoom_max - 1)))
        sh = torch.floor(H * (1 + r[:, 2] * (zoom_max - 1)))
        p[:, 1], p[:, 2] = sw, sh
        p[:, 3] = torch.minimum(torch.floor(r[:, 3] * (sw - W + 1)), sw - W)
        p[:, 4] = torch.minimum(torch.floor(r[:, 4] * (sh - H + 1)), sh - H)
    if "colour" in ops:
        on = r[:, 5] < colour_prob
        p[:, 5] = on.double()
        for col, (lo, hi) in ((6, GAMMA), (7, BRIGHTNESS), (8, GAIN), (9, GAIN), (10, GAIN)):
            p[:, col] = torch.where(on, lo + (hi - lo) * r[:, col], p[:, col])
    return p.float()


def validate_params(params, H, W, zoom_max=1.15):
    """ValueError for a record outside the table of tests/augment_ref.py.  Runs on the CPU tensor before upload (B x 12 numbers)."""
    if params.device.type != "cpu" or params.dtype != torch.float32 or params.dim() != 2 or params.shape[1] != REC:
        raise ValueError(f"augmentation records: expected a float32 CPU tensor [B,{REC}], got {params.dtype} "
                         f"{tuple(params.shape)} on {params.device}")
    p = params
    flip, sw, sh, ox, oy, con = (p[:, i] for i in range(6))

    def need(ok, what):
        if not bool(ok.all()):
            raise ValueError(f"augmentation record {int((~ok).nonzero()[0])}: {what}: {p[int((~ok).nonzero()[0])].tolist()}")

    need(torch.isfinite(p).all(dim=1), "not finite")
    need((flip == 0) | (flip == 1), "flip must be 0 or 1")
    need((con == 0) | (con == 1), "colour_on must be 0 or 1")
    for v, name in ((sw, "sw"), (sh, "sh"), (ox, "ox"), (oy, "oy")):
        need(v == torch.floor(v), f"{name} must be an integer")
    need((sw >= W) & (sw <= int(zoom_max * W)), f"sw must lie in [{W}, {int(zoom_max * W)}]")
    need((sh >= H) & (sh <= int(zoom_max * H)), f"sh must lie in [{H}, {int(zoom_max * H)}]")
    need((ox >= 0) & (ox <= sw - W), "ox must lie in [0, sw - W]")
    need((oy >= 0) & (oy <= sh - H), "oy must lie in [0, sh - H]")
    need((p[:, 6] >= GAMMA[0]) & (p[:, 6] <= GAMMA[1]), f"gamma must lie in {list(GAMMA)}")
    need((p[:, 7] >= BRIGHTNESS[0]) & (p[:, 7] <= BRIGHTNESS[1]), f"brightness must lie in {list(BRIGHTNESS)}")
    for i in (8, 9, 10):
        need((p[:, i] >= GAIN[0]) & (p[:, i] <= GAIN[1]), f"channel gain must lie in {list(GAIN)}")
    need(p[:, 11] == 0, "reserved field must be 0")


def _frame_pairs(src, dst):
    pairs = [(src[k], dst[k], k) for k in FRAME_KEYS]
    es, ed = list(src.get("extra_refs", [])), list(dst.get("extra_refs", []))
    pairs += [(s, d, f"extra_refs[{i}]") for i, (s, d) in enumerate(zip(es, ed))]
    seen, out = set(), []
    for s, d, name in pairs:            # the synthetic single-view batch holds one tensor under two keys: one pass writes it
        key = (s.data_ptr(), d.data_ptr())
        if key not in seen:
            seen.add(key)
            out.append((s, d, name))
    return out


def augment_batch(src, dst, params_dev, value_max=255.0):
    """Write the frames (``img_R2``, ``img_R1``, ``img_L2`` and every tensor of ``extra_refs`` present in both) and ``K``,
    ``Kinv``, ``T_R2L``, ``T_R2L_se3`` of the batch dict ``dst`` from ``src`` under the records ``params_dev`` ([B,12] float32 on
    the device; validate them on the host first).  Enqueues two launches on the current stream, nothing else."""
    pairs = _frame_pairs(src, dst)
    B, C, H, W = pairs[0][1].shape
    if C != 3:
        raise ValueError(f"augment_batch: frames must have 3 channels, got {C}")
    spans = []
    for s, d, name in pairs:
        L.dev(s, f"src[{name}]"), L.dev(d, f"dst[{name}]")
        if tuple(s.shape) != (B, C, H, W) or tuple(d.shape) != (B, C, H, W):
            raise ValueError(f"augment_batch: {name}: expected {(B, C, H, W)}, got src {tuple(s.shape)} dst {tuple(d.shape)}")
        spans.append((s.data_ptr(), d.data_ptr(), name))
    nbytes = 4 * B * C * H * W
    for i, (_, d, name) in enumerate(spans):
        for j, (s, d2, other) in enumerate(spans):
            if d < s + nbytes and s < d + nbytes:
                raise ValueError(f"augment_batch: dst[{name}] aliases src[{other}]: the gather reads the whole source frame, "
                                 "in place is refused")
            if i != j and d < d2 + nbytes and d2 < d + nbytes:
                raise ValueError(f"augment_batch: dst[{name}] aliases dst[{other}]")
    L.dev(params_dev, "params")
    if tuple(params_dev.shape) != (B, REC):
        raise ValueError(f"augment_batch: params: expected {(B, REC)}, got {tuple(params_dev.shape)}")
    small = []
    for k, shape in (("K", (B, 3, 3)), ("Kinv", (B, 3, 3)), ("T_R2L", (B, 6)), ("T_R2L_se3", (B, 6))):
        L.dev(src[k], f"src[{k}]"), L.dev(dst[k], f"dst[{k}]")
        if src[k].numel() != dst[k].numel() or tuple(dst[k].shape) != shape:      # (a loader may hand K over as [B,1,3,3])
            raise ValueError(f"augment_batch: {k}: expected {shape}, got src {tuple(src[k].shape)} dst {tuple(dst[k].shape)}")
        small.append(k)
    lib, st = L.lib(), L.stream()
    for i in range(0, len(pairs), MAX_FRAMES):
        chunk = pairs[i:i + MAX_FRAMES]
        L.check(lib.dvf_augment_frames(L.ptr_array([s for s, _, _ in chunk], "src"), L.ptr_array([d for _, d, _ in chunk], "dst"),
                                       len(chunk), params_dev.data_ptr(), B, C, H, W, float(value_max), st), "dvf_augment_frames")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    L.check(lib.dvf_augment_geometry(p(params_dev), *(p(src[k]) for k in small), *(p(dst[k]) for k in small), B, W, H, st),
            "dvf_augment_geometry")
