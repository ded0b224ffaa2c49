"""The augmentation kernels (csrc/augment.hip through dvf.augment.augment_batch) against the definition in
tests/augment_ref.py (fp64), on shapes that cover odd widths, the scalar tail of the 16-byte stores, clamped taps on every
side and more than one launch geometry; then the equivariance of the PRODUCT losses under a flip-only record."""
import pytest
import torch

import augment_ref as R
from conftest import rel_err
from dvf import augment
from test_augment import ramp_frames, ramp_residual

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (8, 16), (12, 26)]
CASES = [(h, w, f) for (h, w) in SHAPES for f in (3, 5)]
B = 3
SMALL = ("K", "Kinv", "T_R2L", "T_R2L_se3")
TOL = 1e-4                    # the suite's fp32 parity bound (conftest.rel_err)


def _batch(H, W, F, seed=0, zeros=False):
    """CPU float32 batch dict with F frames (3 keyed ones + F-3 extra_refs), off-centre K, noisy stereo poses."""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    frames = [torch.rand(B, 3, H, W, generator=g) * 255 for _ in range(F)]
    if zeros:
        for f in frames:
            f[:, :, ::2, 1::3] = 0.0
    K = torch.tensor([[0.58 * W, 0, 0.5 * W + 1.7], [0, 1.92 * H, 0.5 * H - 0.8], [0, 0, 1.0]], dtype=torch.float64)
    K = K.expand(B, 3, 3).contiguous()
    noise = lambda: 0.03 * torch.randn(B, 6, generator=g)      # noqa: E731
    return {"img_R2": frames[0], "img_R1": frames[1], "img_L2": frames[2], "extra_refs": frames[3:],
            "K": K.float(), "Kinv": torch.inverse(K).float().contiguous(),
            "T_R2L": noise() + torch.tensor([-0.54, 0, 0, 0, 0, 0]),
            "T_R2L_se3": noise() + torch.tensor([0, 0, 0, -0.54, 0, 0])}


def _frames(b):
    return [b["img_R2"], b["img_R1"], b["img_L2"]] + list(b["extra_refs"])


def _cuda(b):
    return {k: ([t.cuda() for t in v] if isinstance(v, list) else v.cuda()) for k, v in b.items()}


def _run(src_cpu, params, value_max=255.0):
    src = _cuda(src_cpu)
    dst = {k: ([torch.full_like(t, -7.0) for t in v] if isinstance(v, list) else torch.full_like(v, -7.0)) for k, v in src.items()}
    augment.augment_batch(src, dst, params.float().cuda(), value_max)
    torch.cuda.synchronize()
    for a, b in zip(_frames(src), _frames(src_cpu)):
        assert torch.equal(a.cpu(), b)                                        # the source is only read
    return {k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in dst.items()}


def _ref(src_cpu, params, value_max=255.0):
    d = lambda t: t.double()                                                   # noqa: E731
    frames, K, Kinv, T_tr, T_se3 = R.apply_ref([d(f) for f in _frames(src_cpu)], d(src_cpu["K"]), d(src_cpu["Kinv"]),
                                               d(src_cpu["T_R2L"]), d(src_cpu["T_R2L_se3"]), d(params), value_max)
    return frames, {"K": K, "Kinv": Kinv, "T_R2L": T_tr, "T_R2L_se3": T_se3}


def _records(H, W, rows):
    """rows: per sample a dict of field overrides on the identity record."""
    p = torch.tensor([R.identity_record(H, W)] * len(rows), dtype=torch.float64)
    names = ["flip", "sw", "sh", "ox", "oy", "colour_on", "gamma", "brightness", "gr", "gg", "gb"]
    for i, row in enumerate(rows):
        for k, v in row.items():
            p[i, names.index(k)] = v
    augment.validate_params(p.float(), H, W)
    return p


@pytest.mark.parametrize("H,W,F", CASES)
def test_identity_record_copies_every_key(H, W, F):
    src = _batch(H, W, F)
    out = _run(src, _records(H, W, [{}] * B))
    for a, b in zip(_frames(out), _frames(src)):
        assert torch.equal(a, b)
    for k in SMALL:
        assert torch.equal(out[k], src[k]), k


@pytest.mark.parametrize("H,W,F", CASES)
def test_flip_only(H, W, F):
    src = _batch(H, W, F)
    p = _records(H, W, [{"flip": 1}, {}, {"flip": 1}])
    out = _run(src, p)
    for a, b in zip(_frames(out), _frames(src)):
        assert torch.equal(a[0], b[0].flip(2)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2].flip(2))
    _, small = _ref(src, p)
    for k in SMALL:
        assert rel_err(out[k], small[k]) < 1e-6, (k, rel_err(out[k], small[k]))
        assert torch.equal(out[k][1], src[k][1]), k
    assert float(out["T_R2L"][0, 0]) > 0.4 and float(out["T_R2L_se3"][0, 3]) > 0.4      # the baseline changed sign


@pytest.mark.parametrize("H,W,F", CASES)
def test_edges_of_the_largest_zoom(H, W, F):
    """sw = int(1.15 W), sh = int(1.15 H), crop at the top-left and at the bottom-right corner, with and without flip: the
    clamped left / top and right / bottom taps, the vector tail and odd widths."""
    sw, sh = int(1.15 * W), int(1.15 * H)
    z = {"sw": sw, "sh": sh}
    lo, hi = dict(z, ox=0, oy=0), dict(z, ox=sw - W, oy=sh - H)
    src = _batch(H, W, F)
    for rows in ([lo, dict(hi, flip=1), dict(lo, flip=1)], [hi, dict(lo, flip=1), dict(hi, flip=1)]):
        p = _records(H, W, rows)
        out = _run(src, p)
        frames, small = _ref(src, p)
        for i, (a, b) in enumerate(zip(_frames(out), frames)):
            assert rel_err(a, b) < TOL, (i, rel_err(a, b))
        for k in SMALL:
            assert rel_err(out[k], small[k]) < 1e-6, k


@pytest.mark.parametrize("H,W,F", CASES)
def test_colour(H, W, F):
    """gamma and brightness at both ends of their ranges (brightness 2 hits the clamp at value_max), distinct gains, exact
    zeros in the input; the colour_on = 0 sample of the same batch is bit-identical to the colour-free result."""
    sw, sh = int(1.15 * W), int(1.15 * H)
    zoom = {"sw": sw, "sh": sh, "ox": sw - W, "oy": 0}
    rows = [{"flip": 1, "colour_on": 1, "gamma": 0.8, "brightness": 2.0, "gr": 0.8, "gg": 1.0, "gb": 1.2},
            dict(zoom, colour_on=1, gamma=1.2, brightness=0.5, gr=1.2, gg=0.9, gb=0.8),
            dict(zoom, flip=1, colour_on=0, gamma=1.2, brightness=2.0, gr=1.2, gg=0.9, gb=0.8)]
    src = _batch(H, W, F, zeros=True)
    p = _records(H, W, rows)
    out = _run(src, p)
    frames, _ = _ref(src, p)
    for i, (a, b) in enumerate(zip(_frames(out), frames)):
        assert rel_err(a, b) < TOL, (i, rel_err(a, b))
        assert float(a.max()) == 255.0 and float(a.min()) == 0.0               # clamp reached; 0 stays 0
        assert bool((a[0][src_zero(src, i).flip(2)] == 0).all())
    plain = _run(src, _records(H, W, [dict(r, colour_on=0) for r in rows]))
    for a, b in zip(_frames(out), _frames(plain)):
        assert torch.equal(a[2], b[2])
        assert not torch.equal(a[1], b[1])


def src_zero(src, i):
    return _frames(src)[i][0] == 0


@pytest.mark.parametrize("H,W,F", CASES)
def test_ramp_ties_intrinsics_to_resample(H, W, F):
    """Frames holding (x, y): A (out0, out1, 1) = (x', y', 1) wherever no tap was clamped, with A read back from the geometry
    kernel (K = I: K' = A M)."""
    sw, sh = int(1.15 * W), int(1.15 * H)
    rows = [{"sw": sw, "sh": sh, "ox": (sw - W) // 2, "oy": (sh - H) // 2},
            {"sw": sw, "sh": sh, "ox": sw - W, "oy": 0, "flip": 1},
            {"flip": 1}]
    p = _records(H, W, rows)
    ramp = ramp_frames(B, H, W, torch.float32)
    eye = torch.eye(3).expand(B, 3, 3).contiguous()
    src = dict(_batch(H, W, F), K=eye, Kinv=eye.clone())
    src.update(img_R2=ramp, img_R1=ramp.clone(), img_L2=ramp.clone(), extra_refs=[ramp.clone() for _ in range(F - 3)])
    out = _run(src, p)
    M = torch.diag_embed(torch.stack([1 - 2 * p[:, 0], torch.ones(B, dtype=torch.float64), torch.ones(B, dtype=torch.float64)], 1))
    A = out["K"].double() @ M
    for f in _frames(out):
        err, n = ramp_residual(f, A, p, H, W)
        assert n >= H * W and err < 1e-5 * W, (err, n)
    assert rel_err(out["K"].double() @ out["Kinv"].double(), torch.eye(3, dtype=torch.float64).expand(B, 3, 3)) < 1e-5


# ---------------------------------------------------------------------------------------------- product losses
def _scene(B2=2, H=32, W=104):
    from dvf.synthetic import synthetic_batch
    g = torch.Generator().manual_seed(11)
    b = synthetic_batch(B2, H, W, seed=5)
    K = b["K"].double().clone()
    K[:, 0, 2] += 1.7
    K[:, 1, 2] -= 0.8
    b["K"], b["Kinv"] = K.float(), torch.inverse(K).float().contiguous()
    b["T_R2L"] = b["T_R2L"] + 0.03 * torch.randn(B2, 6, generator=g)
    b["T_R2L_se3"] = b["T_R2L_se3"] + 0.03 * torch.randn(B2, 6, generator=g)
    depth = 1 + 9 * torch.rand(B2, H, W, generator=g)
    T21 = 0.03 * torch.randn(B2, 6, generator=g)
    p = torch.tensor([R.identity_record(H, W)] * B2, dtype=torch.float32)
    p[:, 0] = 1
    src = _cuda(b)
    dst = {k: ([torch.empty_like(t) for t in v] if isinstance(v, list) else torch.empty_like(v)) for k, v in src.items()}
    augment.augment_batch(src, dst, p.cuda())
    return src, dst, depth.cuda(), T21.cuda()


def test_flip_equivariance_of_the_photometric_loss():
    import loss_functions
    src, dst, depth, T21 = _scene()

    def loss(b, d, t):
        return float(loss_functions.photometric_reconstruction_loss(b["img_R2"], b["img_R1"], b["img_L2"], d, t, b["T_R2L"],
                                                                    b["K"], b["Kinv"], padding_mode="border"))

    base = loss(src, depth, T21)
    mirrored = loss(dst, depth.flip(2).contiguous(), (T21 * torch.tensor(R.TR_FLIP, device="cuda")).contiguous())
    print("photometric, border:", base, mirrored)
    assert base > 1 and abs(mirrored - base) <= 1e-4 * base, (base, mirrored)


def test_flip_equivariance_of_the_se3_pixel_front_end():
    from dvf import lib as L
    from dvf.ops import PhotoLossFn
    src, dst, depth, T21 = _scene()

    def loss(b, d, t):
        pose = torch.stack((b["T_R2L_se3"], t), dim=0).contiguous()
        return float(PhotoLossFn.apply(b["img_R2"], d, pose, b["K"], b["Kinv"], None, L.POSE_SE3 | L.PIXEL_COORDS,
                                       b["img_L2"], b["img_R1"]))

    base = loss(src, depth, T21)
    mirrored = loss(dst, depth.flip(2).contiguous(), (T21 * torch.tensor(R.SE3_FLIP, device="cuda")).contiguous())
    print("se3 / pixel coordinates:", base, mirrored)
    assert base > 1 and abs(mirrored - base) <= 1e-4 * base, (base, mirrored)


# ---------------------------------------------------------------------------------------------- refusals
def test_wrapper_refusals():
    H, W = 8, 16
    cpu = _batch(H, W, 3)
    p = _records(H, W, [{"flip": 1}] * B).float()
    src = _cuda(cpu)
    dst = {k: ([torch.full_like(t, -7.0) for t in v] if isinstance(v, list) else torch.full_like(v, -7.0)) for k, v in src.items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        augment.augment_batch(cpu, dst, p.cuda())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        augment.augment_batch(src, dst, p)
    with pytest.raises(ValueError, match="aliases"):
        augment.augment_batch(src, dict(dst, img_R1=src["img_R1"]), p.cuda())
    with pytest.raises(ValueError, match="aliases"):
        augment.augment_batch(src, dict(dst, img_R1=dst["img_R2"]), p.cuda())
    with pytest.raises(ValueError, match="expected"):
        augment.augment_batch(src, dict(dst, img_L2=torch.empty(B, 3, H, W + 4, device="cuda")), p.cuda())
    with pytest.raises(ValueError, match="expected"):
        augment.augment_batch(src, dst, p[:2].cuda())
    with pytest.raises(RuntimeError, match="contiguous"):
        augment.augment_batch(dict(src, img_R2=src["img_R2"].transpose(2, 3).contiguous().transpose(2, 3)), dst, p.cuda())
    torch.cuda.synchronize()
    for t in _frames(dst) + [dst[k] for k in SMALL]:
        assert bool((t == -7.0).all())                                         # nothing was launched
    # the C entry itself refuses an overlap, before any launch
    from dvf import lib as L
    arr = L.ptr_array([src["img_R2"]])
    assert L.lib().dvf_augment_frames(arr, arr, 1, p.cuda().data_ptr(), B, 3, H, W, 255.0, L.stream()) == -1
