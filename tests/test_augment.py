"""CPU-side checks of the training augmentation: the record sampler and its validation, the definition
(tests/augment_ref.py) against the CPU oracle's photometric losses -- a mirrored batch must give the SAME loss, which pins the
intrinsics and stereo-pose rules -- the tie between the intrinsics rule and the resample, and the --augment flag."""
import argparse

import pytest
import torch

import augment_ref as R
from dvf import augment
from dvf import cli
from oracle import geometry as og
from oracle import losses as ol

H0, W0 = 64, 128


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_sampler_is_deterministic_and_valid():
    a = augment.sample_params(_gen(7), 4096, H0, W0)
    b = augment.sample_params(_gen(7), 4096, H0, W0)
    assert a.dtype == torch.float32 and a.shape == (4096, 12) and torch.equal(a, b)
    assert not torch.equal(a, augment.sample_params(_gen(8), 4096, H0, W0))
    augment.validate_params(a, H0, W0, 1.15)
    assert torch.equal(a[:, 1:5], a[:, 1:5].round())                       # sw, sh, ox, oy are integers
    assert abs(float(a[:, 0].mean()) - 0.5) < 0.05 and abs(float(a[:, 5].mean()) - 0.5) < 0.05
    assert float(a[:, 1].max()) > W0 and float(a[:, 2].max()) > H0 and float(a[:, 3].max()) > 0 and float(a[:, 4].max()) > 0
    on = a[:, 5] > 0
    assert float(a[on, 7].min()) < 0.6 and float(a[on, 7].max()) > 1.9    # brightness spans its range
    assert torch.equal(a[~on, 6:11], torch.ones_like(a[~on, 6:11]))       # colour off: identity fields


def test_sampler_identity_and_single_ops():
    ident = torch.tensor([R.identity_record(H0, W0)] * 64, dtype=torch.float32)
    assert torch.equal(augment.sample_params(_gen(1), 64, H0, W0, ops=()), ident)
    own = {"flip": [0], "zoom": [1, 2, 3, 4], "colour": [5, 6, 7, 8, 9, 10]}
    for op, cols in own.items():
        p = augment.sample_params(_gen(1), 64, H0, W0, ops=(op,))
        others = [c for c in range(12) if c not in cols]
        assert torch.equal(p[:, others], ident[:, others]), op
        assert not torch.equal(p[:, cols], ident[:, cols]), op
        augment.validate_params(p, H0, W0)


@pytest.mark.parametrize("col,value", [(1, W0 - 1.0), (3, 1.0), (3, 0.5), (6, 0.0), (6, -1.0), (0, 0.5), (11, 1.0)],
                         ids=["sw<W", "ox>sw-W", "ox-fraction", "gamma=0", "gamma<0", "flip-fraction", "reserved"])
def test_validate_params_rejects(col, value):
    p = torch.tensor([R.identity_record(H0, W0)] * 3, dtype=torch.float32)
    if (col, value) == (3, 0.5):
        p[:, 1] = W0 + 4                                                   # room for an offset: only its fraction is wrong
    augment.validate_params(p, H0, W0)
    p[1, col] = value
    with pytest.raises(ValueError, match="record 1"):
        augment.validate_params(p, H0, W0)


def _scene(seed=3, B=2, H=12, W=26):
    g = _gen(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)      # noqa: E731
    frames = [rnd(B, 3, H, W) * 255 for _ in range(3)]                     # R2, R1, L2
    depth = 1 + 9 * rnd(B, H, W)
    K = torch.tensor([[0.58 * W, 0, 0.5 * W + 1.7], [0, 1.92 * H, 0.5 * H - 0.8], [0, 0, 1.0]], dtype=torch.float64)
    K = K.expand(B, 3, 3).contiguous()
    noise = lambda: 0.03 * torch.randn(B, 6, generator=g, dtype=torch.float64)   # noqa: E731
    T_2to1, T_2to1_se3 = noise(), noise()
    T_tr = noise() + torch.tensor([-0.54, 0, 0, 0, 0, 0], dtype=torch.float64)
    T_se3 = noise() + torch.tensor([0, 0, 0, -0.54, 0, 0], dtype=torch.float64)
    return frames, depth, K, torch.inverse(K), T_2to1, T_2to1_se3, T_tr, T_se3


def _flip_only(B, H, W):
    p = torch.tensor([R.identity_record(H, W)] * B, dtype=torch.float64)
    p[:, 0] = 1
    return p


@pytest.mark.parametrize("rotation,padding", [("euler", "zeros"), ("quat", "zeros"), ("euler", "border")])
def test_mirrored_batch_has_the_same_photometric_loss(rotation, padding):
    (r2, r1, l2), depth, K, Kinv, T21, _, T_tr, T_se3 = _scene()
    B, _, H, W = r2.shape
    base = ol.photometric_reconstruction_loss(r2, r1, l2, depth, T21, T_tr, K, Kinv, rotation, padding)
    (f2, f1, fl), K2, Kinv2, T_tr2, _ = R.apply_ref([r2, r1, l2], K, Kinv, T_tr, T_se3, _flip_only(B, H, W))
    T21f = T21 * torch.tensor(R.TR_FLIP, dtype=torch.float64)
    mirrored = ol.photometric_reconstruction_loss(f2, f1, fl, depth.flip(2), T21f, T_tr2, K2, Kinv2, rotation, padding)
    assert float(base) > 1 and abs(float(mirrored) - float(base)) <= 1e-12 * float(base), (float(base), float(mirrored))
    # the reference's rule (cx' = w - cx, custom_transforms.py:55) is one pixel off in this convention: visibly not the same
    K_ref = K2.clone()
    K_ref[:, 0, 2] += 1
    off = ol.photometric_reconstruction_loss(f2, f1, fl, depth.flip(2), T21f, T_tr2, K_ref, torch.inverse(K_ref), rotation, padding)
    assert abs(float(off) - float(base)) > 1e-4 * float(base)


def test_mirrored_batch_has_the_same_dvo_loss():
    (r2, r1, l2), depth, K, Kinv, _, T21, T_tr, T_se3 = _scene()
    B, _, H, W = r2.shape
    base = og.dvo_photometric_loss(r2, l2, r1, depth, T_se3, T21, K)
    (f2, f1, fl), K2, _, _, T_se32 = R.apply_ref([r2, r1, l2], K, Kinv, T_tr, T_se3, _flip_only(B, H, W))
    T21f = T21 * torch.tensor(R.SE3_FLIP, dtype=torch.float64)
    mirrored = og.dvo_photometric_loss(f2, fl, f1, depth.flip(2), T_se32, T21f, K2)
    assert float(base) > 1 and abs(float(mirrored) - float(base)) <= 1e-12 * float(base), (float(base), float(mirrored))


RECORDS = {"flip": [1, 26, 12, 0, 0], "zoom": [0, 29, 13, 2, 1], "both": [1, 28, 13, 1, 0]}


@pytest.mark.parametrize("which", list(RECORDS))
def test_intrinsics_and_their_inverse_stay_inverse(which):
    _, _, K, Kinv, _, _, T_tr, T_se3 = _scene()
    p = torch.tensor([R.identity_record(12, 26)] * 2, dtype=torch.float64)
    p[:, :5] = torch.tensor(RECORDS[which], dtype=torch.float64)
    _, K2, Kinv2, _, _ = R.apply_ref([torch.zeros(2, 3, 12, 26, dtype=torch.float64)], K, Kinv, T_tr, T_se3, p)
    assert float((K2 @ Kinv2 - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12
    assert not torch.equal(K2, K)


def ramp_frames(B, H, W, dtype):
    """Channel 0 holds x, channel 1 holds y, channel 2 a constant."""
    x = torch.arange(W, dtype=dtype).view(1, 1, 1, W).expand(B, 1, H, W)
    y = torch.arange(H, dtype=dtype).view(1, 1, H, 1).expand(B, 1, H, W)
    return torch.cat([x, y, torch.full((B, 1, H, W), 7.0, dtype=dtype)], dim=1).contiguous()


def ramp_residual(out, A, params, H, W):
    """max |A (out0, out1, 1) - (x', y', 1)| over the output pixels whose taps were not clamped (and their number)."""
    B = out.shape[0]
    out = out.double()
    old = torch.stack([out[:, 0], out[:, 1], torch.ones_like(out[:, 0])], dim=1).reshape(B, 3, -1)
    new = (A.double() @ old).reshape(B, 3, H, W)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1).expand(B, H, W)
    _, _, free_x, free_y = R.resample_coords(params.double(), H, W, torch.float64)
    free = free_y[:, :, None] & free_x[:, None, :]
    err = torch.stack([new[:, 0] - xs, new[:, 1] - ys, new[:, 2] - 1], dim=1).abs().amax(1)
    return float(err[free].max()), int(free.sum())


def test_intrinsics_rule_is_the_pixel_map_of_the_resample():
    B, H, W = 2, 12, 26
    p = torch.tensor([R.identity_record(H, W)] * B, dtype=torch.float64)
    p[0, :5] = torch.tensor(RECORDS["zoom"], dtype=torch.float64)
    p[1, :5] = torch.tensor(RECORDS["both"], dtype=torch.float64)
    out = R.resample(ramp_frames(B, H, W, torch.float64), p)
    A, Ainv = R.pixel_map(p, H, W, torch.float64)
    err, n = ramp_residual(out, A, p, H, W)
    assert n > B * H * W // 2 and err < 1e-12 * W, (err, n)
    assert float((A @ Ainv - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12


def test_identity_resample_is_a_bit_exact_copy_or_mirror():
    g = _gen(5)
    for dtype in (torch.float64, torch.float32):
        x = (torch.rand(2, 3, 5, 7, generator=g, dtype=torch.float64) * 255).to(dtype)
        p = torch.tensor([R.identity_record(5, 7)] * 2, dtype=torch.float64)
        p[1, 0] = 1
        out = R.colour(R.resample(x, p), p)
        assert torch.equal(out[0], x[0]) and torch.equal(out[1], x[1].flip(2))


def _parser():
    parser = argparse.ArgumentParser()
    cli.add_common_flags(parser)
    return parser


def test_augment_flag():
    assert _parser().parse_args([]).augment is None
    assert _parser().parse_args(["--augment"]).augment == ("flip", "zoom", "colour")
    assert _parser().parse_args(["--augment", "flip,colour"]).augment == ("flip", "colour")
    assert _parser().parse_args(["--augment", "colour,flip", "--no-graph"]).augment == ("flip", "colour")
    with pytest.raises(SystemExit):
        _parser().parse_args(["--augment", "flip,rotate"])


def test_binding_table_has_the_augmentation_entries():
    from dvf import lib as L
    assert {"dvf_augment_frames", "dvf_augment_geometry"} <= set(L.SIGNATURES)
    lib = L.lib()
    assert lib.dvf_augment_frames(None, None, 3, None, 1, 3, 8, 8, 255.0, None) == -1
    assert lib.dvf_augment_geometry(*([None] * 9), 1, 8, 8, None) == -1
