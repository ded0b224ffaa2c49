"""The two photometric_reconstruction_loss functions reach one dispatcher (dvf/appearance.py::appearance_term) with the same
arguments, so on one scale and two views they must agree to the bit: loss, depth gradient and pose gradient, in each of the
three modes, in deterministic mode.  The image gradients are not compared: the fused backward scatters them with float
atomics."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, C, H, W = 2, 3, 20, 72          # one tile boundary in each axis of the 64x16 window tiles, W divisible by 4

_MODES = {"l1": {}, "ssim": dict(ssim_weight=0.85), "minreproj": dict(ssim_weight=0.85, min_reprojection=True, auto_mask=True)}


@pytest.mark.parametrize("mode", sorted(_MODES))
def test_single_and_multi_scale_functions_agree_bitwise(mode):
    import loss_functions as LF
    import loss_functions_sfm as LS
    from dvf import conv
    from dvf.synthetic import synthetic_batch
    batch = synthetic_batch(B, H, W, seed=7, device=DEV)
    tgt, R1, L2 = (batch[k] / 255.0 for k in ("img_R2", "img_R1", "img_L2"))
    K, Kinv = batch["K"], batch["Kinv"]
    gen = torch.Generator().manual_seed(11)
    depth = (1.0 + 9.0 * torch.rand(B, 1, H, W, generator=gen)).to(DEV).requires_grad_(True)
    pose = 0.02 * torch.randn(B, 2, 6, generator=gen)
    pose[:, 1, 0] -= 0.54
    pose = pose.to(DEV).requires_grad_(True)

    def run(fn):
        depth.grad = pose.grad = None
        loss = fn()
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), depth.grad.clone(), pose.grad.clone()

    was = conv.DETERMINISTIC
    conv.set_deterministic(True)
    try:
        multi = run(lambda: LS.photometric_reconstruction_loss(tgt, [R1, L2], K, Kinv, [depth], [None], pose, **_MODES[mode]))
        single = run(lambda: LF.photometric_reconstruction_loss(tgt, R1, L2, depth[:, 0], pose[:, 0], pose[:, 1], K, Kinv,
                                                                **_MODES[mode]))
    finally:
        conv.set_deterministic(was)
    assert torch.isfinite(multi[0]) and float(multi[0]) > 0
    for name, m, s in zip(("loss", "depth gradient", "pose gradient"), multi, single):
        assert float(m.abs().max()) > 0, name
        assert torch.equal(m, s), (name, float((m - s).abs().max()))
