"""unsupervise_losses discards the explainability masks of the pose network (as the reference's unsupervise.py:95 does) and
asks the network not to compute them (need_masks=False): at 2x3x64x208 in deterministic mode the loss terms and the whole
gradient arena are bit-equal with and without the skip, no stride-2 4x4 transposed convolution runs during the skipped
step, and pose_net(...) with defaults still returns four masks."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t4x4s2(geoms):
    """Logged geometries (dvf.conv.GEOM_LOG) of 4x4 stride-2 transposed convolutions: only the mask decoder has them."""
    return [g for g in geoms if g[2][0] == 4 and g[2][1] == 2 and g[2][4]]


def test_unsupervise_skips_the_mask_decoder_bit_exactly(monkeypatch):
    import DispNetS
    import PoseExpNet
    from dvf import conv as C
    from dvf import lib as L
    from dvf import steps as S
    from dvf.engine import FlatAdam
    from dvf.synthetic import synthetic_batch
    torch.manual_seed(0)
    disp, pose = DispNetS.DispNetS(), PoseExpNet.PoseExpNet(output_exp=True)
    disp.init_weights(); pose.init_weights()
    disp.to(DEV).train(); pose.to(DEV).train()
    opt = FlatAdam(list(pose.parameters()) + list(disp.parameters()), lr=1e-3, weight_decay=1e-8, overlap=False)
    batch = synthetic_batch(2, 64, 208, seed=1234, device=DEV)

    def fwd_bwd():
        with C.geom_log() as geoms, L.plan_log() as log:
            loss, terms = S.unsupervise_losses(disp, pose, batch)
            opt.zero_grad()
            loss.backward()
            opt.join_wgrad()
            L.join_aux_streams()
            torch.cuda.synchronize()
        return {k: v.clone() for k, v in terms.items()}, opt.flat_g.clone(), geoms, log.records

    C.set_deterministic(True)
    try:
        terms_skip, grads_skip, geoms_skip, plans_skip = fwd_bwd()
        with monkeypatch.context() as m:
            m.setattr(S, "_pose_only", lambda net, frames: net(frames))      # the masks computed and discarded
            terms_full, grads_full, geoms_full, plans_full = fwd_bwd()
    finally:
        C.set_deterministic(False)
    assert len(_t4x4s2(geoms_full)) == 5, _t4x4s2(geoms_full)               # upconv5 .. upconv1 ran when asked to
    assert len(plans_full) > len(plans_skip) > 0, (len(plans_full), len(plans_skip))
    assert not _t4x4s2(geoms_skip), _t4x4s2(geoms_skip)
    # (dconvt_fwd: the thin transposed layers' direct kernel -- upconv1, 32 -> 16)
    assert not any(p.kernel == L.K_DCONVT_FWD and p.KH == 4 for p in plans_skip), sorted(plans_skip)
    assert len(geoms_full) - len(geoms_skip) == 9, (len(geoms_full), len(geoms_skip))   # five upconvs, four mask heads
    assert terms_skip.keys() == terms_full.keys()
    for k in terms_full:
        assert torch.equal(terms_skip[k], terms_full[k]), (k, float(terms_skip[k]), float(terms_full[k]))
    assert float(grads_full.abs().max()) > 0
    assert torch.equal(grads_skip, grads_full), float((grads_skip - grads_full).abs().max())


def test_pose_net_returns_four_masks_by_default():
    import PoseExpNet
    import PoseExpNet_sfm
    torch.manual_seed(1)
    a, b = torch.rand(2, 3, 64, 208, device=DEV), torch.rand(2, 3, 64, 208, device=DEV)
    net = PoseExpNet.PoseExpNet(output_exp=True).to(DEV).train()
    masks, pose = net((a, b))
    assert len(masks) == 4 and [tuple(m.shape) for m in masks] == [(2, 2, 64 >> i, 208 >> i) for i in range(4)]
    none, pose2 = net((a, b), need_masks=False)
    assert none == [None] * 4 and torch.equal(pose, pose2) and tuple(pose.shape) == (2, 6)
    net.eval()
    with torch.no_grad():
        m0, _ = net((a, b))
    assert tuple(m0.shape) == (2, 2, 64, 208)
    sfm = PoseExpNet_sfm.PoseExpNet(nb_ref_imgs=2, output_exp=True).to(DEV).train()
    assert sorted(sfm.state_dict()) == sorted(net.state_dict())
    masks, pose = sfm(a, [b, a])
    assert len(masks) == 4 and all(m is not None for m in masks) and tuple(pose.shape) == (2, 2, 6)
    none, pose2 = sfm(a, [b, a], need_masks=False)
    assert none == [None] * 4 and torch.equal(pose, pose2)
