"""CPU: the cases of tests/geometry_cases.py are determinate, asserted on the fp64 oracle alone, per operand combination.
Behind-camera family: both counts (behind the camera, overwritten in front of it) are positive and some pixels stay inside;
no p_z lies within 1e-4 of the 1e-3 clamp (nor in (1e-3, 0.25): see the module's docstring); no normalised coordinate lies
within 1e-4 of +-1; the clamped point of every behind-camera pixel misses the image by a pixel or more along both axes, so
fp32 and fp64 put it out on the same side (the argument of warp_exact.behind_is_determinate).  fp32's own coordinate error
is about 1e-5 of a p_x of 10 over Z = 1e-3, a hundredth of a pixel.

Counts (behind the camera / overwritten by the zeros padding / pixels), the same for every operand combination:
(1,2,2) 2 / 3 / 4; (3,5,130) 767 / 1784 / 1950; (2,91,91) 6703 / 15140 / 16562."""
import pytest
import torch

import geometry_cases as G
from conftest import rel_err

IDS = ["%dx%dx%d" % s for s in G.SHAPES]
COUNTS = {(1, 2, 2): (2, 3, 4), (3, 5, 130): (767, 1784, 1950), (2, 91, 91): (6703, 15140, 16562)}


@pytest.fixture(scope="module")
def cases():
    return {(s, f): G.make(s, f) for s in G.SHAPES for f in G.FAMILIES}


@pytest.mark.parametrize("combo", G.COMBOS)
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_behind_family_is_determinate(cases, shape, combo):
    case = cases[(shape, "behind")]
    assert float(case.depth.min()) >= 0.5 and float(case.depth.max()) <= 4.0 and bool((case.vec[:, 2] == -2).all())
    n = G.census(*G.operands(case, combo))
    assert (n.behind, n.overwritten, n.pixels) == COUNTS[shape]
    assert n.behind > 0 and n.overwritten > n.behind and n.inside > 0
    assert n.pz_margin >= 1e-4 and n.min_front_pz >= 0.25
    assert n.edge_margin >= 1e-4
    assert n.behind_miss >= 1.0


@pytest.mark.parametrize("combo", G.COMBOS)
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_front_family_is_determinate(cases, shape, combo):
    n = G.census(*G.operands(cases[(shape, "front")], combo))
    assert n.behind == 0 and n.inside > 0 and n.overwritten > 0 and n.min_front_pz >= 1.5
    assert n.edge_margin >= 1e-4


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_operand_combinations_reach_the_same_points(cases, shape, family):
    case = cases[(shape, family)]
    base = G.project(*G.operands(case, "rot+tr"))[0]
    for combo in G.COMBOS[1:]:
        cam, rot, tr = G.operands(case, combo)
        assert (rot is None) == (combo in ("no_rot", "neither")) and (tr is None) == (combo in ("no_tr", "neither"))
        assert rel_err(G.project(cam, rot, tr)[0], base) < 1e-6


def test_chunk_arithmetic_of_the_shapes():
    chunks = {s: (s[1] * s[2] + G.CHUNK - 1) // G.CHUNK for s in G.SHAPES}
    assert chunks == {(1, 2, 2): 1, (3, 5, 130): 1, (2, 91, 91): 2}
    hw = 91 * 91
    per = (hw + 1) // 2
    assert (per, hw - per) == (4141, 4140)              # a short last chunk


@pytest.mark.parametrize("pad", ["zeros", "border"])
@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("shape", G.SHAPES, ids=IDS)
def test_fp32_oracle_meets_the_bounds_asked_of_the_kernel(cases, shape, family, pad):
    """The oracle itself in fp32 on the same operands against fp64: forward values within 1e-5 and the gradients within
    1e-4, over all pixels and over the pixels in front of the camera alone -- the bounds are ones fp32 can meet."""
    from oracle import geometry as og
    case = cases[(shape, family)]
    cam, rot, tr = G.operands(case, "rot+tr")
    ref = G.oracle_cam2pixel(cam, rot, tr, pad, case.gg)
    leaves = [x.clone().requires_grad_(True) for x in (cam, rot, tr)]
    grid = og.cam2pixel(*leaves, pad)
    (grid * case.gg).sum().backward()
    front = G.project(cam, rot, tr)[0][:, 2] >= 1e-3
    errs = [rel_err(grid, ref[0]), rel_err(grid[front], ref[0][front])] + [rel_err(x.grad, r) for x, r in zip(leaves, ref[1:])]
    errs.append(rel_err(leaves[0].grad.permute(0, 2, 3, 1)[front], ref[1].permute(0, 2, 3, 1)[front]))
    print(shape, family, pad, " ".join("%.2g" % e for e in errs))
    assert errs[0] < 1e-5 and errs[1] < 1e-5 and all(e < 1e-4 for e in errs[2:])


def test_pose_vectors():
    for mode in ("euler", "quat"):
        v = G.pose_vectors(mode)
        assert tuple(v.shape) == (G.N_POSE, 6) and bool((v[0] == 0).all()) and G.N_POSE % 64 and G.N_POSE > 128
    v = G.pose_vectors("se3")
    theta = v[:, :3].double().norm(dim=1)
    assert bool((v[:4, :3] == 0).all()) and bool((v[:4, 3:] != 0).all())
    assert bool(((theta[4:8] - 1).abs() <= 0.11).all())
    assert bool(((theta[8:12] - 1e-3).abs() < 1e-6).all()) and bool((theta[4:] ** 2 >= 1e-8).all())   # far from theta^2 = 1e-12
    out, grad = G.oracle_pose(v, "se3", torch.ones(G.N_POSE, 3, 4))
    eye = torch.eye(3, dtype=torch.float64)
    assert torch.equal(out[:4, :, :3], eye.expand(4, 3, 3)) and torch.equal(out[:4, :, 3], v[:4, 3:].double())
    assert bool(torch.isfinite(grad).all()) and float(grad[:4, :3].abs().max()) > 0
