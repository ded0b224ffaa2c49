"""CPU side of the integer-exact convolution tests (tests/conv_exact.py, tests/test_gpu_conv_exact.py): for every geometry
table available without a GPU, the operand budget holds at full size, and the fp64 reference of a one-image instance drawn
with those amplitudes is integral, inside fp32's exact range and inside the bounds the budget computed."""
import pytest

import conv_exact as X
import test_gpu_conv as TC
import test_gpu_conv_fuzz as TF
import test_gpu_conv_exact as TE

GEOMS = [(c[0], X.case_geom(c)) for c in TC.CASES] + [(c[0], X.fuzz_geom(c)) for c in TF.CASES] + list(TE.EXTRA_CASES)


@pytest.mark.parametrize("name,geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_budget_and_integral_reference(name, geom):
    if geom[2][5] == X.ACT_SIGMOID_AFFINE:
        geom = X.with_act(geom, X.ACT_NONE)          # (the exact run of a sigmoid layer)
    amps, bd = X.budget(geom, acc=TE.ACC_AMP)
    assert all(v <= X.LIMIT for v in bd.values()), bd
    assert min(amps.values()) >= 1
    segs, cout, cfg, (n, h, w), need_in = geom
    small = (segs, cout, cfg, (1, h, w), need_in)
    ops = X.Operands(small, X.seed_of(name))
    # the reduced instance is drawn at the full-size amplitudes (the budget only shrinks with N)
    assert X.budget(small)[0]["x"] >= amps["x"] and X.budget(small)[0]["g"] >= amps["g"]
    for relu_in in (False, True):
        ref = X.Reference(small, ops, relu_in)           # asserts integrality and |v| < 2^24
        sb = X.bounds(small, ops.amps)
        assert float(ref.pre.abs().max()) <= sb["fwd"]
        assert float(ref.dw.abs().max()) <= sb["wgrad"] and float(ref.db.abs().max()) <= sb["bias"]
        assert all(float(g.abs().max()) <= sb["dgrad"] for g in ref.dxs if g is not None)
    # a visible share of exact zeros in weight, bias and gout; every input segment carries non-zero values
    assert float((ops.wt == 0).double().mean()) > 0.2 and float((ops.gout == 0).double().mean()) > 0.2
    assert all(float(x.abs().max()) >= 1 for x in ops.xs)


def test_budget_shrinks_to_unit_amplitudes_and_refuses_beyond():
    # cfg 3's FeatExtractor stem: 24 images of 256x832 -> 5.1M terms per weight-gradient entry
    geom = ((3,), 32, (3, 1, 1, 0, False, 1, 1.0, 0.0, None), (24, 256, 832), (False,))
    amps, bd = X.budget(geom)
    assert bd["wgrad"] <= X.LIMIT and amps["g"] == 1 and amps["x"] == 3
    huge = ((3,), 32, (3, 1, 1, 0, False, 1, 1.0, 0.0, None), (64, 512, 1024), (False,))
    with pytest.raises(AssertionError, match="no integer budget"):
        X.budget(huge)
