"""CPU: the inputs of tests/smooth_seams.py are what tests/test_gpu_smooth_seams.py relies on, asserted on the fp64 oracle
alone.  Every one of the four partial sums contributes; in the float family no second difference is near 0 (every sign is
determinate in fp32); in the integer family exact zeros occur in every term, the fp32 oracle's differences are the fp64 ones
bit for bit, and an exactly-zero gradient element is zero term by term."""
import pytest
import torch

import smooth_seams as S
from oracle import losses as ol

IDS = ["%dx%dx%dx%d" % s for s in S.SHAPES]


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("shape", list(S.SHAPES), ids=IDS)
def test_every_partial_sum_contributes(shape, family):
    m = S.make(shape, family)
    assert m.dtype == torch.float32 and tuple(m.shape) == shape
    sums = S.term_sums(m)
    assert all(s > 0 for s in sums), sums
    loss, (grad,) = S.oracle([m])
    assert float(loss) > 0.1 and float(grad.abs().max()) > 0          # (13.8 at 5x65, integer family)


@pytest.mark.parametrize("shape", list(S.SHAPES), ids=IDS)
def test_float_family_signs_are_determinate(shape):
    """|second difference| >= 1e-4: fp32 forms it from values below 11 with three roundings, an error below 4e-6."""
    m = S.make(shape, "float")
    assert float(m.min()) >= 0.5 and float(m.max()) <= 10.5
    assert S.min_abs_term(m) >= 1e-4, S.min_abs_term(m)


@pytest.mark.parametrize("shape", list(S.SHAPES), ids=IDS)
def test_int_family_is_exact_and_has_zeros(shape):
    m = S.make(shape, "int")
    assert torch.equal(m, m.round()) and float(m.min()) >= -3 and float(m.max()) <= 3
    for t32, t64 in zip(ol._second_order_terms(m), ol._second_order_terms(m.double())):
        assert torch.equal(t32.double(), t64)
    structural, zeros = S.zero_is_structural(m)
    assert structural
    (x0, x1), (y0, y1) = S.flat_band(*shape[2:])
    if m.numel() >= 64:
        assert all(n > 0 for n in S.zero_terms(m)), S.zero_terms(m)
        grad = S.oracle([m])[1][0]
        inner = grad[:, :, y0 + 2:y1 - 2, :] if (x0, x1) == (0, shape[3]) else grad[:, :, :, x0 + 2:x1 - (2 if x1 < shape[3] else 0)]
        assert inner.numel() >= 4 * shape[0] * shape[1] * min(shape[2:]) and bool((inner == 0).all()) and zeros >= inner.numel()
        assert x0 < S.SX <= x1 or y0 < 15 * S.SY <= y1                  # the band ends at or crosses a tile seam
    else:                               # (2x1x3x3: 6 + 8 + 8 + 6 differences, 18 elements touched by up to 12 stencils each)
        assert (x1, y1) == (0, 0) and sum(S.zero_terms(m)) >= 3, S.zero_terms(m)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_multi_scale_inputs(family):
    maps = S.make_multi(family)
    assert [tuple(m.shape) for m in maps] == [(S.MULTI_B, 1, h, w) for h, w in S.MULTI]
    for m in maps:
        assert all(s > 0 for s in S.term_sums(m))
        if family == "float":
            assert S.min_abs_term(m) >= 1e-4
        else:
            assert S.zero_is_structural(m)[0]
    l2, _ = S.oracle(maps, 2)
    l1, _ = S.oracle(maps, 1)
    first, _ = S.oracle(maps[:1])
    assert abs(float(l2) - (float(first) + (float(l1) - float(first)) / 2)) < 1e-12 * float(l2)   # w_1 = w_0 / 2


def test_shapes_cross_the_seams_they_claim():
    for (b, c, h, w), what in S.SHAPES.items():
        assert h >= 3 and w >= 3 and what
    ws, hs = {s[3] for s in S.SHAPES}, {s[2] for s in S.SHAPES}
    assert {S.SX, S.SX + 1, S.SX + 2, S.SX + 3, 2 * S.SX + 2} <= ws and any(w > 3 * S.SX for w in ws)
    assert {S.SY, S.SY + 1, S.SY + 2, S.SY + 3} <= hs and any(h % S.SY for h in hs) and 3 in ws and 3 in hs
