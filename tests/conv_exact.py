"""Integer-exact operands and fp64 references for the convolution kernels (tests/test_gpu_conv_exact.py).

Every operand is a small integer and every reduction is budgeted so that no partial sum, in any order, leaves the range
|v| <= 2^24 where fp32 represents every integer: MFMA tiles, split-K partials, float atomics and ordered finishes then all
give the same, exact result, and a kernel must equal an fp64 reference bit for bit.  A dropped or doubled tap, pixel,
channel or K-chunk is a hard failure however small it is next to the tensor's maximum.

Budget per geometry (worst case of every term at full amplitude):
  forward            A_b + cin * k^2 * A_x * A_w
  input gradient     cout * k^2 * A_g * A_w
  weight / bias grad N * oh * ow * A_x * A_g  (+ A_i: the initial value of an accumulating call)
Amplitudes start at A_x = A_w = A_g = 3, A_b = 7 and shrink (down to {-1, 0, 1}) until every bound is <= 2^24."""
import zlib

import torch
import torch.nn.functional as F

LIMIT = 1 << 24
ACT_NONE, ACT_RELU, ACT_SIGMOID_AFFINE = 0, 1, 2


def out_size(h, k, stride, pad, opad, transposed):
    return (h - 1) * stride - 2 * pad + k + opad if transposed else (h + 2 * pad - k) // stride + 1


def out_hw_of(geom):
    segs, cout, cfg, (n, h, w), _ = geom
    k, stride, pad, opad, transposed, act, alpha, beta, crop = cfg
    oh, ow = out_size(h, k, stride, pad, opad, transposed), out_size(w, k, stride, pad, opad, transposed)
    if crop is not None:
        oh, ow = min(oh, crop[0]), min(ow, crop[1])
    return oh, ow


def seg_amps(segs, ax):
    """Per-segment input amplitudes: one-channel segments (disparity maps) +-1, the others alternate ax, ax - 1 -- a wrong
    segment base or stride reads values of another amplitude."""
    return [1 if c == 1 else (ax if s % 2 == 0 else max(1, ax - 1)) for s, c in enumerate(segs)]


def bounds(geom, amps, acc=0):
    segs, cout, cfg, (n, h, w), _ = geom
    k = cfg[0]
    oh, ow = out_hw_of(geom)
    ax = max(seg_amps(segs, amps["x"]))
    return {"fwd": amps["b"] + sum(segs) * k * k * ax * amps["w"],
            "dgrad": cout * k * k * amps["g"] * amps["w"],
            "wgrad": n * oh * ow * ax * amps["g"] + acc,
            "bias": n * oh * ow * amps["g"] + acc}


def budget(geom, acc=0):
    """Largest amplitudes (from A_x = A_w = A_g = 3, A_b = 7) whose worst-case sums all stay <= 2^24; raises if even
    {-1, 0, 1} operands cannot keep them there."""
    amps = {"x": 3, "w": 3, "g": 3, "b": 7}
    while True:
        bd = bounds(geom, amps, acc)
        if bd["wgrad"] > LIMIT or bd["bias"] > LIMIT:
            key = "g" if amps["g"] > 1 else "x"
        elif bd["fwd"] > LIMIT:
            key = "w" if amps["w"] > 1 else ("x" if amps["x"] > 1 else "b")
        elif bd["dgrad"] > LIMIT:
            key = "w" if amps["w"] > 1 else "g"
        else:
            return amps, bd
        if amps[key] <= 1:
            raise AssertionError(f"no integer budget for {geom}: {bd}")
        amps[key] -= 1


def _ints(shape, amp, gen, zero_share=0.0):
    v = torch.randint(-amp, amp + 1, tuple(shape), generator=gen, dtype=torch.int64)
    if zero_share > 0:
        v = v * (torch.rand(tuple(shape), generator=gen) >= zero_share)
    return v.to(torch.float32)


class Operands:
    """Seeded integer operands of one geometry: per-segment inputs xs (and xs_relu = relu(xs), the form a ReLU layer's
    consumers see), weight, bias and gout with a share of exact zeros."""

    def __init__(self, geom, seed, acc=0):
        segs, cout, cfg, (n, h, w), _ = geom
        k, transposed = cfg[0], cfg[4]
        self.amps, self.bounds = budget(geom, acc)
        for key, v in self.bounds.items():
            assert v <= LIMIT, (key, v, geom)
        gen = torch.Generator().manual_seed(seed)
        cin = sum(segs)
        self.xs = [_ints((n, c, h, w), a, gen) for c, a in zip(segs, seg_amps(segs, self.amps["x"]))]
        self.xs_relu = [x.clamp_min(0) for x in self.xs]
        self.wt = _ints((cin, cout, k, k) if transposed else (cout, cin, k, k), self.amps["w"], gen, 0.25)
        self.b = _ints((cout,), self.amps["b"], gen, 0.25)
        self.gout = _ints((n, cout) + out_hw_of(geom), self.amps["g"], gen, 0.25)


def seed_of(name):
    return zlib.crc32(str(name).encode()) % 100000


def assert_integral(t, what):
    assert torch.equal(t, t.round()), (what, "reference is not integral")
    m = float(t.abs().max()) if t.numel() else 0.0
    assert m < LIMIT, (what, "reference leaves the exact range", m)


class Reference:
    """fp64 CPU forward and gradients of one geometry (act NONE or ReLU) for inputs xs.  dpre = gout * (pre > 0) for ReLU
    (torch: gradient only where y > 0); relu_in: the inputs are ReLU outputs and their gradients leave masked by (x > 0)."""

    def __init__(self, geom, ops, relu_in):
        segs, cout, cfg, (n, h, w), need_in = geom
        k, stride, pad, opad, transposed, act, alpha, beta, crop = cfg
        assert act in (ACT_NONE, ACT_RELU), act
        xs = [x.double().requires_grad_(ng) for x, ng in zip(ops.xs_relu if relu_in else ops.xs, need_in)]
        wt = ops.wt.double().requires_grad_(True)
        b = ops.b.double().requires_grad_(True)
        xin = torch.cat(xs, 1)
        if transposed:
            pre = F.conv_transpose2d(xin, wt, b, stride=stride, padding=pad, output_padding=opad)
        else:
            pre = F.conv2d(xin, wt, b, stride=stride, padding=pad)
        if crop is not None:
            pre = pre[:, :, :crop[0], :crop[1]]
        self.gout = ops.gout.double()
        self.pre = pre.detach()
        self.out = self.pre.clamp_min(0) if act == ACT_RELU else self.pre
        # what the HIP backward receives: gout (plain form), or gout * (y > 0) from masking consumers (fused ReLU layer)
        self.dpre = self.gout * (self.pre > 0) if act == ACT_RELU else self.gout
        leaves = [x for x in xs if x.requires_grad] + [wt, b]
        grads = list(torch.autograd.grad(pre, leaves, self.dpre))
        self.dw, self.db = grads[-2], grads[-1]
        it = iter(grads[:-2])
        self.dxs = [next(it) if ng else None for ng in need_in]
        if relu_in:
            self.dxs = [None if g is None else g * (x.detach() > 0) for g, x in zip(self.dxs, xs)]
        for what, t in [("pre", self.pre), ("dw", self.dw), ("dbias", self.db)] + \
                [(f"dx{i}", g) for i, g in enumerate(self.dxs) if g is not None]:
            assert_integral(t, what)


def mismatch(got, want):
    """None when got (any float tensor, any device) equals the fp64 reference exactly; else a short description."""
    got = got.detach().double().cpu()
    if got.shape == want.shape and torch.equal(got, want):
        return None
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = (got != want).nonzero()
    first = tuple(int(i) for i in bad[0])
    return (f"{bad.shape[0]} of {want.numel()} differ, max |d| {float((got - want).abs().max()):g}, first at {first}: "
            f"{float(got[first]):g} vs {float(want[first]):g}")


def case_geom(case):
    """tests/test_gpu_conv.py::CASES entry -> (segs, cout, cfg, (N, H, W), need_in) as dvf.conv.GEOM_LOG records it."""
    name, segs, cout, k, stride, pad, opad, transposed, act, nhw, out_hw = case
    alpha, beta = (10.0, 0.01) if "affine" in name else (1.0, 0.0)
    return (tuple(segs), cout, (k, stride, pad, opad, transposed, act, alpha, beta, out_hw), tuple(nhw), (True,) * len(segs))


def fuzz_geom(case):
    """tests/test_gpu_conv_fuzz.py::CASES entry -> geometry: ReLU layers where the envelope fuses the bias column."""
    name, segs, cout, k, stride, pad, opad, transposed, nhw, fused = case
    act = ACT_RELU if fused else ACT_NONE
    return (tuple(segs), cout, (k, stride, pad, opad, transposed, act, 1.0, 0.0, None), tuple(nhw), (True,) * len(segs))


def with_act(geom, act):
    segs, cout, cfg, nhw, need_in = geom
    return (segs, cout, tuple(cfg[:5]) + (act,) + tuple(cfg[6:]), nhw, need_in)
