"""The low-register form of conv_pipe_kernel (csrc/conv_pipe.h: two blocks share a CU): forward and dgrad against torch CPU
fp32 at the suite's 1e-4 (max-abs error / max-abs reference), and the routing of csrc/conv_pipe_host.h read back from the plan
records (dvf.lib.PlanRecord: lr, the form that ran; npi, patch pieces per channel).

Two parts.
 * The product library.  It takes the form only on grids of more than one block per CU, so these cases are the smallest
   maps that get there (a few hundred 128-pixel tiles): 3x3 stride 1, stride 2 in both patch forms (4-byte de-interleaved
   lanes, 16-byte lanes), a 65-channel virtual concatenation (channel-tail zero fill) with ReLU-masked dgrads, a plan whose
   piece count equals the table size and the next one above it, which must stay on the wide-table form.
 * The tuning library (`make TUNING=1`), where DVF_PIPE_LR forces either form onto one plan: the two forms must agree bit
   for bit.  With DVF_PIPE_BIGLDS_KB=76 the small maps below plan inside half a CU's LDS and so reach the form's other edges:
   8x32 N=1 and its split-K (KS > 1), a 4x13 N=4 map (several images folded into one tile), 3x3 stride 2 64->128 at 16x32 in
   both patch forms, piece counts 12 and 13.  That part runs in a child process (the library is chosen when dvf.lib is
   imported); build() of __graft_entry__.py makes the tuning library, and its absence is a failure."""
import json
import os
import subprocess
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

TOL = 1e-4
DEV = "cuda"
LR_NPI = 12                 # PIPE_LR_NPI of csrc/conv_pipe.h
LR_LDS = 80 * 1024          # PIPE_LR_LDS

# name, segs, cout, k, stride, pad, opad, transposed, (N, H, W), masked, expected {op: (lr, npi, x4)} of the pipe records
# (None: not checked).  masked: the inputs carry ReluTags, so every dgrad leaves multiplied by (x > 0).
PRODUCT_CASES = [
    ("c3x3_s1_32_32", [32], 32, 3, 1, 1, 0, False, (1, 96, 416), False, {"fwd": (1, None, 1), "dgrad": (1, None, 1)}),
    ("c3x3_s2_32_32_b4", [32], 32, 3, 2, 1, 0, False, (2, 136, 262), False, {"dgrad": (1, None, 0)}),
    ("c3x3_s2_32_32_b16", [32], 32, 3, 2, 1, 0, False, (2, 136, 264), False, {"dgrad": (1, None, 1)}),
    ("concat65_masked", [32, 32, 1], 32, 3, 1, 1, 0, False, (1, 96, 416), True, {"fwd": (1, None, 1), "dgrad": (1, None, 1)}),
    ("npi_eq_table", [16], 32, 5, 2, 2, 0, False, (2, 200, 418), False, {"fwd": (1, LR_NPI, 0)}),
    ("npi_above_table", [16], 32, 6, 2, 2, 0, False, (2, 200, 418), False, {"fwd": (0, LR_NPI + 2, 0)}),
    # two tiles per wave over four parity classes; its dgrad is a 64-channel plan of 6-wave blocks
    ("t4x4_s2_64_32", [64], 32, 4, 2, 1, 0, True, (3, 64, 208), False, {"fwd": (1, None, None), "dgrad": (1, None, None)}),
]
# the tuning build: (case, DVF_PIPE_X4 or None, expected {op: (lr under DVF_PIPE_LR=1, npi)})
TUNING_CASES = [
    (("c3x3_s1_8x32", [32], 32, 3, 1, 1, 0, False, (1, 8, 32), False, None), None, {"fwd": (1, 1), "dgrad": (1, 1)}),
    (("c3x3_s2_64_128_b16", [64], 128, 3, 2, 1, 0, False, (4, 16, 32), False, None), None, {"fwd": (1, 3), "dgrad": (1, 1)}),
    (("c3x3_s2_64_128_b4", [64], 128, 3, 2, 1, 0, False, (4, 16, 32), False, None), "0", {"fwd": (1, 10), "dgrad": (1, 3)}),
    (("fold4_4x13", [32], 32, 3, 1, 1, 0, False, (4, 4, 13), False, None), None, {"fwd": (1, 5), "dgrad": (1, 5)}),
    (("concat65_masked_8x32", [32, 32, 1], 32, 3, 1, 1, 0, False, (1, 8, 32), True, None), None, {"fwd": (1, 1), "dgrad": (1, 1)}),
    (("npi12", [16], 32, 5, 2, 2, 0, False, (1, 32, 130), False, None), None, {"fwd": (1, LR_NPI)}),
    (("npi13", [16], 32, 6, 2, 2, 0, False, (1, 32, 130), False, None), None, {"fwd": (0, LR_NPI + 1)}),
]


def _rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    den = float(b.abs().max())
    return float((a - b).abs().max()) / (den if den > 0 else 1.0)


def _reference(case):
    """torch CPU: inputs, parameters, output, upstream gradient and the input gradients the library must deliver."""
    name, segs, cout, k, stride, pad, opad, transposed, (n, h, w), masked = case[:10]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 10000)
    cin = sum(segs)
    xs = [torch.randn(n, c, h, w, generator=gen) for c in segs]
    if masked:
        xs = [F.relu(x) for x in xs]                # outputs of ReLU layers
    wt = torch.randn((cin, cout, k, k) if transposed else (cout, cin, k, k), generator=gen) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=gen) * 0.1
    rx = [x.clone().requires_grad_(True) for x in xs]
    xin = torch.cat(rx, 1)
    if transposed:
        pre = F.conv_transpose2d(xin, wt, b, stride=stride, padding=pad, output_padding=opad)
    else:
        pre = F.conv2d(xin, wt, b, stride=stride, padding=pad)
    ref = F.relu(pre)
    # (ReLU kink: an output within rounding of 0 may land on either side in two correct fp32 sums: no gradient there)
    gout = torch.randn(ref.shape, generator=gen) * (pre.detach().abs() > 1e-4)
    (ref * gout).sum().backward()
    dref = [r.grad * (x > 0) if masked else r.grad for r, x in zip(rx, xs)]
    return xs, wt, b, ref.detach(), gout, dref


def _run(case, operands):
    """One forward + backward through the library: output, input gradients, the pipe plan records per op."""
    from dvf import lib as L
    from dvf.conv import ConvFn, ReluTag
    name, segs, cout, k, stride, pad, opad, transposed, (n, h, w), masked = case[:10]
    xs, wt, b, _ref, gout, _dref = operands
    gx = [x.clone().to(DEV).requires_grad_(True) for x in xs]
    if masked:
        for x in gx:
            x._dvf_relu_tag = ReluTag()
    gw, gb = wt.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)
    with L.plan_log() as log:
        out = ConvFn.apply(gw, gb, (k, stride, pad, opad, transposed, 1, 1.0, 0.0, None), *gx)
        out.backward(gout.to(DEV))
        torch.cuda.synchronize()
    plans = {}
    for r in sorted(r for r in log.records if r.kernel == L.K_PIPE):
        plans.setdefault(r.op, []).append({"lr": int(r.lr), "npi": r.npi, "x4": int(r.x4), "ks": r.KS, "bn": r.BN, "lds": r.lds})
    return out.detach(), [x.grad for x in gx], plans


def _check_parity(case, operands, out, grads):
    _xs, _wt, _b, ref, _gout, dref = operands
    errs = {"forward": _rel_err(out, ref)}
    for i, (g, r) in enumerate(zip(grads, dref)):
        errs[f"dgrad seg {i}"] = _rel_err(g, r)
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, (case[0], bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PRODUCT_CASES, ids=[c[0] for c in PRODUCT_CASES])
def test_lr_form_product(case):
    operands = _reference(case)
    out, grads, plans = _run(case, operands)
    _check_parity(case, operands, out, grads)
    for op, (lr, npi, x4) in case[10].items():
        got = plans.get(op)
        assert got, (case[0], op, "no conv_pipe record", plans)
        for p in got:      # (the 1-channel segment of the concatenation is a head kernel's: no record here)
            assert p["lr"] == lr, (case[0], op, "form", p)
            assert npi is None or p["npi"] == npi, (case[0], op, "pieces", p)
            assert x4 is None or p["x4"] == x4, (case[0], op, "lane width", p)
            assert not p["lr"] or (p["npi"] <= LR_NPI and p["lds"] <= LR_LDS), (case[0], op, "outside the form's envelope", p)


def _tuning_lib():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.join(here, "depth-vo-feat_amd", "dvf", "libdvf_hip_tuning.so")


def _tuning_child():
    """(child process, DVF_LIB = the tuning library) every TUNING_CASE with DVF_PIPE_LR = 0 and 1: CPU parity of the forced
    low-register run, bit equality of the two forms, and the form / piece count the records report."""
    from dvf import lib as L
    assert L.lib().dvf_build_has_tuning()
    report = []
    for case, x4, expect in TUNING_CASES:
        if x4 is None:
            os.environ.pop("DVF_PIPE_X4", None)
        else:
            os.environ["DVF_PIPE_X4"] = x4
        operands = _reference(case)
        os.environ["DVF_PIPE_LR"] = "0"
        out0, g0, p0 = _run(case, operands)
        os.environ["DVF_PIPE_LR"] = "1"
        out1, g1, p1 = _run(case, operands)
        _check_parity(case, operands, out1, g1)
        assert all(p["lr"] == 0 for ps in p0.values() for p in ps), (case[0], "DVF_PIPE_LR=0 ran the form", p0)
        for op, (lr, npi) in expect.items():
            assert p1.get(op), (case[0], op, "no conv_pipe record", p1)
            for p in p1[op]:
                assert (p["lr"], p["npi"]) == (lr, npi), (case[0], op, p)
        assert torch.equal(out0, out1), (case[0], "forward differs between the forms")
        for i, (a, c) in enumerate(zip(g0, g1)):
            assert torch.equal(a, c), (case[0], f"dgrad seg {i} differs between the forms")
        report.append({"case": case[0], "plans": p1})
    print(json.dumps(report))


@pytest.mark.gpu
def test_lr_form_bit_equal_to_wide_form_tuning_build():
    lib = _tuning_lib()
    assert os.path.exists(lib), "the tuning library is missing: build() makes it (make -C depth-vo-feat_amd/csrc TUNING=1)"
    env = dict(os.environ, DVF_LIB=lib, DVF_PIPE_BIGLDS_KB="76")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tuning-child"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(report) == len(TUNING_CASES)
    # the edges the cases are there for
    by = {e["case"]: e["plans"] for e in report}
    assert by["c3x3_s1_8x32"]["fwd"][0]["ks"] > 1, "a KS > 1 plan"
    assert by["fold4_4x13"]["fwd"][0]["bn"] == 4, "several images folded into one tile"
    assert by["c3x3_s2_64_128_b16"]["fwd"][0]["x4"] == 1 and by["c3x3_s2_64_128_b4"]["fwd"][0]["x4"] == 0


if __name__ == "__main__" and "--tuning-child" in sys.argv:
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (ROOT, os.path.join(ROOT, "depth-vo-feat_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    _tuning_child()
