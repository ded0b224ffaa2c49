"""Bit-exact parity of every convolution plan with integer-valued operands (method and budget: tests/conv_exact.py).

The fp32 parity tests (test_gpu_conv.py, test_gpu_conv_fuzz.py, test_gpu_bench_shapes.py) bound max|a - b| / max|ref|,
which cannot see a structural error that is small next to the largest element: one pixel dropped from a 5M-term weight
gradient, a border row of one transposed parity class, the last partial K-chunk of a split-K.  Here every operand is a small
integer and every reduction stays inside fp32's exact integer range, so forward, every input gradient, the weight and the
bias gradient must EQUAL an fp64 CPU reference -- in every reduction order the kernels use.  Each geometry runs in four
forms: plain and fused (inputs tagged as ReLU outputs: masked dgrad; a ReLU layer's own bias gradient on the weight-gradient
GEMM), each with default and with deterministic (ordered) reductions.  ReLU kinks are not masked: the gate at exactly zero
is part of what is compared.  The sigmoid-affine epilogue is the one inexact step: those layers run exactly with act = NONE,
and their sigmoid forward is bounded per element in ulp.

Geometries: every CASES entry of test_gpu_conv.py, the 48 of test_gpu_conv_fuzz.py, EXTRA_CASES below and every distinct
geometry of the cfg 2-5 bench steps.  The plan records (dvf_conv2d_last_plans) of all exact runs must contain every plan
of those steps and every kernel family."""
import contextlib
import ctypes

import pytest
import torch

import conv_exact as X
import test_gpu_bench_shapes as BS
import test_gpu_conv as TC
import test_gpu_conv_fuzz as TF

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = {"plans": set(), "done": set()}

EXTRA_CASES = [
    # name, geometry (segs, cout, cfg (k, stride, pad, opad, transposed, act, alpha, beta, out_hw), (N, H, W), need_in)
    # two equal-width segments (a swap of their weight-channel offsets reads in bounds), 3 segments on conv_pipe
    ("concat_equal_widths", ((32, 32), 32, (3, 1, 1, 0, False, 1, 1.0, 0.0, None), (2, 24, 40), (True, True))),
    ("concat3_equal_widths", ((16, 16, 16), 64, (3, 1, 1, 0, False, 1, 1.0, 0.0, None), (2, 20, 36), (True, True, True))),
    # padding 5 > 4: wgrad_pipe refuses it, the register-staged conv_wgrad_kernel (DVF_K_WGRAD) takes the weight gradient --
    # no product geometry reaches that kernel
    ("k7_pad5_conv_wgrad", ((8,), 16, (7, 1, 5, 0, False, 1, 1.0, 0.0, None), (2, 12, 20), (True,))),
]


@contextlib.contextmanager
def plan_capture(into):
    """dvf.lib.plan_log(into); a call that reports DVF_PLAN_MAX records may have run a further plan that the log dropped: that
    fails the test."""
    from dvf import lib as L
    with L.plan_log(into) as cap:
        yield cap
    assert not cap.full_calls, ("a call filled the plan log (8 records): a ninth plan may have run unseen", cap.full_calls)


def _to_dev(x, offset):
    if offset:     # a contiguous view at a one-float storage offset: the 16-byte-lane plans are refused at run time
        return torch.empty(x.numel() + 1, device=DEV)[1:].view(x.shape).copy_(x)
    return x.to(DEV)


def _run(geom, ops, fused, offset=False):
    """One HIP forward + backward of the geometry; returns (out, [dx], dw, dbias) on the host."""
    from dvf.conv import ConvFn, ReluTag
    segs, cout, cfg, nhw, need_in = geom
    act = cfg[5]
    xs = ops.xs_relu if fused else ops.xs
    gx = [_to_dev(x, offset).requires_grad_(ng) for x, ng in zip(xs, need_in)]
    if fused:
        for x in gx:
            x._dvf_relu_tag = ReluTag()
    gw, gb = ops.wt.to(DEV).requires_grad_(True), ops.b.to(DEV).requires_grad_(True)
    own_tag = fused and act == X.ACT_RELU
    out = ConvFn.apply(gw, gb, tuple(cfg) + ((ReluTag(),) if own_tag else ()), *gx)
    # a fused ReLU layer receives what its masking consumers deliver: gout * (y > 0)
    go = ops.gout.to(DEV)
    out.backward(go * (out.detach() > 0) if own_tag else go)
    return out.cpu(), [x.grad.cpu() if x.grad is not None else None for x in gx], gw.grad.cpu(), gb.grad.cpu()


def _compare(tag, got, ref, failures):
    out, dxs, dw, db = got
    checks = [("fwd", out, ref.out), ("dw", dw, ref.dw), ("dbias", db, ref.db)]
    checks += [(f"dx{i}", g, r) for i, (g, r) in enumerate(zip(dxs, ref.dxs)) if r is not None]
    for what, g, r in checks:
        if g is None:
            failures.append((tag, what, "no gradient"))
            continue
        m = X.mismatch(g, r)
        if m:
            failures.append((tag, what, m))


def check_geometry(name, geom, seed, offset=False, forms=(False, True)):
    """All four forms of one geometry against fp64, exactly.  A sigmoid-affine layer runs them with act = NONE; its sigmoid
    run must take the same plans, and its forward is bounded per element (_check_sigmoid).  forms: (False,) or (True,) runs
    the plain or the fused pair alone, for a caller that spreads a large geometry's two fp64 references over two cases."""
    from dvf import conv as C
    failures = []
    sig = geom[2][5] == X.ACT_SIGMOID_AFFINE
    exact_geom = X.with_act(geom, X.ACT_NONE) if sig else geom
    ops = X.Operands(exact_geom, seed)
    for fused in forms:
        ref = X.Reference(exact_geom, ops, relu_in=fused)
        for det in (False, True):
            for off in ((False, True) if offset and not fused else (False,)):
                tag = f"{name} {'fused' if fused else 'plain'}{' det' if det else ''}{' offset' if off else ''}"
                plans = set()
                C.set_deterministic(det)
                try:
                    with plan_capture(plans):
                        got = _run(exact_geom, ops, fused, off)
                finally:
                    C.set_deterministic(False)
                _compare(tag, got, ref, failures)
                STATE["plans"] |= plans
                if sig and not fused and not det and not off:
                    failures += _check_sigmoid(name, geom, ops, ref, plans)
        del ref
    assert not failures, failures


# Sigmoid-affine epilogue, out = alpha * (1 / (1 + expf(-pre))) + beta in fp32 (conv_pipe.h, conv_head.hip), with pre exact.
# Relative errors, u = 2^-23: expf <= 1 ulp (HIP device math: u); 1 + e rounds (u/2) and carries e's error scaled by
# e / (1 + e) < 1: <= 1.5u; the correctly rounded division adds u/2: 2u on s; alpha * s adds u/2: 2.5u; adding beta >= 0
# (alpha > 0, so alpha * s <= out) adds u/2 of out: |out - exact| <= 3u |out|.  One ulp of out is >= |out| u / 2, so
# the bound is 6 ulp of the fp32 output; + 2^-126 where a subnormal result may be flushed to zero.
SIGMOID_ULP = 6


def _check_sigmoid(name, geom, ops, ref, none_plans):
    from dvf.conv import ConvFn
    segs, cout, cfg, nhw, need_in = geom
    alpha, beta = cfg[6], cfg[7]
    plans = set()
    gx = [x.to(DEV).requires_grad_(ng) for x, ng in zip(ops.xs, need_in)]
    gw, gb = ops.wt.to(DEV).requires_grad_(True), ops.b.to(DEV).requires_grad_(True)
    with plan_capture(plans):
        out = ConvFn.apply(gw, gb, tuple(cfg), *gx)
        out.backward(ops.gout.to(DEV))
    STATE["plans"] |= plans
    failures = []
    if plans != none_plans:
        failures.append((name, "sigmoid run plans differ from the act=NONE run", sorted(plans ^ none_plans)))
    # alpha / beta as the descriptor holds them (fp32)
    a64 = float(torch.tensor(alpha, dtype=torch.float32))
    b64 = float(torch.tensor(beta, dtype=torch.float32))
    want = a64 * torch.sigmoid(ref.pre) + b64
    got = out.detach().double().cpu()
    w32 = want.float().abs()
    ulp = (torch.nextafter(w32, torch.tensor(float("inf"))) - w32).double()
    err = (got - want).abs()
    bad = err > SIGMOID_ULP * ulp + 2.0 ** -126
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        failures.append((name, "sigmoid fwd", int(bad.sum()), float((err / ulp).max()), i, float(got[i]), float(want[i])))
    normal = want.abs() >= 2.0 ** -126
    print("%s: sigmoid forward within %.2f ulp (normal outputs)" % (name, float((err / ulp)[normal].max()) if normal.any() else 0.0))
    return failures


@pytest.mark.parametrize("case", TC.CASES, ids=[c[0] for c in TC.CASES])
def test_conv_cases_exact(case):
    check_geometry(case[0], X.case_geom(case), X.seed_of(case[0]), offset="offset" in case[0])


@pytest.mark.parametrize("case", TF.CASES, ids=[c[0] for c in TF.CASES])
def test_fuzz_cases_exact(case):
    check_geometry(case[0], X.fuzz_geom(case), X.seed_of(case[0]))


@pytest.mark.parametrize("name,geom", EXTRA_CASES, ids=[c[0] for c in EXTRA_CASES])
def test_extra_cases_exact(name, geom):
    check_geometry(name, geom, X.seed_of(name))


def _bench_step(config):
    """Distinct convolution geometries and the plan records of one cfg step (default and deterministic passes)."""
    import argparse
    from dvf import conv as C
    from dvf import lib as L
    key = ("bench", config)
    if key in STATE:
        return STATE[key]
    bench = BS._bench_module()
    cfg = bench.CONFIGS[config]
    args = argparse.Namespace(batch=cfg["batch"], height=cfg["height"], width=cfg["width"], seed=0, force_ddp=False,
                              no_graph=True)
    step, fwd_bwd, opt, _, nets = bench.build(args, cfg, torch.device(DEV), 1, 0)
    plans, geoms = set(), []
    try:
        for det in (False, True):
            C.set_deterministic(det)
            fwd_bwd()                                 # (first pass of a mode: packs, workspaces)
            with C.geom_log(geoms), plan_capture(plans):
                fwd_bwd()
                L.join_aux_streams()
                torch.cuda.synchronize()
    finally:
        C.set_deterministic(False)
    del step, fwd_bwd, opt, nets
    torch.cuda.empty_cache()
    STATE[key] = (BS._distinct(geoms), plans)
    return STATE[key]


@pytest.mark.parametrize("config", [2, 3, 4, 5])
def test_bench_geometries_exact(config):
    """Every distinct convolution geometry of a bench step, exactly, in all four forms; then the step's plans (default and
    deterministic) must all have run in an exact case."""
    geoms, step_plans = _bench_step(config)
    assert geoms and step_plans
    failures = []
    for gi, geom in enumerate(geoms):
        if geom in STATE["done"]:
            continue
        try:
            check_geometry(f"cfg{config} #{gi} {geom}", geom, 1000 * config + gi)
        except AssertionError as e:
            failures.append(str(e)[:2000])
        STATE["done"].add(geom)
        torch.cuda.empty_cache()
    assert not failures, failures
    missing = sorted(step_plans - STATE["plans"])
    assert not missing, (config, "step plans no exact case ran", missing)
    print("cfg %d: %d geometries exact, %d step plans all covered" % (config, len(geoms), len(step_plans)))


def _wgrad_call(geom, ops, dw, db, ws):
    from dvf import lib as L
    from dvf.conv import _Geo
    segs, cout, cfg, nhw, need_in = geom
    g = _Geo(ops.wt, cfg, ops.xs)
    xs = [x.to(DEV) for x in ops.xs]
    inarr = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    dpre = ops.gout.to(DEV)
    L.check(L.lib().dvf_conv2d_wgrad(g.dref, inarr, g.segarr, g.nseg, dpre.data_ptr(), dw.data_ptr(), 1, db.data_ptr(), 1,
                                     ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                     L.stream_raw()), "dvf_conv2d_wgrad")
    torch.cuda.synchronize()
    return g


ACC_AMP = 50     # amplitude of the initial gradient arena contents


@pytest.mark.parametrize("case", TC.CASES + TF.CASES, ids=[c[0] for c in TC.CASES + TF.CASES])
def test_wgrad_accumulates_exactly(case):
    """dvf_conv2d_wgrad(accumulate=1, accumulate_dbias=1) into a non-zero integer dw / dbias -- FlatAdam's arena -- with and
    without the deterministic scratch: initial + reference, exactly."""
    from dvf import lib as L
    geom = X.case_geom(case) if len(case) == 11 else X.fuzz_geom(case)
    geom = X.with_act(geom, X.ACT_NONE)
    ops = X.Operands(geom, X.seed_of(case[0]) + 1, acc=ACC_AMP)
    ref = X.Reference(geom, ops, relu_in=False)
    gen = torch.Generator().manual_seed(X.seed_of(case[0]) + 2)
    dw0 = X._ints(ops.wt.shape, ACC_AMP, gen)
    db0 = X._ints(ops.b.shape, ACC_AMP, gen)
    failures = []
    for det in (False, True):
        dw, db = dw0.to(DEV), db0.to(DEV)
        ws = None
        if det:
            from dvf.conv import _Geo
            g = _Geo(ops.wt, geom[2], ops.xs)
            n = int(L.lib().dvf_conv2d_wgrad_ws_floats(g.dref, g.segarr, g.nseg))
            ws = torch.empty(max(n, 1), device=DEV) if n > 0 else None
        plans = set()
        with plan_capture(plans):
            _wgrad_call(geom, ops, dw, db, ws)
            L.note_plans("wgrad")
        STATE["plans"] |= plans
        for what, g, r in (("dw", dw, dw0.double() + ref.dw), ("dbias", db, db0.double() + ref.db)):
            m = X.mismatch(g, r)
            if m:
                failures.append((case[0], "det" if det else "default", what, m))
    assert not failures, failures


def _bench_planes():
    planes = set()
    for config in (2, 3, 4, 5):
        for segs, cout, cfg, (n, h, w), need_in in _bench_step(config)[0]:
            oh, ow = X.out_hw_of((segs, cout, cfg, (n, h, w), need_in))
            planes.add((n, cout, oh * ow))
    return sorted(planes)


def test_act_bwd_accumulates_exactly():
    """dvf_act_bwd(accumulate_dbias=1) at every (N, C, HW) plane of the bench steps, ReLU and NONE, with and without the
    ordered scratch: dpre = dy * (y > 0) (ReLU: y has exact zeros) and dbias = initial + channel sums, exactly."""
    from dvf import lib as L
    lib = L.lib()
    failures = []
    for pi, (n, c, hw) in enumerate(_bench_planes()):
        gen = torch.Generator().manual_seed(777 + pi)
        amp = max(1, min(3, (X.LIMIT - ACC_AMP) // (n * hw)))
        assert n * hw * amp + ACC_AMP <= X.LIMIT, (n, c, hw)
        dy = X._ints((n, c, hw), amp, gen, 0.25)
        y = X._ints((n, c, hw), 2, gen).clamp_min(0)         # a ReLU output: exact zeros
        db0 = X._ints((c,), ACC_AMP, gen)
        for act in (L.ACT_RELU, L.ACT_NONE):
            dpre_ref = dy.double() * (y > 0) if act == L.ACT_RELU else dy.double()
            db_ref = db0.double() + dpre_ref.sum((0, 2))
            for det in (False, True):
                gdy, gy = dy.to(DEV), y.to(DEV)
                dpre = torch.full_like(gdy, float("nan"))
                db = db0.to(DEV)
                ws = torch.empty(max(int(lib.dvf_act_bwd_ws_floats(n, c, hw)), 1), device=DEV) if det else None
                L.check(lib.dvf_act_bwd(gdy.data_ptr(), gy.data_ptr() if act == L.ACT_RELU else None,
                                        dpre.data_ptr() if act == L.ACT_RELU else None, db.data_ptr(), n, c, hw, act,
                                        1.0, 0.0, 1, ws.data_ptr() if ws is not None else None,
                                        ws.numel() if ws is not None else 0, L.stream_raw()), "dvf_act_bwd")
                torch.cuda.synchronize()
                tag = ((n, c, hw), "relu" if act == L.ACT_RELU else "none", "det" if det else "default")
                checks = [("dbias", db, db_ref)] + ([("dpre", dpre, dpre_ref)] if act == L.ACT_RELU else [])
                for what, g, r in checks:
                    m = X.mismatch(g, r)
                    if m:
                        failures.append(tag + (what, m))
    assert not failures, failures


# Kernel families (dvf.lib.KERNELS) that no exact case reaches, with the reason.  Empty: every family ran.
UNREACHED_FAMILIES = {}


def test_plan_family_coverage():
    """Runs after the cases above: every kernel family 1-9 appeared in an exact run (or is named in UNREACHED_FAMILIES)."""
    if not STATE["plans"]:
        pytest.fail("no exact case ran before this test (run the whole module)")
    from dvf.lib import KERNELS
    seen = {}
    for rec in STATE["plans"]:
        seen.setdefault(rec.kernel, set()).add(rec.op)
    print("exact plan coverage: %d records; " % len(STATE["plans"]) +
          ", ".join("%d %s %s" % (f, KERNELS[f], sorted(seen.get(f, ())) or "-") for f in sorted(KERNELS)))
    missing = sorted(set(KERNELS) - set(seen) - set(UNREACHED_FAMILIES))
    assert not missing, ("kernel families no exact case reached", [KERNELS[f] for f in missing])
    stale = sorted(set(UNREACHED_FAMILIES) & set(seen))
    assert not stale, ("reached now: remove from UNREACHED_FAMILIES", stale)
