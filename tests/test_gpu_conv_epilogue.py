"""Every cell of the convolution kernels' shared tile epilogue (csrc/conv_epilogue.h: store_tile) and split-K finisher
(csrc/conv_pipe_host.h: finish_output), and every FMA site of the head kernel, on the smallest geometries that reach them.

test_gpu_conv_exact.py requires every plan to equal an fp64 reference on integer operands, but cannot say which cells of
the epilogue / finisher matrix its geometries exercised.  Here each run's plan records (dvf_conv2d_last_plans) and geometry
are turned into the cells it hit, and the last test asserts that the union equals REQUIRED: a cell silently routed to another
kernel or another output mode fails.  Every result must equal the fp64 reference exactly (float atomics are exact on these
operands in any order); the sigmoid-affine forward is bounded to 6 ulp next to its exact act = NONE twin, as in
check_geometry.

Routes: ConvFn (always supplies a workspace: fused and workspace modes) through check_geometry -- plain and masked dgrad,
default and deterministic; and the C ABI called directly with ws = NULL (atomics into a zeroed output) or packed = NULL
(the gather kernel on 32 / 64 output channels: the only way to "every row of a wave exists" in that kernel)."""
import ctypes

import pytest
import torch

import conv_exact as X
import test_gpu_conv_exact as TE

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIT = set()
NONE, RELU, SIG = X.ACT_NONE, X.ACT_RELU, X.ACT_SIGMOID_AFFINE
ACT_NAME = {NONE: "none", RELU: "relu", SIG: "sigmoid"}


def geom(segs, cout, nhw, act=RELU, k=3, stride=1, pad=1, opad=0, transposed=False):
    alpha, beta = (10.0, 0.01) if act == SIG else (1.0, 0.0)
    return (tuple(segs), cout, (k, stride, pad, opad, transposed, act, alpha, beta, None), tuple(nhw), (True,) * len(segs))


HEAD_COUT, HEAD_CIN = (1, 2, 3, 4), (4, 6, 37)
REQUIRED = (
    # output mode x family (pipelined: workspace mode with KS < 8 and KS >= 8 -- the two reduce kernels)
    {("mode", "pipe", m) for m in ("fused", "ws_lt8", "ws_ge8", "atomic")} |
    {("mode", "gather", m) for m in ("fused", "ws", "atomic")} |
    # every channel row of a wave exists / does not
    {("rows", f, r) for f in ("pipe", "gather") for r in ("full", "ragged")} |
    # fused bias + activation
    {("act", f, a) for f in ("pipe", "gather") for a in ("none", "relu", "sigmoid")} |
    # dgrad with and without the ReLU mask of the producing layer, in every output mode
    {("mask", f, m, w) for f in ("pipe", "gather") for m in ("fused", "ws", "atomic") for w in ("masked", "plain")} |
    # batch folded into the tile with N not a multiple of BN; one image per block with N = 2
    {("batch", "pipe", "folded_ragged"), ("batch", "gather", "n2")} |
    # non-zero class offsets in the store: dgrad of a stride-2 Conv2d, forward of a ConvTranspose2d
    {("classes", "stride2"), ("classes", "transposed")} |
    # head kernel: four-in-flight loop, tail, chunk boundary; 16-channel variant; both tiles; narrow-segment dgrad
    {("head", co, ci) for co in HEAD_COUT for ci in HEAD_CIN} |
    {("head16", (16, 1)), ("head_tile", "32x4"), ("head_tile", "8x8"), ("seg_dgrad", "masked"), ("seg_dgrad", "plain")})


def cells_of(g, recs, masked):
    """Cells hit by the plan records `recs` (dvf.lib.PlanRecord) of runs of geometry g; masked: the forms of its dgrad
    that ran ({"masked", "plain"} for check_geometry)."""
    from dvf.lib import K_PIPE, K_GATHER, K_HEAD_FWD, K_HEAD_SEG_DGRAD
    segs, cout, cfg, (n, h, w), _ = g
    stride, transposed, act = cfg[1], cfg[4], cfg[5]
    acts = {ACT_NAME[act]} | ({"none"} if act == SIG else set())        # (a sigmoid layer also ran as its exact twin)
    out = set()
    for rec in recs:
        op, kern = rec.op, rec.kernel
        if kern in (K_PIPE, K_GATHER) and op in ("fwd", "dgrad"):
            fam = "pipe" if kern == K_PIPE else "gather"
            mt, ks, bn, mode, ncls = rec.MT, rec.KS, rec.BN, rec.out_mode, rec.ncls
            out.add(("mode", fam, mode + (("_ge8" if ks >= 8 else "_lt8") if (fam == "pipe" and mode == "ws") else "")))
            m = cout if op == "fwd" else (segs[0] if len(segs) == 1 else None)      # (several segments: the record does not say whose)
            if m is not None:
                out.add(("rows", fam, "full" if m % (32 * mt) == 0 else "ragged"))
            if op == "fwd" and mode == "fused":
                out |= {("act", fam, a) for a in acts}
            if op == "dgrad":
                out |= {("mask", fam, mode, form) for form in masked}
            if fam == "pipe" and bn > 1 and n % bn != 0:
                out.add(("batch", "pipe", "folded_ragged"))
            if fam == "gather" and n == 2:
                out.add(("batch", "gather", "n2"))
            if ncls > 1 and stride == 2:
                if transposed and op == "fwd":
                    out.add(("classes", "transposed"))
                if not transposed and op == "dgrad":
                    out.add(("classes", "stride2"))
        if (kern, op) in ((K_HEAD_FWD, "fwd"), (K_HEAD_SEG_DGRAD, "dgrad")):
            mo, c = (cout, sum(segs)) if kern == K_HEAD_FWD else (rec.segc, cout)
            lowres = n * h * w <= 4 * 64 * 208 and mo <= 4 and c >= 32          # head_fwd_launch (csrc/conv_head.hip)
            out.add(("head_tile", "32x4" if lowres else "8x8"))
            if kern == K_HEAD_SEG_DGRAD:
                out |= {("seg_dgrad", form) for form in masked}
            elif mo == 16:
                out.add(("head16", tuple(segs)))
            else:
                out.add(("head", mo, c))
    return out


def run_exact(name, g):
    """check_geometry (all four forms against fp64, exactly) with this geometry's plan records to itself."""
    saved, TE.STATE["plans"] = TE.STATE["plans"], set()
    try:
        TE.check_geometry(name, g, X.seed_of(name))
        recs = TE.STATE["plans"]
    finally:
        TE.STATE["plans"] = saved | TE.STATE["plans"]
    hit = cells_of(g, recs, {"masked", "plain"})
    print(name, sorted(recs), sorted(hit, key=str))
    HIT.update(hit)
    return hit


# ---- ConvFn route: fused and workspace modes
MFMA_CASES = [
    # pipelined forward, fused (one reduction chunk): the three activations; rows full (32 = 32 * MT).  Its dgrad (16
    # channels) is the gather kernel's, split-K through the workspace.
    ("pipe_fused_none", geom((16,), 32, (2, 8, 26), NONE)),
    ("pipe_fused_relu", geom((16,), 32, (2, 8, 26), RELU)),
    ("pipe_fused_sigmoid", geom((16,), 32, (2, 8, 26), SIG)),
    ("pipe_ragged_48", geom((16,), 48, (2, 8, 26), NONE)),          # MT = 2, 48 of 64 rows
    ("pipe_ws_ks2", geom((32,), 32, (1, 8, 26))),                   # forward and dgrad: split-K, KS = 2
    ("pipe_ws_ks8", geom((64,), 64, (2, 4, 13))),                   # forward and dgrad: KS = 8, the k-parallel reduce
    ("pipe_dgrad_fused", geom((32,), 16, (2, 8, 26))),              # dgrad: one chunk, mask in the epilogue; forward: gather, split-K
    ("pipe_batch_folded", geom((64,), 64, (3, 2, 7))),              # 2x7 maps: BN = 4 images per tile, N = 3
    ("pipe_stride2", geom((16,), 32, (2, 9, 27), stride=2)),        # dgrad: four output-parity classes
    ("pipe_transposed", geom((32,), 32, (2, 4, 13), stride=2, opad=1, transposed=True)),    # forward: four classes
    ("gather_fused_none", geom((8,), 8, (2, 8, 26), NONE)),         # forward and dgrad fused, 8 of 32 rows
    ("gather_fused_relu", geom((8,), 8, (2, 8, 26), RELU)),
    ("gather_fused_sigmoid", geom((8,), 8, (2, 8, 26), SIG)),
    ("gather_fwd_ws", geom((32,), 8, (2, 8, 26))),                  # forward: split-K, KS = 2
    ("gather_dgrad_ws", geom((8,), 32, (2, 8, 26))),                # dgrad: split-K, KS = 2
]


@pytest.mark.parametrize("name,g", MFMA_CASES, ids=[c[0] for c in MFMA_CASES])
def test_mfma_epilogue_cells(name, g):
    run_exact(name, g)


# ---- head kernels: 3x3, stride 1, pad 1; H, W no multiples of the 64 x 4 / 64 x 8 tile
HEAD_ACT = {1: SIG, 2: SIG, 3: NONE, 4: RELU}
HEAD_CASES = [("head_%d_%d" % (co, ci), geom((ci,), co, (2, 9, 67) if ci >= 32 else (1, 11, 70), HEAD_ACT[co]))
              for co in HEAD_COUT for ci in HEAD_CIN]
HEAD_CASES += [
    ("head16_concat", geom((16, 1), 16, (1, 65, 66))),          # 16-channel variant; dgrad: wide and narrow segments, 8x8 tile
    ("seg_dgrad_lowres", geom((8, 2), 32, (2, 8, 26))),         # dgrad of the 2-channel segment over 32 channels: 32x4 tile
]


@pytest.mark.parametrize("name,g", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_head_kernel_cells(name, g):
    run_exact(name, g)


# ---- C ABI route: ws = NULL (atomics), packed = NULL (gather kernel whatever the channel count)
def _records(L, op, into):
    recs, full = L.last_plans(op)
    assert not full, "the plan log is full: a further plan may have run unseen"
    into |= set(recs)


def run_abi(name, g, use_packed, use_ws):
    """dvf_conv2d_fwd and dvf_conv2d_dgrad (plain and masked) called directly into NaN-filled outputs, against fp64."""
    from dvf import conv as C
    from dvf import lib as L
    lib = L.lib()
    segs, cout, cfg, nhw, need_in = g
    ops = X.Operands(g, X.seed_of(name))
    failures, hit = [], set()
    w, b = ops.wt.to(DEV), ops.b.to(DEV)
    for masked in (False, True):
        ref = X.Reference(g, ops, relu_in=masked)
        xs = [x.to(DEV) for x in (ops.xs_relu if masked else ops.xs)]
        geo = C._Geo(w, cfg, xs)

        def operands(kind):
            packed, ws = C._packed_weights(w, w, geo.desc, geo.segc, kind, geo.pkey, geo.segarr)
            ws = ws if use_ws else None
            return (packed.data_ptr() if (use_packed and packed is not None) else None,
                    ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0)

        recs = set()
        out = torch.full((nhw[0], cout, geo.oh, geo.ow), float("nan"), device=DEV)
        inarr = (ctypes.c_void_p * geo.nseg)(*[x.data_ptr() for x in xs])
        pk, wsp, wsn = operands(0)
        L.check(lib.dvf_conv2d_fwd(geo.dref, inarr, geo.segarr, geo.nseg, pk, w.data_ptr(), b.data_ptr(), out.data_ptr(),
                                   wsp, wsn, L.stream_raw()), "dvf_conv2d_fwd")
        _records(L, "fwd", recs)
        dpre = ref.dpre.float().to(DEV)
        gins = [torch.full_like(x, float("nan")) for x in xs]
        ginarr = (ctypes.c_void_p * geo.nseg)(*[t.data_ptr() for t in gins])
        marr = (ctypes.c_void_p * geo.nseg)(*[x.data_ptr() for x in xs]) if masked else None
        pk, wsp, wsn = operands(1)
        L.check(lib.dvf_conv2d_dgrad(geo.dref, dpre.data_ptr(), pk, w.data_ptr(), ginarr, geo.segarr, geo.nseg, wsp, wsn,
                                     marr, L.stream_raw()), "dvf_conv2d_dgrad")
        _records(L, "dgrad", recs)
        torch.cuda.synchronize()
        form = "masked" if masked else "plain"
        for what, got, want in [("fwd", out, ref.out)] + [(f"dx{i}", t, r) for i, (t, r) in enumerate(zip(gins, ref.dxs))]:
            m = X.mismatch(got, want)
            if m:
                failures.append((name, form, what, m))
        hit |= cells_of(g, recs, {form})
        print(name, form, sorted(recs))
    assert not failures, failures
    print(name, sorted(hit, key=str))
    HIT.update(hit)
    return hit


ABI_CASES = [
    # name, geometry, packed, ws
    ("pipe_atomic", geom((32,), 32, (1, 8, 26)), True, False),          # forward and dgrad: KS = 2 without a workspace
    ("gather_fwd_atomic", geom((32,), 8, (2, 8, 26)), True, False),
    ("gather_dgrad_atomic", geom((8,), 32, (2, 8, 26)), True, False),
    ("gather_full_32", geom((16,), 32, (2, 8, 26)), False, True),       # MT = 1: 32 of 32 rows
    ("gather_full_64", geom((16,), 64, (2, 8, 26), NONE), False, True),     # MT = 2: 64 of 64 rows
]


@pytest.mark.parametrize("name,g,use_packed,use_ws", ABI_CASES, ids=[c[0] for c in ABI_CASES])
def test_abi_epilogue_cells(name, g, use_packed, use_ws):
    hit = run_abi(name, g, use_packed, use_ws)
    if not use_packed:
        assert not [c for c in hit if c[1] == "pipe"], ("packed = NULL ran the pipelined kernel", hit)


def test_matrix_covered():
    """Runs after the cases above: the cells they hit are exactly the required matrix."""
    if not HIT:
        pytest.fail("no case ran before this test (run the whole module)")
    missing, extra = sorted(REQUIRED - HIT, key=str), sorted(HIT - REQUIRED, key=str)
    assert not missing and not extra, ("cells not reached", missing, "cells outside the matrix", extra)
