"""Per-layer micro-benchmark of the convolution kernels (GPU box).  usage: conv_bench.py [filter] ; env DVF_DBG for
ablations (1: no patch staging, 2: no weight staging, 4: no MFMA loop).

CB_FORMS=0,1 (tuning build, DVF_LIB=.../libdvf_hip_tuning.so): A/B of the two forms of conv_pipe_kernel instead of the plain
table.  The listed DVF_PIPE_LR values (0: wide piece tables everywhere, 1: the low-register form wherever the plan fits it)
alternate CB_ROUNDS times (default 5) per layer in one process, CB_ITERS forward + backward passes each; per value: median /
min / max over the rounds of the mean event time of a forward and of a dgrad call, whether outputs and input gradients of
all values are bit-equal, and the conv_pipe plan records (op, (MT, NT, WM, CK, TBU), threads, LDS bytes, form bit)."""
import os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-vo-feat_amd"))
from dvf.conv import ConvFn
from dvf import lib as L
LAYERS = [  # name, cin segs, cout, k, s, p, op, transposed, act, (N,H,W), out_hw
    ("conv1.2 7x7s1 32->32 @128x416", [32], 32, 7, 1, 3, 0, False, 1, (4, 128, 416), None),
    ("conv2.0 5x5s2 32->64", [32], 64, 5, 2, 2, 0, False, 1, (4, 128, 416), None),
    ("conv2.2 5x5s1 64->64 @64x208", [64], 64, 5, 1, 2, 0, False, 1, (4, 64, 208), None),
    ("conv3.0 3x3s2 64->128", [64], 128, 3, 2, 1, 0, False, 1, (4, 64, 208), None),
    ("conv3.2 3x3s1 128->128 @32x104", [128], 128, 3, 1, 1, 0, False, 1, (4, 32, 104), None),
    ("conv4.2 3x3s1 256->256 @16x52", [256], 256, 3, 1, 1, 0, False, 1, (4, 16, 52), None),
    ("conv5.2 3x3s1 512->512 @8x26", [512], 512, 3, 1, 1, 0, False, 1, (4, 8, 26), None),
    ("conv6.2 3x3s1 512->512 @4x13", [512], 512, 3, 1, 1, 0, False, 1, (4, 4, 13), None),
    ("iconv4 3x3s1 256->128 @32x104", [128, 128], 128, 3, 1, 1, 0, False, 1, (4, 32, 104), None),
    ("iconv2 3x3s1 65->32 @128x416", [32, 32, 1], 32, 3, 1, 1, 0, False, 1, (4, 128, 416), None),
    ("iconv1 3x3s1 17->16 @256x832", [16, 1], 16, 3, 1, 1, 0, False, 1, (4, 256, 832), None),
    ("disp1 3x3s1 16->1 @256x832", [16], 1, 3, 1, 1, 0, False, 2, (4, 256, 832), None),
    ("disp2 3x3s1 32->1 @128x416", [32], 1, 3, 1, 1, 0, False, 2, (4, 128, 416), None),
    ("disp3 3x3s1 64->1 @64x208", [64], 1, 3, 1, 1, 0, False, 2, (4, 64, 208), None),
    ("disp4 3x3s1 128->1 @32x104", [128], 1, 3, 1, 1, 0, False, 2, (4, 32, 104), None),
    ("upconv4 T3x3s2 256->128 ->32x104", [256], 128, 3, 2, 1, 1, True, 1, (4, 16, 52), None),
    ("upconv2 T3x3s2 64->32 ->128x416", [64], 32, 3, 2, 1, 1, True, 1, (4, 64, 208), None),
    ("upconv1 T3x3s2 32->16 ->256x832", [32], 16, 3, 2, 1, 1, True, 1, (4, 128, 416), None),
    ("pose up T4x4s2 128->64 ->64x208", [128], 64, 4, 2, 1, 0, True, 1, (4, 32, 104), None),
    ("iconv7 3x3s1 1024->512 @4x13", [512, 512], 512, 3, 1, 1, 0, False, 1, (4, 4, 13), None),
    ("iconv6 3x3s1 1024->512 @8x26", [512, 512], 512, 3, 1, 1, 0, False, 1, (4, 8, 26), None),
    ("iconv5 3x3s1 512->256 @16x52", [256, 256], 256, 3, 1, 1, 0, False, 1, (4, 16, 52), None),
    ("iconv3 3x3s1 129->64 @64x208", [64, 64, 1], 64, 3, 1, 1, 0, False, 1, (4, 64, 208), None),
    ("conv7.2 3x3s1 512->512 @2x7", [512], 512, 3, 1, 1, 0, False, 1, (4, 2, 7), None),
    # further layers with a launch on a grid of more than 256 blocks (the two forms of conv_pipe_kernel)
    ("conv1.0 7x7s2 3->32 @256x832", [3], 32, 7, 2, 3, 0, False, 1, (4, 256, 832), None),
    ("upconv3 T3x3s2 128->64 ->64x208", [128], 64, 3, 2, 1, 1, True, 1, (4, 32, 104), None),
    ("pose up T4x4s2 64->32 ->128x416", [64], 32, 4, 2, 1, 0, True, 1, (4, 64, 208), None),
    ("pose conv2 5x5s2 16->32 @128x416", [16], 32, 5, 2, 2, 0, False, 1, (4, 128, 416), None),
    ("pose conv3 3x3s2 32->64 @64x208", [32], 64, 3, 2, 1, 0, False, 1, (4, 64, 208), None),
]
flt = sys.argv[1] if len(sys.argv) > 1 else ""
iters = int(os.environ.get("CB_ITERS", "10"))
forms = [m for m in os.environ.get("CB_FORMS", "").split(",") if m]
rounds = int(os.environ.get("CB_ROUNDS", "5"))
if forms:
    assert L.lib().dvf_build_has_tuning(), "CB_FORMS needs the tuning build (DVF_PIPE_LR is one of its knobs)"


def ab_forms(name, wt, b, cfg, xs, g):
    res, t = {}, {m: {"conv_fwd": [], "conv_dgrad": []} for m in forms}
    for _ in range(rounds):
        for m in forms:
            os.environ["DVF_PIPE_LR"] = m
            L.TIMER = L.KernelTimer()
            with L.plan_log() as log:
                for _ in range(iters):
                    for x in xs:
                        x.grad = None
                    out = ConvFn.apply(wt, b, cfg, *xs)
                    out.backward(g)
            summ, plans = L.TIMER.summary(), log.records
            L.TIMER = None
            for kind in t[m]:
                t[m][kind].append(summ[kind]["ms"] / summ[kind]["calls"] * 1e3)
            res[m] = (out.detach().clone(), [x.grad.clone() for x in xs], plans)
    o0, g0, _ = res[forms[0]]
    eq = all(torch.equal(o0, res[m][0]) and all(torch.equal(a, c) for a, c in zip(g0, res[m][1])) for m in forms)
    for m in forms:
        pipes = sorted((pl.op, (pl.MT, pl.NT, pl.WM, pl.CK, pl.TBU), pl.threads, pl.lds, int(pl.lr)) for pl in res[m][2] if pl.kernel == L.K_PIPE)
        line = f"{name:36s} LR={m}"
        for kind in ("conv_fwd", "conv_dgrad"):
            v = t[m][kind]
            line += f" | {kind[5:]:5s} med {statistics.median(v):7.1f} min {min(v):7.1f} max {max(v):7.1f} us"
        print(line, "| biteq", eq, "|", pipes, flush=True)


for name, segs, cout, k, s, p, op, tr, act, (n, h, w), ohw in LAYERS:
    if flt not in name:
        continue
    cin = sum(segs)
    xs = [torch.randn(n, c, h, w, device="cuda", requires_grad=True) for c in segs]
    wt = (torch.randn((cin, cout, k, k) if tr else (cout, cin, k, k), device="cuda") / (cin * k * k) ** 0.5).requires_grad_(True)
    b = torch.zeros(cout, device="cuda", requires_grad=True)
    cfg = (k, s, p, op, tr, act, 1.0, 0.0, ohw)
    out = ConvFn.apply(wt, b, cfg, *xs)
    g = torch.randn_like(out)
    out.backward(g)
    torch.cuda.synchronize()
    if forms:
        ab_forms(name, wt, b, cfg, xs, g)
        continue
    L.TIMER = L.KernelTimer()
    for _ in range(iters):
        out = ConvFn.apply(wt, b, cfg, *xs)
        out.backward(g)
    summ = L.TIMER.summary()
    L.TIMER = None
    line = f"{name:36s}"
    for kind in ("conv_fwd", "conv_dgrad", "conv_wgrad"):
        d = summ[kind]
        ms = d["ms"] / d["calls"]
        line += f" | {kind[5:]:5s} {ms*1e3:7.1f} us {d['flops']/d['calls']/(ms*1e-3)/1e12:6.1f} TF"
    print(line, flush=True)
