"""Parity AT THE SHAPES THE BENCHMARK RUNS (cfg 2: 256x832, batch 4).

The convolution planner is shape dependent (tile arrangement, NT, stage count / LDS budget, split-K factor, producer
waves, wgrad channel chunks and vector paths all derive from N*H*W), so the toy-size cases of test_gpu_conv.py do not
prove the kernel variants the headline number runs on.  Here:

  1. one full-size training step (DispNetS + PoseExpNet, photometric V=2 + 10*smooth) is compared with the CPU oracle
     -- per-term losses and every parameter's gradient -- while every convolution geometry of the step and every plan
     record the library reports (dvf_conv2d_last_plans) is collected;
  2. every distinct convolution geometry of that step is run alone (forward, dgrad of the segments that need it, wgrad,
     bias grad) against torch CPU conv2d / conv_transpose2d at 1e-4;
  3. the set of plans hit in 2 must contain the set the step used in 1;
  4. deterministic mode (dvf.conv.set_deterministic): every geometry of 2 again with the ordered weight / bias reductions,
     at 1e-4 against the same torch CPU tensors and bit-identical from run to run; per configuration, the deterministic
     step against the default one (see test_deterministic_step_matches_default).
Bound: 1e-4 relative (max-abs error / max-abs reference) per layer; for the step, losses at 1e-4 and gradients by
norm at 1e-4, and by norm of the difference at max(2e-4, 8 x the fp32 oracle's own distance from an fp64 run of the
oracle): composite gradients of the deep layers are ill-conditioned in fp32 for ANY implementation (the CPU oracle is
2.5e-4 away from fp64 at conv7), so the bound is stated relative to that measured floor; a wrong kernel is O(1) off."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import nets as onets
from oracle import steps as osteps

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda"
B, H, W = 4, 256, 832
STATE = {}


def _ref_act(x, act, alpha, beta):
    if act == 1:
        return F.relu(x)
    if act == 2:
        return alpha * torch.sigmoid(x) + beta
    return x


def _step_nets():
    import DispNetS
    import PoseExpNet
    dsd = onets.fill_params(onets.dispnet_layers(), seed=1)
    psd = onets.fill_params(onets.posenet_layers(6, 6, 2, True), seed=2)
    disp, pose = DispNetS.DispNetS(), PoseExpNet.PoseExpNet(output_exp=True)
    disp.load_state_dict({k: v.clone() for k, v in dsd.items()})
    pose.load_state_dict({k: v.clone() for k, v in psd.items()})
    return dsd, psd, disp.to(DEV).train(), pose.to(DEV).train()


def test_fullsize_step_vs_oracle():
    """cfg-2 step at the benchmark size through FlatAdam's arena (weight gradients accumulate in place on the side
    streams, exactly as bench.py runs it) vs oracle.steps.step_unsupervise(do_update=False)."""
    from dvf import conv as C
    from dvf import lib as L
    from dvf.engine import FlatAdam
    from dvf.steps import unsupervise_losses
    from dvf.synthetic import synthetic_batch
    dsd, psd, disp, pose = _step_nets()
    opt = FlatAdam(list(pose.parameters()) + list(disp.parameters()), lr=1e-3, weight_decay=1e-8)
    batch = synthetic_batch(B, H, W, seed=1234, device=DEV)
    STATE["geoms"], STATE["step_plans"] = [], set()
    with C.geom_log(STATE["geoms"]), L.plan_log(STATE["step_plans"]):
        loss, terms = unsupervise_losses(disp, pose, batch)
        opt.zero_grad()
        loss.backward()
        opt.join_wgrad()
        L.join_aux_streams()
        torch.cuda.synchronize()
    ref, grads, _ = osteps.step_unsupervise(dsd, psd, osteps.synthetic_batch(B, H, W, seed=1234), do_update=False)
    # fp64 run of the same oracle: ground truth for the noise floor of fp32 itself (ReLU gates and bilinear tap sets of
    # near-degenerate pixels flip under a different summation order; the deep 2x7 layers collect that noise)
    d64 = lambda sd: {k: v.double() for k, v in sd.items()}
    _, grads64, _ = osteps.step_unsupervise(d64(dsd), d64(psd), osteps.synthetic_batch(B, H, W, seed=1234, dtype=torch.float64),
                                            do_update=False)
    for k in ("img", "smooth", "total"):
        assert rel_err(terms[k], ref[k]) < TOL, (k, float(terms[k]), float(ref[k]))
    worst = (0.0, 0.0, "")
    for name, mod in (("disp", disp), ("pose", pose)):
        for k, p in mod.named_parameters():
            if k not in grads[name]:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
                continue
            r = grads[name][k].double()
            g = p.grad.detach().double().cpu()
            rn = max(float(r.norm()), 1e-30)
            e_norm, e_diff = abs(float(g.norm()) - rn) / rn, float((g - r).norm()) / rn
            worst = max(worst, (e_diff, e_norm, f"{name}.{k}"))
            r64 = grads64[name][k]
            floor, e64 = float((r - r64).norm()) / rn, float((g - r64).norm()) / rn
            assert e_norm < TOL or abs(float(g.norm()) - float(r64.norm())) / rn < max(TOL, 2 * abs(float(r.norm()) - float(r64.norm())) / rn), (name, k, e_norm)
            # direction: 2e-4, or 8x the distance of the fp32 ORACLE ITSELF from the fp64 truth for this parameter.
            # Round 3 measured what that factor is (profiles/r03_gradient_noise_seeds.txt, r03_noise_knobs.txt,
            # r03_blocked_accumulation.txt): with the SAME kernels the ratio |g - g64| / |g32 - g64| of the deep layers is
            # 0.3 ... 8 depending on the data / weight seed alone, and on this seed it moves 0.9 <-> 9 with the summation
            # blocking of the forward / dgrad kernels although every layer's own rms error stays at or below torch's CPU
            # kernels' (1.4-2.0e-7).  It counts which of two fp32 runs drew the worse set of ReLU-gate / bilinear-cell flips;
            # it cannot be tightened to 2x by better arithmetic.  A wrong kernel is O(1) off.
            assert e_diff < max(2e-4, 8 * floor) and e64 < max(2e-4, 8 * floor), (name, k, e_diff, e64, floor)
    print("worst gradient: |g-ref|/|ref| = %.2e, norm error %.2e at %s" % worst)


def _distinct(geoms):
    seen, out = set(), []
    for g in geoms:
        if g not in seen:
            seen.add(g)
            out.append(g)
    return out


def _check_geometry(gi, geom, failures):
    """Forward / dgrad / wgrad / bias-grad of one convolution geometry against torch CPU at 1e-4: plain, and in the fused
    form the steps run (masked dgrad, weight gradient + bias column)."""
    from dvf.conv import ConvFn, ReluTag
    segs, cout, cfg, (n, h, w), need_in = geom
    k, stride, pad, opad, transposed, act, alpha, beta, out_hw = cfg
    gen = torch.Generator().manual_seed(1000 + gi)
    cin = sum(segs)
    xs = [torch.randn(n, c, h, w, generator=gen) for c in segs]
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    wt = torch.randn(wshape, generator=gen) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=gen) * 0.1
    rx = [x.clone().requires_grad_(ng) for x, ng in zip(xs, need_in)]
    rw, rb = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xin = torch.cat(rx, 1)
    if transposed:
        pre = F.conv_transpose2d(xin, rw, rb, stride=stride, padding=pad, output_padding=opad)
    else:
        pre = F.conv2d(xin, rw, rb, stride=stride, padding=pad)
    if out_hw is not None:
        pre = pre[:, :, :out_hw[0], :out_hw[1]]
    ref = _ref_act(pre, act, alpha, beta)
    gout = torch.randn(ref.shape, generator=gen)
    if act == 1:
        gout = gout * (pre.detach().abs() > 1e-4)       # ReLU kink: see test_gpu_conv.py
    (ref * gout).sum().backward()
    gx = [x.clone().to(DEV).requires_grad_(ng) for x, ng in zip(xs, need_in)]
    gw, gb = wt.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)
    out = ConvFn.apply(gw, gb, cfg, *gx)
    (out * gout.to(DEV)).sum().backward()
    tag = f"{'T' if transposed else 'C'}{k}x{k}s{stride} {list(segs)}->{cout} @{h}x{w} N{n}"
    errs = {"fwd": rel_err(out, ref), "wgrad": rel_err(gw.grad, rw.grad), "bias": rel_err(gb.grad, rb.grad)}
    for i, (a, r) in enumerate(zip(gx, rx)):
        if r.grad is not None:
            errs[f"dgrad{i}"] = rel_err(a.grad, r.grad)
    bad = {kk: v for kk, v in errs.items() if not v < TOL}
    if bad or tuple(out.shape) != tuple(ref.shape):
        failures.append((tag, bad))
    del out, gx, gw, gb

    def plain():
        hx = [x.clone().to(DEV).requires_grad_(ng) for x, ng in zip(xs, need_in)]
        hw, hb = wt.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)
        ConvFn.apply(hw, hb, cfg, *hx).backward(gout.to(DEV))
        return hw.grad, hb.grad
    _check_deterministic(tag, "", plain, rw.grad, rb.grad, failures)
    del rx, rw, rb, ref, pre, gout
    # ---- the same geometry as the step runs it (dvf/conv.py::ReluTag): inputs are outputs of ReLU layers, so the
    # dgrad leaves multiplied by (x > 0); a ReLU layer itself receives dL/dpre (its consumers masked it) and its
    # bias gradient is the extra column of the weight-gradient kernel (dvf_conv2d_wgrad)
    xs2 = [F.relu(x) for x in xs]
    rx = [x.clone().requires_grad_(ng) for x, ng in zip(xs2, need_in)]
    rw, rb = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xin = torch.cat(rx, 1)
    if transposed:
        pre = F.conv_transpose2d(xin, rw, rb, stride=stride, padding=pad, output_padding=opad)
    else:
        pre = F.conv2d(xin, rw, rb, stride=stride, padding=pad)
    if out_hw is not None:
        pre = pre[:, :, :out_hw[0], :out_hw[1]]
    ref = _ref_act(pre, act, alpha, beta)
    gout = torch.randn(ref.shape, generator=gen)
    if act == 1:
        gout = gout * (pre.detach().abs() > 1e-4)
    (ref * gout).sum().backward()
    gx = [x.clone().to(DEV).requires_grad_(ng) for x, ng in zip(xs2, need_in)]
    for x in gx:
        x._dvf_relu_tag = ReluTag()
    gw, gb = wt.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)
    out = ConvFn.apply(gw, gb, tuple(cfg) + ((ReluTag(),) if act == 1 else ()), *gx)
    go = gout * (ref.detach() > 0) if act == 1 else gout        # what masking consumers deliver
    out.backward(go.to(DEV))
    errs = {"fused wgrad": rel_err(gw.grad, rw.grad), "fused bias": rel_err(gb.grad, rb.grad)}
    for i, (a, r, x0) in enumerate(zip(gx, rx, xs2)):
        if r.grad is not None:
            errs[f"masked dgrad{i}"] = rel_err(a.grad, r.grad * (x0 > 0))
    bad = {kk: v for kk, v in errs.items() if not v < TOL}
    if bad:
        failures.append((tag, bad))
    del out, gx, gw, gb

    def fused():
        hx = [x.clone().to(DEV).requires_grad_(ng) for x, ng in zip(xs2, need_in)]
        for x in hx:
            x._dvf_relu_tag = ReluTag()
        hw, hb = wt.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)
        ConvFn.apply(hw, hb, tuple(cfg) + ((ReluTag(),) if act == 1 else ()), *hx).backward(go.to(DEV))
        return hw.grad, hb.grad
    _check_deterministic(tag, "fused ", fused, rw.grad, rb.grad, failures)
    del rx, rw, rb, ref, pre, gout, go


def _check_deterministic(tag, form, run, ref_w, ref_b, failures):
    """Two runs of `run` (returns the weight and bias gradients of one HIP backward) under dvf.conv.set_deterministic(True):
    ordered weight / bias reductions (wgrad_pipe slabs + wgrad_reduce_kernel, act_bwd partials + bias_finish_kernel, head
    partials + head_wgrad_finish_kernel).  Both against the same torch CPU reference at 1e-4, and bit-identical to each
    other.  Their plan records go to STATE['det_layer_plans']."""
    from dvf import conv as C
    from dvf import lib as L
    C.set_deterministic(True)
    try:
        with L.plan_log(STATE.setdefault("det_layer_plans", set())):
            (w1, b1), (w2, b2) = run(), run()
    finally:
        C.set_deterministic(False)
    errs = {f"det {form}wgrad": rel_err(w1, ref_w), f"det {form}bias": rel_err(b1, ref_b)}
    bad = {kk: v for kk, v in errs.items() if not v < TOL}
    if not torch.equal(w1, w2):
        bad[f"det {form}wgrad repeat"] = float((w1 - w2).abs().max())
    if not torch.equal(b1, b2):
        bad[f"det {form}bias repeat"] = float((b1 - b2).abs().max())
    if bad:
        failures.append((tag, bad))


def _check_geometries(geoms, seed_base):
    """Run the geometries not parity-checked yet (any configuration); their plan records join STATE['layer_plans']."""
    from dvf import lib as L
    done = STATE.setdefault("checked_geoms", set())
    failures = []
    with L.plan_log(STATE.setdefault("layer_plans", set())):
        for gi, geom in enumerate(geoms):
            if geom in done:
                continue
            _check_geometry(seed_base + gi, geom, failures)
            done.add(geom)
            torch.cuda.empty_cache()
    assert not failures, failures


def test_every_bench_layer_geometry():
    """Forward / dgrad / wgrad / bias-grad of every distinct convolution geometry of the cfg-2 step at batch 4."""
    if "geoms" not in STATE:
        test_fullsize_step_vs_oracle()
    geoms = _distinct(STATE["geoms"])
    assert len(geoms) >= 40, len(geoms)            # DispNetS: 14 + 7 + 7 + 4, PoseExpNet: 7 + 1 + 5 + 4 (some coincide)
    _check_geometries(geoms, 0)


def test_bench_plans_are_the_tested_plans():
    """Every (op, kernel, tiling) record of the full-size step also ran in a per-layer parity case."""
    if "layer_plans" not in STATE:
        test_every_bench_layer_geometry()
    step, layer = STATE["step_plans"], STATE["layer_plans"]
    assert step, "the library reported no plans"
    missing = sorted(step - layer)
    assert not missing, missing
    from dvf.lib import K_PIPE, K_WGRAD_PIPE
    kernels = {p.kernel for p in step}
    assert {K_PIPE, K_WGRAD_PIPE} <= kernels, kernels
    print("%d distinct plans in the step, all parity-tested; kernels used: %s" % (len(step), sorted(kernels)))


# ---------------------------------------------------------------------------------------------------- cfg 3 / 4 / 5
# The other benchmark configurations (bench.CONFIGS): FeatExtractor on 3 x 8 full-resolution images
# (reference: unsupervise.py:104-111), the 4-scale train.py body with the feature term, and 384x1280 with a five-frame
# window (PoseExpNet_sfm.py:22-36: a 15-channel first convolution; loss_functions_sfm.py:9-46 with V = 4).  One full-size
# step per configuration collects every convolution geometry and every plan record; each geometry not seen before is
# parity-checked against torch CPU at 1e-4 (plain and fused forms); the step's plans must be a subset of the
# parity-checked plans.  The step itself -- every loss term and every parameter's gradient in FlatAdam's arena -- is
# compared with a full-size oracle step from the same weights and batch, in fp32 and in fp64 (about 10-35 s of CPU time
# each, up to ~23 GB of host memory for cfg 5 in fp64), with the bound shape of test_fullsize_step_vs_oracle.  A few
# gradients are sums over millions of pixels that cancel: the fp32 oracle itself is more than 1e-2 away from fp64 there
# (CANCELLING), so only their distance from fp64 is bounded, against the fp32 oracle's; tests/test_gpu_bench_kernels.py
# checks the kernels behind them directly.
CANCELLING = {3: {"feat.conv_3_bb4_up.bias"}, 4: set(), 5: set()}
LOSS_FLOOR_FACTOR = 4


def _oracle_step(cfg, sds, dtype):
    """(loss terms, {net: {param: grad}}) of the full-size oracle step of one configuration in `dtype`."""
    b = osteps.synthetic_batch(cfg["batch"], cfg["height"], cfg["width"], seed=1234, n_views=cfg["nb_ref"])
    b = {k: ([x.to(dtype) for x in v] if isinstance(v, list) else v.to(dtype)) for k, v in b.items()}
    sd = {n: {k: v.to(dtype) for k, v in d.items()} for n, d in sds.items()}
    if cfg["body"] == "unsupervise":
        out, grads, _ = osteps.step_unsupervise(sd["disp"], sd["pose"], b, feat_sd=sd.get("feat"), do_update=False)
    else:
        out, grads, _ = osteps.step_train_sfm(sd["disp"], sd["pose"], b, feat_sd=sd.get("feat"), nb_ref_imgs=cfg["nb_ref"],
                                              do_update=False)
    return {k: float(v) for k, v in out.items()}, grads


def _check_step_vs_oracle(config, cfg, terms, grads, sds):
    """terms: the HIP step's loss terms (floats); grads: {"net.param": HIP gradient (CPU)}; sds: the networks' state dicts
    (CPU).  Returns the worst ratio of a gradient's distance to its bound."""
    ref, g32 = _oracle_step(cfg, sds, torch.float32)
    ref64, g64 = _oracle_step(cfg, sds, torch.float64)
    failures = []
    for k, v in terms.items():
        floor = abs(ref[k] - ref64[k]) / abs(ref64[k])
        if not (abs(v - ref[k]) <= TOL * abs(ref[k]) or
                abs(v - ref64[k]) <= max(TOL, LOSS_FLOOR_FACTOR * floor) * abs(ref64[k])):
            failures.append((k, v, ref[k], ref64[k]))
    worst = (0.0, "", 0.0)
    for name, g in grads.items():
        net, k = name.split(".", 1)
        if k not in g32[net]:
            if float(g.abs().max()) != 0.0:
                failures.append((name, "gradient where the oracle has none"))
            continue
        g = g.double()
        r, r64 = g32[net][k].double(), g64[net][k]
        rn = max(float(r.norm()), 1e-30)
        floor = float((r - r64).norm()) / rn
        if name in CANCELLING[config]:
            # a cancelling sum: no further from fp64 than 8x the fp32 oracle, plus 1e-4 of the fp64 norm
            if not float((g - r64).norm()) <= 8 * float((r - r64).norm()) + 1e-4 * float(r64.norm()):
                failures.append((name, "cancelling", float((g - r64).norm()), float((r - r64).norm())))
            continue
        # norm and direction, both within max(2e-4, 8 x floor), floor = |g32 - g64| / |g32| (the cfg-2 bound)
        bound = max(2e-4, 8 * floor)
        e_norm, e_norm64 = abs(float(g.norm()) - rn) / rn, abs(float(g.norm()) - float(r64.norm())) / rn
        e_diff, e64 = float((g - r).norm()) / rn, float((g - r64).norm()) / rn
        if not (e_norm < TOL or e_norm64 < bound) or not (e_diff < bound and e64 < bound):
            failures.append((name, e_norm, e_norm64, e_diff, e64, floor))
        worst = max(worst, (max(e_diff, e64) / bound, name, floor))
    assert not failures, (config, failures)
    return worst


def _bench_module():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("dvf_bench_for_tests", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("config", [3, 4, 5])
def test_other_bench_configs_geometries_and_plans(config):
    import argparse
    from dvf import conv as C
    from dvf import lib as L
    bench = _bench_module()
    cfg = bench.CONFIGS[config]
    args = argparse.Namespace(batch=cfg["batch"], height=cfg["height"], width=cfg["width"], seed=0, force_ddp=False,
                              no_graph=True)
    step, fwd_bwd, opt, _, nets = bench.build(args, cfg, torch.device(DEV), 1, 0)
    # the same batch as bench.build's (dvf.synthetic); the oracle builds its own from its own copy of the recipe
    from dvf.synthetic import synthetic_batch
    mine = synthetic_batch(cfg["batch"], cfg["height"], cfg["width"], seed=1234, n_views=cfg["nb_ref"])
    theirs = osteps.synthetic_batch(cfg["batch"], cfg["height"], cfg["width"], seed=1234, n_views=cfg["nb_ref"])
    for k, v in theirs.items():
        assert all(torch.equal(a, b) for a, b in zip(v, mine[k])) if isinstance(v, list) else torch.equal(v, mine[k]), k
    assert len(theirs["extra_refs"]) == len(mine["extra_refs"]) == cfg["nb_ref"] - 2
    del mine, theirs
    sds = {n: {k: v.detach().cpu().clone() for k, v in net.state_dict().items()} for n, net in nets.items()}
    fwd_bwd()                                         # (first pass: packs, workspaces)
    with C.geom_log() as geoms, L.plan_log() as log:
        total, terms = fwd_bwd()
        L.join_aux_streams()
        torch.cuda.synchronize()
    geoms, step_plans = _distinct(geoms), log.records
    assert torch.isfinite(total).all(), float(total)
    assert float(opt.flat_g.abs().max()) > 0 and torch.isfinite(opt.flat_g).all()
    terms = {k: float(v) for k, v in terms.items()}
    grads = {f"{n}.{k}": opt.flat_g[p._dvf_offset:p._dvf_offset + p.numel()].view(p.shape).cpu()
             for n, net in nets.items() for k, p in net.named_parameters()}
    del step, fwd_bwd, opt, nets
    torch.cuda.empty_cache()
    assert geoms and step_plans
    _check_geometries(geoms, 10000 * config)
    missing = sorted(step_plans - STATE["layer_plans"])
    assert not missing, (config, missing)
    print("cfg %d: %d geometries, %d plans, all parity-tested" % (config, len(geoms), len(step_plans)))
    ratio, name, floor = _check_step_vs_oracle(config, cfg, terms, grads, sds)
    print("cfg %d vs oracle: worst gradient at %.2f of its bound, %s (fp32 oracle floor %.2e)" % (config, ratio, name, floor))


# ---------------------------------------------------------------------------------------------------- deterministic mode
# dvf.conv.set_deterministic(True) swaps every float-atomic weight / bias sum of the step for an ordered one.  Per layer,
# _check_geometry compares those paths with torch CPU (above).  Per step, on the arena path (side streams, accumulation into
# FlatAdam.flat_g, modules used twice), three eager passes from the same weights -- deterministic, deterministic, default --
# must give (a) bit-identical arenas for the two deterministic passes outside the feature term's exception, (b) the default
# arena up to reduction noise (only the summation order of weight / bias gradients differs, and those feed nothing else in
# the step: an O(1) difference is a mapping bug), (c) ordered weight-gradient kernels only, (d) no plan the per-layer
# deterministic checks did not run.
DET_TOL = 1e-5         # deterministic vs default arena, per parameter (rel_err)
DET_TOL_FEAT = 1e-4    # FeatExtractor parameters: their gradients come through the photometric kernel's atomic scatter


@pytest.mark.parametrize("config", [2, 3, 4, 5])
def test_deterministic_step_matches_default(config):
    import argparse
    from dvf import conv as C
    from dvf import lib as L
    bench = _bench_module()
    cfg = bench.CONFIGS[config]
    args = argparse.Namespace(batch=cfg["batch"], height=cfg["height"], width=cfg["width"], seed=0, force_ddp=False,
                              no_graph=True)
    step, fwd_bwd, opt, _, nets = bench.build(args, cfg, torch.device(DEV), 1, 0)

    def arena():
        fwd_bwd()
        L.join_aux_streams()
        torch.cuda.synchronize()
        return opt.flat_g.clone()

    # the first deterministic pass of the process grows the side streams' scratch (dvf/conv.py::_workspace)
    C.set_deterministic(True)
    try:
        with C.geom_log() as geoms, L.plan_log() as log:
            det1 = arena()
        geoms, det_plans = _distinct(geoms), log.records
        det2 = arena()
    finally:
        C.set_deterministic(False)
    default = arena()
    assert float(det1.abs().max()) > 0 and torch.isfinite(det1).all()
    worst, worst_feat = (0.0, ""), (0.0, "")
    for net_name, net in nets.items():
        for k, p in net.named_parameters():
            name = f"{net_name}.{k}"
            sl = slice(p._dvf_offset, p._dvf_offset + p.numel())
            a, a2, d = det1[sl], det2[sl], default[sl]
            feat = net_name == "feat"
            if not feat:
                # (a) outside the feature term's source-gradient scatter (float atomics across blocks), bit identity
                assert torch.equal(a, a2), (config, name, float((a - a2).abs().max()))
            e = rel_err(a, d)
            assert e <= (DET_TOL_FEAT if feat else DET_TOL), (config, name, e)
            if feat:
                worst_feat = max(worst_feat, (e, name))
            else:
                worst = max(worst, (e, name))
    del step, fwd_bwd, opt, nets, arena, det1, det2, default
    torch.cuda.empty_cache()
    # (c) every weight gradient of the deterministic step went through an ordered path
    # (PlanRecord.ordered: wgrad_pipe with its slabs in scratch, the direct head kernel with its partials buffer)
    wrecs = [r for r in det_plans if r.op == "wgrad"]
    assert wrecs, "the library reported no weight-gradient plans"
    unordered = sorted(r for r in wrecs if not r.ordered)
    assert not unordered, (config, unordered)
    # (d) and through plans the per-layer deterministic checks ran against torch CPU
    _check_geometries(geoms, 10000 * config)
    missing = sorted(det_plans - STATE["det_layer_plans"])
    assert not missing, (config, missing)
    print("cfg %d deterministic vs default: worst rel_err %.2e at %s; FeatExtractor %s; %d plans" %
          (config, worst[0], worst[1], "%.2e at %s" % worst_feat if worst_feat[1] else "-", len(det_plans)))
