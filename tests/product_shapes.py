"""The lattice of product shapes whose convolution plans are pinned exactly (tests/test_gpu_conv_product_shapes.py), and
the recorded table of their layer geometries (tests/product_shape_geoms.json, written by tools/product_shape_geoms.py).

The bench configurations run at 256x832 / 384x1280 with batch 4 / 8; the planner's thresholds (image batching at px <= 64,
WM = 2, NT = 1 below 512 blocks, split-K below 160, the 150 KB LDS budget, the two-blocks-per-CU form, the 16-byte lanes)
fall elsewhere at the shapes training actually runs at.  LATTICE holds those: 128x416 (the reference's and SfMLearner's
default) at batch 1 and 4, 192x640 (the monodepth2 recipe) at batch 12 and at an odd per-rank batch of 3, 320x1024 at
batch 2.  A body is the network set and loss composition of a bench configuration (bench.CONFIGS), run at a lattice shape.

Everything above record_step() is plain data handling and runs without a GPU."""
import json
import os

LATTICE = [(1, 128, 416), (4, 128, 416), (3, 192, 640), (12, 192, 640), (2, 320, 1024)]
BODIES = {"cfg4": 4, "cfg2": 2, "cfg5": 5}        # body -> the bench configuration whose body fields it takes
# cfg 4 (DispNetS + PoseExpNet_sfm, nb_ref = 2, + FeatExtractor; train_sfm) everywhere; PoseExpNet / unsupervise and the
# five-frame window (nb_ref = 4) at the odd-batch 192x640 point
STEPS = [("cfg4", s) for s in LATTICE] + [("cfg2", (3, 192, 640)), ("cfg5", (3, 192, 640))]
BENCH_CONFIGS = (2, 3, 4, 5)
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "product_shape_geoms.json")
FORMAT = 1


def step_key(body, shape):
    return "%s %dx%dx%d" % ((body,) + tuple(shape))


def geom_to_json(geom):
    segs, cout, cfg, nhw, need_in = geom
    k, stride, pad, opad, transposed, act, alpha, beta, out_hw = cfg
    return [[int(c) for c in segs], int(cout),
            [int(k), int(stride), int(pad), int(opad), bool(transposed), int(act), float(alpha), float(beta),
             None if out_hw is None else [int(v) for v in out_hw]],
            [int(v) for v in nhw], [bool(v) for v in need_in]]


def geom_from_json(j):
    """The tuple form of dvf.conv.GEOM_LOG: (segs, cout, cfg[:9], (N, H, W), need_in); equal to and hashing as a live one."""
    segs, cout, cfg, nhw, need_in = j
    out_hw = None if cfg[8] is None else tuple(cfg[8])
    return (tuple(segs), cout, tuple(cfg[:8]) + (out_hw,), tuple(nhw), tuple(need_in))


def plan_to_json(rec):
    return [rec[0]] + [int(v) for v in rec[1:]]


def plan_from_json(j):
    from dvf.plans import PlanRecord
    return PlanRecord((j[0],) + tuple(j[1:]))


def geom_label(geom):
    """Short name of a layer geometry for test ids."""
    segs, cout, cfg, (n, h, w), need_in = geom
    k, stride, pad, opad, transposed, act, alpha, beta, out_hw = cfg
    crop = "" if out_hw is None else "_crop%dx%d" % tuple(out_hw)
    return "%s%dx%ds%d_%s-%d_act%d_in%dx%dx%d%s_g%s" % ("T" if transposed else "C", k, k, stride, "+".join(map(str, segs)), cout,
                                                      act, n, h, w, crop, "".join("1" if v else "0" for v in need_in))


def dump_table(bench_geoms, steps, path=TABLE):
    """steps: {(body, shape): (geometries, plan records)}.  One geometry / record per line, so that a regenerated table
    diffs by layer."""
    def rows(items, indent):
        return (",\n" + indent).join(json.dumps(i) for i in items)
    out = ['{"format": %d,' % FORMAT, ' "bench_geometries": [\n  ' + rows([geom_to_json(g) for g in bench_geoms], "  ") + "],",
           ' "steps": {']
    blocks = []
    for (body, shape), (geoms, plans) in steps.items():
        blocks.append('  %s: {"body": %s, "shape": %s,\n   "geometries": [\n    %s],\n   "plans": [\n    %s]}' % (
            json.dumps(step_key(body, shape)), json.dumps(body), json.dumps(list(shape)),
            rows([geom_to_json(g) for g in geoms], "    "),
            rows(sorted(plan_to_json(r) for r in plans), "    ")))
    out.append(",\n".join(blocks))
    out.append(" }\n}")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def load_table(path=TABLE):
    """-> (bench geometries, {(body, shape): (geometries, plan records as plain lists)}) in the GEOM_LOG tuple form."""
    with open(path) as f:
        j = json.load(f)
    assert j["format"] == FORMAT, j["format"]
    steps = {}
    for key, s in j["steps"].items():
        body, shape = s["body"], tuple(s["shape"])
        assert key == step_key(body, shape), key
        steps[(body, shape)] = ([geom_from_json(g) for g in s["geometries"]], [list(p) for p in s["plans"]])
    return [geom_from_json(g) for g in j["bench_geometries"]], steps


# ------------------------------------------------------------------------------------------------------------ GPU side
def record_step(body, shape):
    """One default and one deterministic fwd_bwd() of a body at a lattice shape, built as test_gpu_conv_exact._bench_step
    builds the bench steps (bench.build with the configuration's body fields), under geom_log + plan_log.
    -> (distinct geometries in call order, plan records of the default pass, of the deterministic pass)."""
    import argparse
    import torch
    import test_gpu_bench_shapes as BS
    import test_gpu_conv_exact as TE
    from dvf import conv as C
    from dvf import lib as L
    bench = BS._bench_module()
    cfg = bench.CONFIGS[BODIES[body]]
    args = argparse.Namespace(batch=shape[0], height=shape[1], width=shape[2], seed=0, force_ddp=False, no_graph=True)
    step, fwd_bwd, opt, _, nets = bench.build(args, cfg, torch.device(TE.DEV), 1, 0)
    geoms, plans = [], {False: set(), True: set()}
    try:
        for det in (False, True):
            C.set_deterministic(det)
            fwd_bwd()                                 # (first pass of a mode: packs, workspaces)
            with C.geom_log(geoms), TE.plan_capture(plans[det]):
                fwd_bwd()
                L.join_aux_streams()
                torch.cuda.synchronize()
    finally:
        C.set_deterministic(False)
    del step, fwd_bwd, opt, nets
    torch.cuda.empty_cache()
    return BS._distinct(geoms), plans[False], plans[True]


def live_bench_geoms():
    """Distinct geometries of the four bench steps, in configuration and call order."""
    import test_gpu_bench_shapes as BS
    import test_gpu_conv_exact as TE
    return BS._distinct([g for config in BENCH_CONFIGS for g in TE._bench_step(config)[0]])
