"""Bit-exact parity of every convolution plan at the shapes the product trains at (tests/product_shapes.py: 128x416 at
batch 1 and 4, 192x640 at batch 3 and 12, 320x1024 at batch 2; the cfg-4 body everywhere, the cfg-2 and cfg-5 bodies at
3x192x640).  test_gpu_conv_exact.py proves "step plans are exactly tested plans" for the four bench steps only; the coarse
maps here are 2x7 ... 12x40 at 256-512 channels, another corner of every planner threshold, with ragged tiles no bench
step forms.

One case per recorded layer geometry (tests/product_shape_geoms.json; geometries of the bench steps are pinned there and
left out): test_gpu_conv_exact.check_geometry, i.e. plain / fused x default / deterministic, forward and every gradient
EQUAL to the fp64 reference (sigmoid layers: act = NONE, and 6 ulp on the sigmoid forward).  One case per (body, shape)
then runs the live step: its geometries must be the table's, its plan records must all have run in an exact case of that
shape, every weight gradient of its deterministic pass must be ordered.  No call may fill the plan log (plan_capture)."""
import time

import pytest
import torch

import conv_exact as X
import product_shapes as PS
import test_gpu_conv_exact as TE

pytestmark = pytest.mark.gpu

BENCH_GEOMS, TABLE = PS.load_table()
# per (body, shape): plan records of its exact cases, the geometries that ran, wall time per case id
STATE = {"plans": {k: set() for k in TABLE}, "ran": {k: set() for k in TABLE}, "seconds": {}, "step": {}}

# A geometry that several bodies run at one shape (DispNetS at 3x192x640) is one case, named after the first of them; its
# plan records count for each.
OWNERS = {}
for _key, (_geoms, _) in TABLE.items():
    for _g in _geoms:
        OWNERS.setdefault(_g, []).append(_key)

# check_geometry costs what its two fp64 CPU references cost (plain; fused: inputs as ReLU outputs): about 0.4 s per 1e9
# multiply-adds of the forward pass for all four forms.  Above this many the plain and the fused pair of forms are two cases
# of 2-4 s; the two 36x192x640 layers of 40.8e9 still take 7-11 s per half, and a smaller N, H or W would be another plan
# (measured: profiles/product_shapes_exact.txt).
SPLIT_MACS = 10e9


def _macs(geom):
    segs, cout, cfg, (n, h, w), _ = geom
    oh, ow = X.out_hw_of(geom)
    taps = cfg[0] * cfg[0] / (cfg[1] * cfg[1]) if cfg[4] else cfg[0] * cfg[0]
    return n * cout * oh * ow * sum(segs) * taps


CASES = [(geom, forms) for geom in OWNERS
         for forms in (((False,), (True,)) if _macs(geom) > SPLIT_MACS else ((False, True),))]


def _case_id(geom, forms):
    body, shape = OWNERS[geom][0]
    return "%s-%dx%dx%d-%s%s" % ((body,) + tuple(shape) + (PS.geom_label(geom), {(False,): "-plain", (True,): "-fused"}.get(forms, "")))


def _exact(keys, name, geom, forms=(False, True)):
    """check_geometry with the plan records of its runs kept apart, under the (body, shape)s they belong to (the union
    that test_gpu_conv_exact.py collects stays its own: the report below measures against it)."""
    saved, mine = TE.STATE["plans"], set()
    TE.STATE["plans"] = mine
    t0 = time.perf_counter()
    try:
        TE.check_geometry(name, geom, X.seed_of(name), forms=forms)
    finally:
        TE.STATE["plans"] = saved
        for key in keys:
            STATE["plans"][key] |= mine
        STATE["seconds"][name] = time.perf_counter() - t0
        torch.cuda.empty_cache()
    for key in keys:
        STATE["ran"][key].add((geom, forms))


@pytest.mark.parametrize("geom,forms", CASES, ids=[_case_id(*c) for c in CASES])
def test_product_geometry_exact(geom, forms):
    _exact(OWNERS[geom], _case_id(geom, forms), geom, forms)


# Weight-gradient plan records of a deterministic step that are not .ordered, with the reason: {(body, shape): {record: why}}.
# Empty: every weight gradient of every lattice step runs an ordered reduction.
UNORDERED_IN_DETERMINISTIC_STEP = {}


@pytest.mark.parametrize("body,shape", PS.STEPS, ids=[PS.step_key(*s).replace(" ", "-") for s in PS.STEPS])
def test_product_step_plans_are_the_tested_plans(body, shape):
    """Runs after the exact cases of its (body, shape)."""
    key = (body, shape)
    table_geoms = TABLE[key][0]
    if STATE["ran"][key] != {c for c in CASES if key in OWNERS[c[0]]}:
        pytest.fail("the exact cases of %s did not all pass before this test (run the whole module)" % PS.step_key(*key))
    bench = PS.live_bench_geoms()
    assert bench == BENCH_GEOMS, ("the bench steps' geometries changed: rerun tools/product_shape_geoms.py",
                                  sorted(map(str, set(bench) ^ set(BENCH_GEOMS))))
    geoms, plans, det_plans = PS.record_step(body, shape)
    STATE["step"][key] = (geoms, plans | det_plans)
    # (a) the table is what the step runs
    live = [g for g in geoms if g not in set(bench)]
    assert live == table_geoms, (key, "the step's geometries changed: rerun tools/product_shape_geoms.py",
                                 sorted(map(str, set(live) ^ set(table_geoms))))
    assert sorted(PS.plan_to_json(r) for r in plans | det_plans) == TABLE[key][1], \
        (key, "the step's plan records changed: rerun tools/product_shape_geoms.py")
    # (b) step plans within exactly tested plans; a geometry shared with a bench step is run here unless
    # test_bench_geometries_exact has run it in this process
    tested = set(STATE["plans"][key])
    shared = [g for g in geoms if g in set(bench)]
    for gi, geom in enumerate(shared):
        if geom in TE.STATE["done"]:
            tested |= TE.STATE["plans"]
        else:
            _exact([key], "%s shared #%d %s" % (PS.step_key(*key), gi, PS.geom_label(geom)), geom)
            tested |= STATE["plans"][key]
    missing = sorted((plans | det_plans) - tested)
    assert not missing, (key, "step plans no exact case of this shape ran", missing)
    # ordered reductions in the deterministic pass
    wrecs = [r for r in det_plans if r.op == "wgrad"]
    assert wrecs, "the library reported no weight-gradient plans"
    allowed = UNORDERED_IN_DETERMINISTIC_STEP.get(key, {})
    unordered = {r for r in wrecs if not r.ordered}
    assert not sorted(unordered - set(allowed)), (key, "unordered weight gradients in deterministic mode",
                                                  sorted(unordered - set(allowed)))
    stale = sorted(set(allowed) - unordered)
    assert not stale, (key, "ordered now: remove from UNORDERED_IN_DETERMINISTIC_STEP", stale)
    print("%s: %d geometries exact (+%d shared with a bench step), %d step plans all covered" %
          (PS.step_key(*key), len(table_geoms), len(shared), len(plans | det_plans)))


def test_product_shape_report():
    """Runs last: what the module pinned (profiles/product_shapes_exact.txt is this output).  Per (body, shape) the
    geometries and plan records; the step plan records that no exact run of test_gpu_conv_exact.py reaches, by kernel
    family (only when that module ran in this process); the slowest cases."""
    from dvf.lib import KERNELS
    if set(STATE["step"]) != set(PS.STEPS):
        pytest.fail("the step cases did not all run before this test (run the whole module)")
    for key in PS.STEPS:
        print("%-18s %3d geometries, %3d step plan records, %3d records in its exact cases" %
              (PS.step_key(*key), len(TABLE[key][0]), len(STATE["step"][key][1]), len(STATE["plans"][key])))
    earlier = TE.STATE["plans"]
    if not earlier:
        print("(test_gpu_conv_exact.py did not run in this process: no difference against its plan records)")
    else:
        step_all = set().union(*(STATE["step"][k][1] for k in PS.STEPS))
        exact_all = set().union(*STATE["plans"].values())
        print("test_gpu_conv_exact.py reached %d plan records; the lattice steps run %d, of which %d are new; "
              "the lattice's exact cases ran %d, of which %d are new" %
              (len(earlier), len(step_all), len(step_all - earlier), len(exact_all), len(exact_all - earlier)))
        for fam in sorted(KERNELS):
            new = sorted(r for r in step_all - earlier if r.kernel == fam)
            if new:
                print("%s: %d new step plan records" % (KERNELS[fam], len(new)))
                for r in new:
                    print("   ", tuple(r))
    slow = sorted(STATE["seconds"].items(), key=lambda kv: -kv[1])
    print("exact cases: %d, %.1f s in all; slowest:" % (len(slow), sum(s for _, s in slow)))
    for name, s in slow[:8]:
        print("    %6.2f s  %s" % (s, name))
