"""Record tests/product_shape_geoms.json (GPU box): the convolution layer geometries and plan records of the product-shape
lattice (tests/product_shapes.py: LATTICE, STEPS), for tests/test_gpu_conv_product_shapes.py and the CPU budget test.

usage: python tools/product_shape_geoms.py [output path]

Per (body, shape): one default and one deterministic fwd_bwd() under geom_log + plan_log.  Geometries that a bench step
(cfg 2-5) runs are left out of the steps' lists -- test_gpu_conv_exact.py pins those -- and listed once, as bench_geometries,
so that the table can be checked against them without a GPU.  Rerun after a change of a network or of the planner."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: F401,E402  (puts the package and the repository root on sys.path)
import product_shapes as PS  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else PS.TABLE
    bench = PS.live_bench_geoms()
    print("bench steps: %d distinct geometries" % len(bench))
    known = set(bench)
    steps = {}
    for body, shape in PS.STEPS:
        geoms, plans, det_plans = PS.record_step(body, shape)
        new = [g for g in geoms if g not in known]
        steps[(body, shape)] = (new, plans | det_plans)
        print("%-18s %3d geometries (%d more shared with a bench step), %3d plan records" %
              (PS.step_key(body, shape), len(new), len(geoms) - len(new), len(plans | det_plans)), flush=True)
    PS.dump_table(bench, steps, out)
    back_bench, back = PS.load_table(out)
    assert back_bench == bench and {k: v[0] for k, v in back.items()} == {k: v[0] for k, v in steps.items()}
    print("wrote %s" % out)


if __name__ == "__main__":
    main()
