"""CPU side of tests/test_gpu_conv_product_shapes.py: the recorded geometry table (tests/product_shape_geoms.json) is whole,
free of repeats, and every geometry in it has an integer-exact operand budget (tests/conv_exact.py) at its full size."""
import conv_exact as X
import product_shapes as PS

BENCH_GEOMS, TABLE = PS.load_table()


def test_table_covers_the_lattice():
    assert len(PS.LATTICE) == 5 and len(PS.STEPS) == 7
    assert set(TABLE) == set(PS.STEPS), sorted(set(TABLE) ^ set(PS.STEPS))
    assert BENCH_GEOMS
    for (body, shape), (geoms, plans) in TABLE.items():
        assert geoms and plans, (body, shape)
        for geom in geoms:
            segs, cout, cfg, nhw, need_in = geom
            assert len(cfg) == 9 and len(need_in) == len(segs) and cout >= 1 and min(segs) >= 1, geom
            # every layer of a step sees the per-GPU batch or a multiple of it (frames / views stacked on N), on a map no
            # larger than the input
            assert nhw[0] % shape[0] == 0 and nhw[1] <= shape[1] and nhw[2] <= shape[2], (body, shape, geom)
            assert PS.geom_from_json(PS.geom_to_json(geom)) == geom
        for rec in plans:
            assert rec[0] in ("fwd", "dgrad", "wgrad") and len(rec) == 13 and all(isinstance(v, int) for v in rec[1:]), rec


def test_no_geometry_repeats_or_is_a_bench_geometry():
    bench = set(BENCH_GEOMS)
    assert len(bench) == len(BENCH_GEOMS)
    for body in PS.BODIES:
        seen = {}
        for (b, shape), (geoms, _) in TABLE.items():
            if b != body:
                continue
            for geom in geoms:
                assert geom not in bench, (body, shape, "a bench step runs this geometry", geom)
                assert geom not in seen, (body, shape, "repeats", seen[geom], geom)
                seen[geom] = shape


ALL_GEOMS = sorted({g for geoms, _ in TABLE.values() for g in geoms}, key=str)


def test_every_geometry_meets_the_exactness_budget():
    """Amplitudes >= 1 with all three bounds inside fp32's exact integer range, written out here rather than read back
    from conv_exact.bounds: forward A_b + cin k^2 A_x A_w, input gradient cout k^2 A_g A_w, weight gradient
    N oh ow A_x A_g (the bias gradient, N oh ow A_g, is below it)."""
    assert X.LIMIT == 2 ** 24
    worst = {"fwd": 0, "dgrad": 0, "wgrad": 0}
    for geom in ALL_GEOMS:
        if geom[2][5] == X.ACT_SIGMOID_AFFINE:
            geom = X.with_act(geom, X.ACT_NONE)          # (the exact run of a sigmoid layer)
        amps, _ = X.budget(geom)                          # raises when even {-1, 0, 1} operands do not fit
        assert min(amps.values()) >= 1, (geom, amps)
        segs, cout, cfg, (n, h, w), _ = geom
        k = cfg[0]
        oh, ow = X.out_hw_of(geom)
        ax = max(X.seg_amps(segs, amps["x"]))
        assert 1 <= ax <= amps["x"]
        bd = {"fwd": amps["b"] + sum(segs) * k * k * ax * amps["w"], "dgrad": cout * k * k * amps["g"] * amps["w"],
              "wgrad": n * oh * ow * ax * amps["g"]}
        assert all(v <= 2 ** 24 for v in bd.values()), (geom, amps, bd)
        worst = {key: max(worst[key], bd[key]) for key in bd}
    print("%d geometries; largest bounds %s of %d" % (len(ALL_GEOMS), worst, 2 ** 24))


def test_largest_lattice_point_leaves_room():
    # 12 x 192 x 640: N oh ow = 1 474 560 terms per weight-gradient entry of a full-resolution layer: A_x A_g <= 11.
    # FeatExtractor runs the three frames of a sample as one batch of 36: 4 423 680 terms, A_x A_g <= 3.
    assert 12 * 192 * 640 == 1474560 and 11 * 1474560 <= 2 ** 24 < 12 * 1474560 and 3 * 3 * 1474560 <= 2 ** 24
    full = [g for g in TABLE[("cfg4", (12, 192, 640))][0] if X.out_hw_of(g) == (192, 640)]
    assert {g[3][0] for g in full} == {12, 36}, {g[3][0] for g in full}
    for geom in full:
        amps, _ = X.budget(X.with_act(geom, X.ACT_NONE))
        assert max(X.seg_amps(geom[0], amps["x"])) * amps["g"] * geom[3][0] * 192 * 640 <= 2 ** 24, (geom, amps)
