"""CPU tests of tests/adam_ref.py: the fp64 Adam reference is tied to torch.optim.Adam in double, the GPU bounds
(BOUND_UPDATE / BOUND_M / BOUND_V) are measured here from the float32 restatement of the kernel, and the same measurement
shows what those bounds can see (a 1e-5 effect such as beta2 = 0.999 instead of 0.999f, a dropped weight-decay term).
Run with ``pytest -s`` to print the measured figures that adam_ref.py records."""
import numpy as np
import pytest
import torch

import adam_ref as R

N = 1 << 18
LR, BETAS, EPS = R.RECIPES[0]


@pytest.fixture(scope="module")
def grad():
    return R.make_grad(N, seed=11)


def _errors(g, t, wd, gs, round_hyper, lr=LR):
    """Relative errors (update, m, v) of the float32 restatement against adam_ref64, one step from the seeded state, p = 0."""
    m, v = R.make_state(g, seed=13, t=t)
    p = np.zeros_like(g)
    out = R.adam_f32_restatement(p, g, m, v, t, lr, BETAS, EPS, wd, gs)
    ref = R.adam_ref64(p, g, m, v, t, lr, BETAS, EPS, wd, gs, round_hyper=round_hyper)
    assert np.array_equal(out[1], -out[0])            # p = 0: the stored parameter is minus the update
    return R.rel_err_elem(out[0], ref[0]), R.rel_err_elem(out[2], ref[2]), R.rel_err_elem(out[3], ref[3])


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_ref64_matches_torch_adam_in_double(wd):
    """adam_ref64(round_hyper=False) carried over 50 steps against torch.optim.Adam on float64 parameters with the same python
    doubles.  Gradients keep their sign over the steps and p has the sign of g, so nothing cancels."""
    n, steps = 4096, 50
    rng = np.random.default_rng(5)
    g0 = R.make_grad(n, seed=3).astype(np.float64)
    p0 = np.sign(g0) * rng.uniform(0.5, 2.0, n)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, amsgrad=False, foreach=False)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    worst = 0.0
    for t in range(1, steps + 1):
        g = g0 * rng.uniform(0.5, 2.0, n)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        _, p, m, v = R.adam_ref64(p, g, m, v, t, LR, BETAS, EPS, wd, 1.0, round_hyper=False)
        st = opt.state[tp]
        worst = max(worst, R.rel_err_elem(p, tp.detach().numpy()), R.rel_err_elem(m, st["exp_avg"].numpy()),
                    R.rel_err_elem(v, st["exp_avg_sq"].numpy()))
    print(f"\nadam_ref64 vs float64 torch.optim.Adam, wd={wd}: {worst:.2e}")
    assert worst <= 1e-12


def test_bound_measurement(grad):
    """The maximum error of the float32 restatement over the grid of the GPU test is within HALF of each BOUND_* constant (the
    bounds are twice what is measured here): change the inputs or the restatement and the constants cannot go stale silently."""
    worst = np.zeros(3)
    for lr, _betas, _eps in R.RECIPES:
        for t in R.T_GRID:
            for wd, gs in R.WD_GS_GRID:
                worst = np.maximum(worst, _errors(grad, t, wd, gs, True, lr=lr))
    print("\nrestatement vs adam_ref64(round_hyper=True): update %.3e  m %.3e  v %.3e" % tuple(worst))
    assert (R.BOUND_UPDATE, R.BOUND_M, R.BOUND_V) == (2 * R.MEASURED_UPDATE, 2 * R.MEASURED_M, 2 * R.MEASURED_V)
    assert worst[0] <= 0.5 * R.BOUND_UPDATE and worst[1] <= 0.5 * R.BOUND_M and worst[2] <= 0.5 * R.BOUND_V
    # ... and the constants are what was measured, not a comfortable multiple of it
    assert worst[0] >= 0.9 * R.MEASURED_UPDATE and worst[1] >= 0.9 * R.MEASURED_M and worst[2] >= 0.9 * R.MEASURED_V


def test_bounds_see_double_hyperparameters(grad):
    """Against the reference with UNROUNDED hyper-parameters (beta2 = 0.999, not 0.999f) the same restatement must exceed the
    bounds: the GPU test can see a 1e-5 effect."""
    upd = max(_errors(grad, t, 0.0, 1.0, False)[0] for t in (2, 3, 10, 100, 1000))
    v1 = _errors(grad, 1, 0.0, 1.0, False)[2]
    print(f"\nrestatement vs adam_ref64(round_hyper=False): update (t in 2..1000) {upd:.3e}  v (t=1) {v1:.3e}")
    assert upd > R.BOUND_UPDATE and v1 > R.BOUND_V
    assert 0.9 * R.MEASURED_DOUBLE_HYPER_UPDATE <= upd <= 1.1 * R.MEASURED_DOUBLE_HYPER_UPDATE
    assert 0.9 * R.MEASURED_DOUBLE_HYPER_V_T1 <= v1 <= 1.1 * R.MEASURED_DOUBLE_HYPER_V_T1


def test_distance_to_float32_torch_adam(grad):
    """Recorded, not required: one step of a float32 torch.optim.Adam from the same state lies several BOUND_UPDATE away from
    the reference the kernel is held to (adam_ref.py's module docstring); that is why it is not the reference."""
    worst = 0.0
    for t in (2, 3, 10, 100, 1000):
        m, v = R.make_state(grad, seed=13, t=t)
        tp = torch.nn.Parameter(torch.zeros(N))
        opt = torch.optim.Adam([tp], lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0, amsgrad=False, foreach=False)
        tp.grad = torch.from_numpy(grad.copy())
        opt.step()                                     # creates the state; overwritten below
        st = opt.state[tp]
        st["step"].fill_(t - 1)
        st["exp_avg"].copy_(torch.from_numpy(m))
        st["exp_avg_sq"].copy_(torch.from_numpy(v))
        with torch.no_grad():
            tp.zero_()
        opt.step()
        ref = R.adam_ref64(np.zeros_like(grad), grad, m, v, t, LR, BETAS, EPS, 0.0, 1.0)
        worst = max(worst, R.rel_err_elem(-tp.detach().numpy(), ref[0]))
    print(f"\nfloat32 torch.optim.Adam vs adam_ref64(round_hyper=True): update (t in 2..1000) {worst:.3e}")
    assert np.isfinite(worst)


def test_weight_decay_is_visible():
    """wd = 0.5 with p of order 1: dropping the term from the reference moves m' by far more than any bound."""
    p, g = R.make_wd_case(4096, seed=17)
    m, v = R.make_state(g, seed=19, t=10)
    with_wd = R.adam_ref64(p, g, m, v, 10, LR, BETAS, EPS, 0.5, 1.0)
    without = R.adam_ref64(p, g, m, v, 10, LR, BETAS, EPS, 0.0, 1.0)
    # t = 1 (zero state): m' = (1-b1) gi, so the change is the whole decay term
    z = np.zeros_like(g)
    d1 = R.rel_err_elem(R.adam_ref64(p, g, z, z, 1, LR, BETAS, EPS, 0.0, 1.0)[2], R.adam_ref64(p, g, z, z, 1, LR, BETAS, EPS, 0.5, 1.0)[2])
    d10 = float(np.max(np.abs(without[2] - with_wd[2]) / np.abs(with_wd[2])))
    print(f"\nm' without wd vs with wd = 0.5: t=1 {d1:.2f}  t=10 (max) {d10:.3f}")
    assert d1 > 0.1
    # and the restatement with wd stays within the GPU bounds of this case
    out = R.adam_f32_restatement(p, g, m, v, 10, LR, BETAS, EPS, 0.5, 1.0)
    assert R.rel_err_elem(out[2], with_wd[2]) <= R.BOUND_M and R.rel_err_elem(out[3], with_wd[3]) <= R.BOUND_V
    ulp = np.spacing(np.abs(out[1])).astype(np.float64)
    assert np.all(np.abs(out[1].astype(np.float64) - with_wd[1]) <= 0.5 * ulp + R.BOUND_UPDATE * np.abs(with_wd[0]))


@pytest.mark.parametrize("gs,wd", R.EXACT_GRID)
@pytest.mark.parametrize("fused", [False, True])
def test_exact_case_is_exact(gs, wd, fused):
    """exact_case's expected outputs equal the float32 restatement bit for bit, with every operation rounded and with the sums'
    products kept in float64 (a stand-in for FMA): no operation of the step rounds."""
    c = R.exact_case(5000, seed=23, grad_scale=gs, wd=wd)
    assert np.all(c["g"] != 0) and np.all(c["p"] != 0)
    _, p_new, m_new, v_new = R.adam_f32_restatement(c["p"], c["g"], c["m"], c["v"], 1, R.EXACT_LR, R.EXACT_BETAS, R.EXACT_EPS,
                                                    wd, gs, fused=fused)
    for key, got in (("p_new", p_new), ("m_new", m_new), ("v_new", v_new)):
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), c[key].view(np.int32)), key
    assert np.array_equal(np.abs(c["p_new"] - c["p"]), np.full(5000, R.EXACT_LR, np.float32))
    ss, bc = R.prep_ref(1, R.EXACT_LR, R.EXACT_BETAS)
    assert [1.0, R.EXACT_LR, ss, bc] == c["opt_state"].tolist()
    if wd:      # the decay term is wired in: without it a good part of the signs of gi (hence of the step) would differ
        other = R.exact_case(5000, seed=23, grad_scale=gs, wd=0.0)
        assert np.mean(np.sign(other["m_new"]) != np.sign(c["m_new"])) > 0.1
