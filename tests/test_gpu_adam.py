"""dvf_adam_step (csrc/elementwise.hip: adam_prep_kernel + adam_kernel) element by element.

Reference: tests/adam_ref.py::adam_ref64, torch's _single_tensor_adam in float64 with the hyper-parameters rounded to float as
the C ABI receives them; single steps from a given state, the update observed through p = 0.  Every tolerance is one of
adam_ref's BOUND_* constants (twice the error of the kernel's float32 restatement, measured in tests/test_adam_ref.py) or an ulp
expression; the wiring of weight_decay / grad_scale is pinned bit-exactly (adam_ref.exact_case).

The kernel is called on slices of larger buffers, at element offsets 0 and 1 (the C ABI states no alignment contract), with 64
sentinel floats on each side.  After every call: the guards of p, m and v, the whole g buffer and opt_state[1] (lr) are
bit-unchanged."""
import functools

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENTINEL = -0x21524111                 # 0xDEADBEEF as int32: a finite float (-6.26e18) that no test value equals
GRID_STRIDE_N = 4096 * 256 + 257       # one element more than a full grid of 4096 blocks x 256 threads, plus an odd tail
SIZES = (1, 63, 64, 65, 255, 256, 257, GRID_STRIDE_N)
INVALID_ARG = -1                       # DVF_ERR_INVALID_ARG (include/dvf_hip.h)


def _bits(t):
    return t.view(torch.int32)


class Arena:
    """p, g, m, v: device buffers of GUARD + offset + n + GUARD floats filled with the sentinel, the operands in the middle."""

    def __init__(self, n, offset, p, g, m, v):
        self.n, self.lo = n, GUARD + offset
        self.buf = {}
        for name, host in (("p", p), ("g", g), ("m", m), ("v", v)):
            host = np.array(host, dtype=np.float32)         # a copy: the cached inputs are read-only
            assert host.shape == (n,)
            full = torch.full((self.lo + n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
            full[self.lo:self.lo + n].copy_(torch.from_numpy(host))
            self.buf[name] = full
        self.g_before = self.buf["g"].clone()

    def view(self, name, start=0, count=None):
        count = self.n - start if count is None else count
        assert 0 <= start and count >= 1 and start + count <= self.n
        return self.buf[name][self.lo + start:self.lo + start + count]

    def host(self, name):
        return self.view(name).cpu().numpy()

    def check_untouched(self):
        for name in ("p", "m", "v"):
            b = _bits(self.buf[name])
            assert bool((b[:self.lo] == SENTINEL).all()) and bool((b[self.lo + self.n:] == SENTINEL).all()), name + " guard"
        assert torch.equal(_bits(self.buf["g"]), _bits(self.g_before)), "g was written"


def make_state(t, lr):
    return torch.tensor([float(t), lr, 0.0, 0.0], dtype=torch.float32, device=DEV)


def adam_step(a, state, advance, betas, eps, wd, gs, start=0, count=None):
    """One dvf_adam_step on elements [start, start + count) of the arena; checks the guards, g and lr afterwards."""
    from dvf import lib as L
    count = a.n - start if count is None else count
    views = [a.view(k, start, count) for k in ("p", "g", "m", "v")]
    assert all(x.numel() == count for x in views) and state.numel() == 4
    lr_bits = _bits(state)[1].item()
    L.check(L.lib().dvf_adam_step(L.dev(views[0]), L.dev(views[1]), L.dev(views[2]), L.dev(views[3]), count, L.dev(state),
                                  advance, betas[0], betas[1], eps, wd, gs, L.stream()), "dvf_adam_step")
    torch.cuda.synchronize()
    a.check_untouched()
    assert _bits(state)[1].item() == lr_bits, "opt_state[1] (lr) was written"


def assert_rel(out, ref, bound, what):
    err = R.rel_err_elem(out, ref)
    print(f"{what}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (what, err, bound)


def assert_no_new_nonfinite(a, refs):
    for name, ref in zip(("p", "m", "v"), refs):
        assert np.all(np.isfinite(ref)), "the reference itself is not finite"
        assert np.all(np.isfinite(a.host(name))), name + " has NaN or Inf where the reference has none"


@functools.lru_cache(maxsize=None)
def _inputs(n, t):
    """(g, m, v) of the single-step cases, computed once per (n, t == 1) and never modified."""
    g = R.make_grad(n, seed=101 + n % 1000)
    m, v = R.make_state(g, seed=202, t=t)
    for x in (g, m, v):
        x.setflags(write=False)
    return g, m, v


# ---------------------------------------------------------------------------------------------- a. bit-exact step
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_exact_step(n, offset):
    """Operands for which nothing rounds (adam_ref.exact_case): p', m', v' and opt_state are bit-exact, at every size and
    alignment, for every grad_scale and weight_decay of the case."""
    for gs, wd in R.EXACT_GRID:
        c = R.exact_case(n, seed=n + 31 * offset, grad_scale=gs, wd=wd)
        a = Arena(n, offset, c["p"], c["g"], c["m"], c["v"])
        state = make_state(0, R.EXACT_LR)
        adam_step(a, state, 1, R.EXACT_BETAS, R.EXACT_EPS, wd, gs)
        assert torch.equal(state.cpu(), torch.from_numpy(c["opt_state"])), (gs, wd, state)
        for name, key in (("p", "p_new"), ("m", "m_new"), ("v", "v_new")):
            assert torch.equal(a.view(name).cpu(), torch.from_numpy(c[key])), (name, gs, wd)


# ---------------------------------------------------------------------------------------------- b. single step from a state
@pytest.mark.parametrize("n", [65, GRID_STRIDE_N])
@pytest.mark.parametrize("t", R.T_GRID)
def test_single_step_from_state(t, n):
    """Step t entered by writing t-1 into opt_state[0]; p = 0, so the parameter read back is minus the update."""
    g, m, v = _inputs(n, 1 if t == 1 else 2)
    zeros = np.zeros(n, np.float32)
    for lr, betas, eps in R.RECIPES:
        ss, bc = R.prep_ref(t, lr, betas)
        for wd, gs in R.WD_GS_GRID:
            a = Arena(n, 1, zeros, g, m, v)
            state = make_state(t - 1, lr)
            adam_step(a, state, 1, betas, eps, wd, gs)
            st = state.cpu().numpy()
            assert st[0] == t
            assert abs(float(st[2]) - ss) <= float(np.spacing(np.float32(ss))), (st[2], ss)      # 1 ulp of the double value
            assert abs(float(st[3]) - bc) <= float(np.spacing(np.float32(bc))), (st[3], bc)
            upd, _, m_ref, v_ref = R.adam_ref64(zeros, g, m, v, t, lr, betas, eps, wd, gs)
            tag = f"t={t} n={n} lr={lr} wd={wd} gs={gs}"
            assert_rel(-a.host("p").astype(np.float64), upd, R.BOUND_UPDATE, "update " + tag)
            assert_rel(a.host("m"), m_ref, R.BOUND_M, "m " + tag)
            assert_rel(a.host("v"), v_ref, R.BOUND_V, "v " + tag)


# ---------------------------------------------------------------------------------------------- c. weight decay, stored parameter
@pytest.mark.parametrize("n", [65, GRID_STRIDE_N])
def test_weight_decay_and_stored_parameter(n):
    """wd = 0.5 with p of order 1 (the decay term is a third to two thirds of gi).  The stored parameter adds one rounding of
    p' itself: |p' - p_ref| <= 0.5 ulp(p') + BOUND_UPDATE |update|."""
    lr, betas, eps = R.RECIPES[0]
    p, g = R.make_wd_case(n, seed=17)
    m, v = R.make_state(g, seed=19, t=10)
    a = Arena(n, 1, p, g, m, v)
    state = make_state(9, lr)
    adam_step(a, state, 1, betas, eps, 0.5, 1.0)
    upd, p_ref, m_ref, v_ref = R.adam_ref64(p, g, m, v, 10, lr, betas, eps, 0.5, 1.0)
    assert_rel(a.host("m"), m_ref, R.BOUND_M, "m")
    assert_rel(a.host("v"), v_ref, R.BOUND_V, "v")
    p_new = a.host("p")
    ulp = np.spacing(np.abs(p_new)).astype(np.float64)
    excess = np.abs(p_new.astype(np.float64) - p_ref) - (0.5 * ulp + R.BOUND_UPDATE * np.abs(upd))
    assert float(excess.max()) <= 0.0, float(excess.max())
    assert np.all(p_new != p)


# ---------------------------------------------------------------------------------------------- d. advance_step = 0
def test_second_range_does_not_advance():
    """FlatAdam launches once per contiguous range: only the first launch of a step advances the counter.  A second call with
    advance_step = 0 leaves opt_state bit-unchanged and computes what ONE call over both ranges computes."""
    lr, betas, eps = R.RECIPES[0]
    n1, n2 = 321, 200
    n = n1 + n2
    g = R.make_grad(n, seed=5)
    m, v = R.make_state(g, seed=6, t=3)
    p = np.sign(g) * np.abs(R.make_grad(n, seed=7, lo=-1.0, hi=0.0))       # the sign of g: gi = g*gs + wd*p does not cancel
    split, whole = Arena(n, 0, p, g, m, v), Arena(n, 0, p, g, m, v)
    s_split, s_whole = make_state(2, lr), make_state(2, lr)
    adam_step(split, s_split, 1, betas, eps, 1e-2, 0.5, start=0, count=n1)
    after_first = s_split.clone()
    assert after_first[0].item() == 3
    assert torch.equal(split.view("p", n1), torch.from_numpy(p[n1:]).to(DEV)), "the first call went past its range"
    adam_step(split, s_split, 0, betas, eps, 1e-2, 0.5, start=n1, count=n2)
    assert torch.equal(_bits(s_split), _bits(after_first))
    adam_step(whole, s_whole, 1, betas, eps, 1e-2, 0.5)
    assert torch.equal(_bits(s_split), _bits(s_whole))
    for name in ("p", "m", "v"):
        assert torch.equal(split.buf[name], whole.buf[name]), name
    # and the pair is a real step 3, not step 4 on the second range
    upd, p_ref, _, _ = R.adam_ref64(p, g, m, v, 3, lr, betas, eps, 1e-2, 0.5)
    ulp = np.spacing(np.abs(split.host("p"))).astype(np.float64)
    assert np.all(np.abs(split.host("p").astype(np.float64) - p_ref) <= 0.5 * ulp + R.BOUND_UPDATE * np.abs(upd))


# ---------------------------------------------------------------------------------------------- e. edge values
def test_zero_gradient_zero_state_is_a_no_op():
    """g = 0, m = v = 0, eps = 1e-8: denom = eps, update = step_size * (0 / eps) = 0 exactly; p stays bit-unchanged (a parameter
    of a touched range that received no gradient yet must not move or turn into NaN through 0/0)."""
    lr, betas, eps = R.RECIPES[0]
    n = 257
    p = R.make_grad(n, seed=9, lo=-3.0, hi=1.0)
    z = np.zeros(n, np.float32)
    a = Arena(n, 1, p, z, z, z)
    adam_step(a, make_state(0, lr), 1, betas, eps, 0.0, 1.0)
    assert np.array_equal(a.host("p").view(np.int32), p.view(np.int32))
    assert not a.host("m").any() and not a.host("v").any()


def test_zero_gradient_with_state():
    """g = 0 with a non-zero state: the moments decay (m' = b1 m, v' = b2 v) and the parameter keeps moving."""
    lr, betas, eps = R.RECIPES[0]
    n, t = 257, 10
    m, v = R.make_state(R.make_grad(n, seed=10), seed=11, t=t)
    z = np.zeros(n, np.float32)
    a = Arena(n, 1, z, z, m, v)
    adam_step(a, make_state(t - 1, lr), 1, betas, eps, 0.0, 1.0)
    upd, p_ref, m_ref, v_ref = R.adam_ref64(z, z, m, v, t, lr, betas, eps, 0.0, 1.0)
    assert_no_new_nonfinite(a, (p_ref, m_ref, v_ref))
    assert_rel(-a.host("p").astype(np.float64), upd, R.BOUND_UPDATE, "update")
    assert_rel(a.host("m"), m_ref, R.BOUND_M, "m")
    assert_rel(a.host("v"), v_ref, R.BOUND_V, "v")


@pytest.mark.parametrize("t", [1, 10])
def test_tiny_gradient_denormal_second_moment(t):
    """|g| = 1e-20: g^2 = 1e-40 is below the smallest normal float (1.18e-38); v' is a DENORMAL (about 1e-43 at t = 1, up to
    4e-40 at t = 10).  Expectation, derived from the kernel's arithmetic under IEEE float32 with gradual underflow:
      * m' ~ 1e-21 is normal: BOUND_M holds;
      * v' lies on the denormal grid of spacing q = 2^-149.  (1-b2)*gi ~ 1e-23 is normal (relative rounding, inside BOUND_V);
        b2*v and ((1-b2)*gi)*gi each round to the grid (<= q/2 each) and their sum is exact there (both are multiples of q):
        |v' - v_ref| <= q + BOUND_V |v_ref| (q/2 would do at t = 1, where v = 0);
      * sqrt(v')/bc2_sqrt <= 1e-19 vanishes against eps = 1e-8: denom = eps to 1e-11, so the update = step_size m'/eps does not
        depend on v' at all and BOUND_UPDATE holds, flushed or not.
    A device that flushed denormals to zero would give v' = 0 here and fail the second point."""
    lr, betas, eps = R.RECIPES[0]
    n = 257
    g = (np.sign(R.make_grad(n, seed=12)) * 1e-20).astype(np.float32)
    m, v = R.make_state(g, seed=13, t=t)
    z = np.zeros(n, np.float32)
    a = Arena(n, 1, z, g, m, v)
    adam_step(a, make_state(t - 1, lr), 1, betas, eps, 0.0, 1.0)
    upd, p_ref, m_ref, v_ref = R.adam_ref64(z, g, m, v, t, lr, betas, eps, 0.0, 1.0)
    assert_no_new_nonfinite(a, (p_ref, m_ref, v_ref))
    assert_rel(-a.host("p").astype(np.float64), upd, R.BOUND_UPDATE, "update")
    assert_rel(a.host("m"), m_ref, R.BOUND_M, "m")
    quantum = float(np.spacing(np.float32(0.0)))                  # 2^-149
    v_dev = a.host("v").astype(np.float64)
    print("v' on the device:", v_dev[:4], "reference:", v_ref[:4])
    assert np.all(v_dev > 0), "v' was flushed to zero"
    assert np.all(np.abs(v_dev - v_ref) <= quantum + R.BOUND_V * np.abs(v_ref))


def test_huge_gradient():
    """|g| = 1e18: g^2 = 1e36 and v <= 4e36 are finite in float32 (max 3.4e38); the ordinary bounds hold and nothing overflows."""
    lr, betas, eps = R.RECIPES[0]
    n, t = 257, 10
    g = (np.sign(R.make_grad(n, seed=14)) * 1e18).astype(np.float32)
    m, v = R.make_state(g, seed=15, t=t)
    z = np.zeros(n, np.float32)
    a = Arena(n, 1, z, g, m, v)
    adam_step(a, make_state(t - 1, lr), 1, betas, eps, 0.0, 1.0)
    upd, p_ref, m_ref, v_ref = R.adam_ref64(z, g, m, v, t, lr, betas, eps, 0.0, 1.0)
    assert_no_new_nonfinite(a, (p_ref, m_ref, v_ref))
    assert_rel(-a.host("p").astype(np.float64), upd, R.BOUND_UPDATE, "update")
    assert_rel(a.host("m"), m_ref, R.BOUND_M, "m")
    assert_rel(a.host("v"), v_ref, R.BOUND_V, "v")


# ---------------------------------------------------------------------------------------------- f. argument checks
def test_invalid_arguments_launch_nothing():
    from dvf import lib as L
    lr, betas, eps = R.RECIPES[0]
    n = 65
    g = R.make_grad(n, seed=16)
    m, v = R.make_state(g, seed=17, t=2)
    a = Arena(n, 0, g, g, m, v)
    before = {k: b.clone() for k, b in a.buf.items()}
    state = make_state(1, lr)
    state_before = state.clone()
    ptr = {k: L.dev(a.view(k)) for k in ("p", "g", "m", "v")}
    st = L.dev(state)

    def call(p, gr, n_, s):
        return L.lib().dvf_adam_step(p, gr, ptr["m"], ptr["v"], n_, s, 1, betas[0], betas[1], eps, 0.0, 1.0, L.stream())

    assert call(None, ptr["g"], n, st) == INVALID_ARG
    assert call(ptr["p"], None, n, st) == INVALID_ARG
    assert call(ptr["p"], ptr["g"], n, None) == INVALID_ARG
    assert call(ptr["p"], ptr["g"], 0, st) == INVALID_ARG
    torch.cuda.synchronize()
    assert torch.equal(_bits(state), _bits(state_before))
    for k, b in a.buf.items():
        assert torch.equal(_bits(b), _bits(before[k])), k


# ---------------------------------------------------------------------------------------------- g. graph replay
def test_graph_replay_follows_device_state():
    """opt_state lives in device memory so that a captured step replays correctly: three replays of ONE captured call equal
    three eager calls bit for bit (the step counter advances inside the graph), and a learning rate written into opt_state[1]
    between replays is the one the next replay uses."""
    lr, betas, eps = R.RECIPES[0]
    n, wd, gs = 257, 1e-2, 0.5
    g = R.make_grad(n, seed=18)
    p = R.make_grad(n, seed=19, lo=-1.0, hi=0.0)
    z = np.zeros(n, np.float32)
    warm = Arena(n, 1, p, g, z, z)
    adam_step(warm, make_state(0, lr), 1, betas, eps, wd, gs)        # the kernels are loaded before the capture
    graphed, eager = Arena(n, 1, p, g, z, z), Arena(n, 1, p, g, z, z)
    s_graph, s_eager = make_state(0, lr), make_state(0, lr)
    from dvf import lib as L
    views = [graphed.view(k) for k in ("p", "g", "m", "v")]
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        L.check(L.lib().dvf_adam_step(L.dev(views[0]), L.dev(views[1]), L.dev(views[2]), L.dev(views[3]), n, L.dev(s_graph), 1,
                                      betas[0], betas[1], eps, wd, gs, L.stream()), "dvf_adam_step")
    torch.cuda.synchronize()
    assert s_graph[0].item() == 0, "the capture pass must not execute"

    def compare(step):
        torch.cuda.synchronize()
        graphed.check_untouched()
        assert s_graph[0].item() == step
        assert torch.equal(_bits(s_graph), _bits(s_eager)), (step, s_graph, s_eager)
        for k in ("p", "m", "v"):
            assert torch.equal(_bits(graphed.buf[k]), _bits(eager.buf[k])), (step, k)

    for step in (1, 2, 3):
        graph.replay()
        adam_step(eager, s_eager, 1, betas, eps, wd, gs)
        compare(step)
    p3 = graphed.host("p")
    s_graph[1:2].fill_(lr / 2)
    s_eager[1:2].fill_(lr / 2)
    graph.replay()
    adam_step(eager, s_eager, 1, betas, eps, wd, gs)
    compare(4)
    assert np.all(graphed.host("p") != p3)
    assert abs(float(s_graph[2].item()) - R.prep_ref(4, lr / 2, betas)[0]) <= float(np.spacing(np.float32(lr)))
