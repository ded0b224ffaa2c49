"""References for the fused Adam kernel (csrc/elementwise.hip: adam_prep_kernel + adam_kernel) and for FlatAdam's
bookkeeping (dvf/engine.py).  Plain numpy; used by tests/test_adam_ref.py (CPU) and by tests/test_gpu_adam.py /
tests/test_gpu_flat_adam.py (GPU).

Why the reference is NOT a float32 torch.optim.Adam.  The C ABI receives lr, beta1, beta2, eps, weight_decay and
grad_scale as ``float`` and opt_state[1] stores lr as a float: the kernel is a self-consistent Adam whose beta2 is
0.999f = 0.99900001287...  A float32 torch.optim.Adam mixes three different beta2: 0.999f in ``mul_``, (float)(1 - 0.999)
in ``addcmul_`` and the double 0.999 in the bias correction.  Measured on a CPU (tests/test_adam_ref.py prints the figures
with ``pytest -s``), one step from a given (m, v) state, 2^18 elements, lr 1e-3, betas (0.9, 0.999), eps 1e-8:

    float32 restatement of the kernel  vs  adam_ref64(round_hyper=True)     update 3.35e-7   m 1.15e-7   v 1.17e-7
    the same                           vs  adam_ref64(round_hyper=False)    update 6.92e-6 (t in 2..1000), v 1.30e-5 (t = 1)
    float32 torch.optim.Adam           vs  adam_ref64(round_hyper=True)     update 6.95e-6 (t in 2..1000)   [TORCH_F32_DISTANCE]

The last line is a known and accepted difference, not a bug: it is the distance between two roundings of the
hyper-parameters, twenty times the kernel's own rounding error.  Over a trajectory, fp32 rounding of the STORED parameter
swamps both (an ulp of p ~ 0.1 is 7.5e-6 of lr = 1e-3).  The GPU tests therefore
  * compare single steps from a given state with the fp64 reference that uses the hyper-parameters as the ABI receives them,
  * observe the update through p = 0 (the stored parameter is then minus the update, at full fp32 relative precision),
  * pin the wiring of weight_decay and grad_scale bit-exactly with operands for which every operation is exact (exact_case).
"""
import numpy as np

# Measured by tests/test_adam_ref.py::test_bound_measurement: maximum per-element relative error of adam_f32_restatement against
# adam_ref64(round_hyper=True) over T_GRID x WD_GS_GRID x RECIPES, 2^18 elements, p = 0 (3.343e-7, 1.145e-7, 1.170e-7, rounded
# up).  That test fails if the restatement leaves them, or falls more than a tenth below them.
MEASURED_UPDATE = 3.35e-7
MEASURED_M = 1.15e-7
MEASURED_V = 1.17e-7
# The GPU bounds: twice the restatement's error.  The margin covers another association or FMA contraction in the compiled
# kernel (contraction only removes roundings).  2^-24 = 5.96e-8 is one rounding: the bounds are ~12, 4 and 4 roundings.
BOUND_UPDATE = 2.0 * MEASURED_UPDATE
BOUND_M = 2.0 * MEASURED_M
BOUND_V = 2.0 * MEASURED_V
# What the bounds can see (same test module): the restatement against round_hyper=False, and float32 torch.optim.Adam.
MEASURED_DOUBLE_HYPER_UPDATE = 6.92e-6     # max over t in 2..1000
MEASURED_DOUBLE_HYPER_V_T1 = 1.30e-5       # t = 1: (1 - 0.999f) / (1 - 0.999) - 1
TORCH_F32_DISTANCE = 6.95e-6               # float32 torch.optim.Adam, update, max over t in 2..1000

T_GRID = (1, 2, 3, 10, 100, 1000, 10000, 1000000)
WD_GS_GRID = ((0.0, 1.0), (1e-2, 0.125), (1e-8, 1.0))
RECIPES = ((1e-3, (0.9, 0.999), 1e-8), (2e-4, (0.9, 0.999), 1e-8))     # (lr, betas, eps) of the two training recipes

_f32 = np.float32


def round_f32(x):
    """A python double rounded to float32 and back: what a ``float`` argument of the C ABI carries."""
    return float(_f32(x))


def adam_ref64(p, g, m, v, t, lr, betas, eps, wd, grad_scale, round_hyper=True):
    """One step of torch's _single_tensor_adam (amsgrad off, L2-in-gradient weight decay) in float64.
    Returns (update, p_new, m_new, v_new) with p_new = p - update.  round_hyper: lr, betas, eps, wd and grad_scale are rounded to
    float32 first, as the C ABI (and opt_state[1] for lr) does."""
    b1, b2 = betas
    if round_hyper:
        lr, b1, b2, eps, wd, grad_scale = (round_f32(x) for x in (lr, b1, b2, eps, wd, grad_scale))
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    gi = g * grad_scale + wd * p
    m_new = b1 * m + (1.0 - b1) * gi
    v_new = b2 * v + (1.0 - b2) * gi * gi
    bc1, bc2 = 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)
    update = (lr / bc1) * m_new / (np.sqrt(v_new) / np.sqrt(bc2) + eps)
    return update, p - update, m_new, v_new


def prep_ref(t, lr, betas, round_hyper=True):
    """(step_size, bc2_sqrt) of adam_prep_kernel in double: lr / (1 - beta1^t), sqrt(1 - beta2^t)."""
    b1, b2 = betas
    if round_hyper:
        lr, b1, b2 = round_f32(lr), round_f32(b1), round_f32(b2)
    return lr / (1.0 - b1 ** float(t)), float(np.sqrt(1.0 - b2 ** float(t)))


def adam_f32_restatement(p, g, m, v, t, lr, betas, eps, wd, grad_scale, fused=False):
    """The kernel's arithmetic restated in numpy float32: same operation order, every operation rounded (no FMA).  The bias
    corrections are computed in double from the float hyper-parameters and rounded to float, as adam_prep_kernel does.
    Returns float32 (update, p_new, m_new, v_new).  It exists to MEASURE the GPU bounds on a CPU, not as a reference.
    fused=True: every ``a*x + b*y`` and the final ``p - s*q`` keep their products in float64 (exact: 24 x 24 bits) and round the
    sum once -- a stand-in for FMA contraction, used to show that exact_case does not depend on what the compiler fuses."""
    lr, b1, b2, eps, wd, gs = (_f32(x) for x in (lr, betas[0], betas[1], eps, wd, grad_scale))
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    tf = float(_f32(t))                                          # the step counter is a float in opt_state[0]
    step_size = _f32(float(lr) / (1.0 - float(b1) ** tf))
    bc2_sqrt = _f32(np.sqrt(1.0 - float(b2) ** tf))
    one = _f32(1.0)
    d = np.float64

    def axpby(a, x, b, y):
        if fused:
            return (d(a) * x.astype(d) + y.astype(d) * d(b)).astype(_f32)
        return a * x + b * y

    gi = g * gs
    if wd != 0:
        gi = (gi.astype(d) + d(wd) * p.astype(d)).astype(_f32) if fused else gi + wd * p
    m_new = axpby(b1, m, one - b1, gi)
    if fused:
        v_new = (d(b2) * v.astype(d) + ((one - b2) * gi).astype(d) * gi.astype(d)).astype(_f32)
    else:
        v_new = b2 * v + ((one - b2) * gi) * gi
    denom = np.sqrt(v_new) / bc2_sqrt + eps
    q = m_new / denom
    update = step_size * q
    p_new = (p.astype(d) - d(step_size) * q.astype(d)).astype(_f32) if fused else p - update
    return update, p_new, m_new, v_new


# ---------------------------------------------------------------------------------------------- seeded inputs
def make_grad(n, seed, lo=-6.0, hi=1.0):
    """float32 gradients with magnitudes spread log-uniformly over 10^lo .. 10^hi, random signs, no zeros."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(lo, hi, n)
    return (np.where(rng.random(n) < 0.5, -1.0, 1.0) * mag).astype(np.float32)


def make_state(g, seed, t):
    """float32 (m, v) that a run could have reached before step t: m = sign(g) U(0.1,4) |g|, v = U(0.1,4) g^2; zero for t = 1.
    m has the sign of g and v > 0, so no sum of the Adam formula cancels and per-element relative error is well conditioned."""
    g64 = np.asarray(g, dtype=np.float64)
    if t == 1:
        return np.zeros(g64.shape, np.float32), np.zeros(g64.shape, np.float32)
    rng = np.random.default_rng(seed + 7919)
    m = rng.uniform(0.1, 4.0, g64.shape) * g64
    v = rng.uniform(0.1, 4.0, g64.shape) * g64 * g64
    return m.astype(np.float32), v.astype(np.float32)


def make_wd_case(n, seed):
    """The weight-decay inputs: |g| ~ 1 (U(0.5,2), random sign), p = sign(g) U(0.5,2), so that with wd = 0.5 the decay term is
    a third to two thirds of gi and nothing cancels.  Returns float32 (p, g)."""
    rng = np.random.default_rng(seed)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = sign * rng.uniform(0.5, 2.0, n)
    p = sign * rng.uniform(0.5, 2.0, n)
    return p.astype(np.float32), g.astype(np.float32)


def rel_err_elem(out, ref):
    """max over elements of |out - ref| / |ref| (ref must have no zeros)."""
    out, ref = np.asarray(out, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.all(ref != 0)
    return float(np.max(np.abs(out - ref) / np.abs(ref)))


EXACT_LR, EXACT_BETAS, EXACT_EPS = 2.0 ** -7, (0.5, 0.75), 0.0
EXACT_GRID = tuple((gs, wd) for gs in (1.0, 0.5, 0.25) for wd in (0.0, 0.5))


def exact_case(n, seed, grad_scale=1.0, wd=0.0):
    """Operands for which ONE Adam step is exact in float32, whatever the compiler fuses or reassociates.
    betas (0.5, 0.75), eps 0, t = 1, lr = 2^-7, zero moments; grad_scale in {1, 0.5, 0.25}, wd in {0, 0.5}; g = a/8 and p = b/8
    with integers 1 <= |a|, |b| <= 63.  Then gi = g*gs + wd*p = K/32 with the integer K = a*4gs + 2b*[wd] (|K| <= 378: 9 bits;
    b's sign is flipped where K would be 0), and
        m' = gi/2,  v' = gi^2/4 (K^2 < 2^18),  step_size = lr/(1-0.5) = 2 lr,  bc2_sqrt = sqrt(1-0.75) = 0.5,
        denom = sqrt(v')/0.5 + 0 = |gi|,  m'/denom = sign(gi)/2,  p' = p - lr sign(gi)
    are all exact: no operation rounds, so FMA contraction or another association cannot change a bit.  This rests on sqrtf and
    '/' being correctly rounded, which is hipcc's default with this project's flags (no fast-math option in csrc/Makefile).
    Returns a dict: float32 p, g, m, v (inputs), p_new, m_new, v_new (expected, computed in integers / float64 and cast) and the
    expected opt_state [1, lr, 2 lr, 0.5]."""
    assert (grad_scale, wd) in EXACT_GRID
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 64, n) * np.where(rng.random(n) < 0.5, -1, 1)
    b = rng.integers(1, 64, n) * np.where(rng.random(n) < 0.5, -1, 1)
    ca, cb = int(4 * grad_scale), (2 if wd else 0)
    b = np.where(a * ca + b * cb == 0, -b, b)
    k = a * ca + b * cb                                # gi = k / 32
    assert np.all(k != 0) and int(np.abs(k).max()) < 4096
    gi = k.astype(np.float64) / 32.0
    p = b.astype(np.float64) / 8.0
    exact = {"p": p, "g": a.astype(np.float64) / 8.0, "m": np.zeros(n), "v": np.zeros(n),
             "p_new": p - EXACT_LR * np.sign(gi), "m_new": gi / 2.0, "v_new": (k * k).astype(np.float64) / 4096.0}
    out = {key: val.astype(np.float32) for key, val in exact.items()}
    for key, val in exact.items():                     # operands and expected values are float32 numbers: the cast did not round
        assert np.array_equal(out[key].astype(np.float64), val), key
    out["opt_state"] = np.array([1.0, EXACT_LR, 2.0 * EXACT_LR, 0.5], np.float32)
    return out


# ---------------------------------------------------------------------------------------------- FlatAdam bookkeeping
class FlatAdamRef:
    """fp64 model of FlatAdam's semantics over a list of parameters: ONE global step counter; a parameter takes part from the
    first step it receives a gradient in, and from then on in every step (with g = 0 when it receives none: the gradient arena
    is zeroed, which is torch.optim.Adam after ``zero_grad(set_to_none=False)``).  A parameter that first takes part in step
    k > 1 is updated with the GLOBAL t = k (torch.optim.Adam would start its own counter at 1).
    It also carries the error budget of the fp32 arenas against this model, per parameter and element:
        moments after k participations: k * BOUND_M, k * BOUND_V (relative);
        parameter: sum over its steps j = 1..k of 0.5 ulp(p_j) + j * BOUND_UPDATE |update_j|.  The update of step j is computed
        from moments that already carry (j-1) (BOUND_M, BOUND_V): its relative error is at most
        BOUND_UPDATE + (j-1) (BOUND_M + BOUND_V / 2) <= j BOUND_UPDATE; the 0.5 ulp is the rounding of the stored parameter."""

    def __init__(self, params, lr, betas, eps, wd, grad_scale=1.0):
        self.p = [np.asarray(a, dtype=np.float64).copy() for a in params]
        self.m = [np.zeros_like(a) for a in self.p]
        self.v = [np.zeros_like(a) for a in self.p]
        self.lr, self.betas, self.eps, self.wd, self.gs = lr, betas, eps, wd, grad_scale
        self.t = 0
        self.count = [0] * len(self.p)                 # participations so far
        self.budget = [np.zeros_like(a) for a in self.p]

    def step(self, grads):
        """grads: {parameter index: float32 array} of the parameters that receive a gradient in this step."""
        self.t += 1
        for i in range(len(self.p)):
            if i not in grads and self.count[i] == 0:
                continue
            g = np.asarray(grads[i], dtype=np.float64).reshape(self.p[i].shape) if i in grads else np.zeros_like(self.p[i])
            upd, self.p[i], self.m[i], self.v[i] = adam_ref64(self.p[i], g, self.m[i], self.v[i], self.t, self.lr, self.betas,
                                                              self.eps, self.wd, self.gs)
            self.count[i] += 1
            ulp = np.spacing(np.abs(self.p[i]).astype(np.float32)).astype(np.float64)
            self.budget[i] += 0.5 * ulp + self.count[i] * BOUND_UPDATE * np.abs(upd)
