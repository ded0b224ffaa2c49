"""FlatAdam's bookkeeping (dvf/engine.py) without any network: six plain parameters, gradients fed by hand through
``p._dvf_grad.copy_(g); opt.grad_ready(p)``, compared per parameter and element with tests/adam_ref.py::FlatAdamRef (adam_ref64
carried over the steps in float64 from the same start, with FlatAdam's semantics: one global step counter, a parameter takes
part from its first gradient on).  Error budget (FlatAdamRef's docstring): moments k BOUND_M / k BOUND_V after k participations,
parameter sum of 0.5 ulp(p_j) + j BOUND_UPDATE |update_j|.

Gradients are fresh every step but keep their per-element sign, and the parameters start with that sign at magnitude U(0.5, 2):
no sum of the Adam formula cancels (weight decay included), so per-element relative error of the moments is well conditioned.

Arena layout of the six parameters (reverse registration order, 64-float padding), with 256-float buckets:
    bucket 0: (3,5,7) @ 0, (1000,) @ 128       bucket 1: (65,) @ 1152, (8,8) @ 1280, (63,) @ 1344       bucket 2: (1,) @ 1408
Parameter 2, (8,8), never receives a gradient: bucket 1 then has TWO touched ranges around it, and a step makes four launches of
which only the first may advance the step counter."""
import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1,), (63,), (8, 8), (65,), (1000,), (3, 5, 7)]
UNTOUCHED = 2
FED = [i for i in range(len(SHAPES)) if i != UNTOUCHED]
BUCKET_MB = 256 * 4 / 2 ** 20          # 256 floats
LR, BETAS, EPS = R.RECIPES[0]
STEPS = 4


def _sign(i):
    return np.sign(R.make_grad(int(np.prod(SHAPES[i])), seed=50 + i)).reshape(SHAPES[i])


def start_values():
    rng = np.random.default_rng(1)
    return [(_sign(i) * rng.uniform(0.5, 2.0, SHAPES[i])).astype(np.float32) for i in range(len(SHAPES))]


def grads_of(step, idxs=FED, wd=0.0):
    """Seeded gradients of one step with the parameter's fixed sign pattern; magnitudes 1e-6 .. 10 without weight decay.
    With weight decay gi = g + wd*p carries roundings that the measurement behind BOUND_M / BOUND_V (p = 0) does not contain, and
    a first step squares them into v' = (1-b2) gi^2.  The runs with weight decay therefore keep |g| in 0.1 .. 10: the decay term
    (wd |p| <= 0.02) is at most a sixth of gi, still 1e5 bounds large, and its rounding stays inside the bounds' factor 2."""
    lo = -1.0 if wd else -6.0
    return {i: (_sign(i) * np.abs(R.make_grad(int(np.prod(SHAPES[i])), seed=1000 * step + i, lo=lo)).reshape(SHAPES[i])
                ).astype(np.float32) for i in idxs}


def build(start, **kw):
    from dvf.engine import FlatAdam
    ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in start]
    kw.setdefault("lr", LR)
    kw.setdefault("bucket_mb", BUCKET_MB)
    opt = FlatAdam(ps, betas=BETAS, eps=EPS, **kw)
    assert len(opt.buckets) == 3
    return ps, opt


def feed(opt, ps, grads, order=None):
    """zero_grad, then the gradients 'arrive' in backward order (last parameter first) unless ``order`` says otherwise."""
    opt.zero_grad()
    for i in (order if order is not None else sorted(grads, reverse=True)):
        ps[i]._dvf_grad.copy_(torch.from_numpy(grads[i]).to(DEV))
        opt.grad_ready(ps[i])


def bits(t):
    return t.view(torch.int32)


def padding_mask(opt):
    mask = torch.ones(opt.total, dtype=torch.bool)
    for p in opt.params:
        mask[p._dvf_offset:p._dvf_offset + p.numel()] = False
    assert int(mask.sum()) == opt.total - sum(int(np.prod(s)) for s in SHAPES) > 0
    return mask


def check_layout(opt, ps):
    """p.data are views of flat_p at p._dvf_offset; every padding float of the four arenas is bit-zero."""
    for p, shape in zip(ps, SHAPES):
        assert tuple(p.data.shape) == shape and p._dvf_offset % 64 == 0
        assert p.data.data_ptr() == opt.flat_p.data_ptr() + 4 * p._dvf_offset
        assert p._dvf_grad.data_ptr() == opt.flat_g.data_ptr() + 4 * p._dvf_offset
    mask = padding_mask(opt)
    for name in ("flat_p", "flat_g", "flat_m", "flat_v"):
        assert not bool(bits(getattr(opt, name)).cpu()[mask].any()), name + " padding"


def check_against_ref(opt, ps, ref, frozen):
    """frozen: {index: (p, m, v) int32 bit patterns} of the parameters that have not taken part yet."""
    torch.cuda.synchronize()
    st = opt.opt_state.cpu().numpy()
    assert st[0] == ref.t, (st, ref.t)
    assert st[1] == np.float32(ref.lr)
    ss, bc = R.prep_ref(ref.t, ref.lr, BETAS)
    assert abs(float(st[2]) - ss) <= float(np.spacing(np.float32(ss))) and abs(float(st[3]) - bc) <= float(np.spacing(np.float32(bc)))
    for i, p in enumerate(ps):
        o, n = p._dvf_offset, p.numel()
        m, v = opt.flat_m[o:o + n].cpu().numpy(), opt.flat_v[o:o + n].cpu().numpy()
        if ref.count[i] == 0:
            for got, want in zip((p.data.cpu().numpy().ravel(), m, v), frozen[i]):
                assert np.array_equal(got.view(np.int32), want), ("a parameter without a gradient changed", i)
            assert p.grad is None
            continue
        k = ref.count[i]
        err = np.abs(p.data.cpu().numpy().astype(np.float64) - ref.p[i])
        assert np.all(err <= ref.budget[i]), (i, ref.t, float((err - ref.budget[i]).max()))
        assert R.rel_err_elem(m, ref.m[i].ravel()) <= k * R.BOUND_M, (i, ref.t)
        assert R.rel_err_elem(v, ref.v[i].ravel()) <= k * R.BOUND_V, (i, ref.t)
        assert p.grad is not None and p.grad.data_ptr() == p._dvf_grad.data_ptr()
    check_layout(opt, ps)


def seed_untouched_moments(opt, ps):
    """Non-zero moments under the parameter that never gets a gradient (as a loaded checkpoint could hold): an Adam launch that
    ran over it would decay them and move the parameter even with weight_decay = 0."""
    p = ps[UNTOUCHED]
    o, n = p._dvf_offset, p.numel()
    opt.flat_m[o:o + n].copy_(p.data.flatten() * 0.25)
    opt.flat_v[o:o + n].fill_(0.5)


def run_schedule(schedule, wd=0.0, lr_at=None, **kw):
    """schedule[k]: indices fed in step k+1.  lr_at: {step: lr} applied through set_lr before that step."""
    start = start_values()
    kw.setdefault("overlap", False)
    kw.setdefault("wgrad_stream", False)
    ps, opt = build(start, weight_decay=wd, **kw)
    seed_untouched_moments(opt, ps)
    torch.cuda.synchronize()
    frozen = {i: tuple(x.cpu().numpy().ravel().view(np.int32).copy()
                       for x in (p.data, opt.flat_m[p._dvf_offset:p._dvf_offset + p.numel()],
                                 opt.flat_v[p._dvf_offset:p._dvf_offset + p.numel()])) for i, p in enumerate(ps)}
    ref = R.FlatAdamRef(start, LR, BETAS, EPS, wd)
    check_layout(opt, ps)
    for k, idxs in enumerate(schedule, start=1):
        if lr_at and k in lr_at:
            opt.set_lr(lr_at[k])
            ref.lr = lr_at[k]
            assert opt.lr == lr_at[k]
            assert opt.opt_state[1].item() == float(np.float32(lr_at[k]))
        grads = grads_of(k, idxs, wd)
        feed(opt, ps, grads)
        opt.step()
        ref.step(grads)
        check_against_ref(opt, ps, ref, frozen)
    return ps, opt, ref


# ---------------------------------------------------------------------------------------------- a, b. basic run, weight decay
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_four_steps_against_reference(wd):
    """Five of six parameters get a gradient in each of four steps: parameters and moments follow the fp64 reference, the step
    counter advances ONCE per step although a step makes four launches in three buckets, the parameter without a gradient and its
    (non-zero) moments stay bit-unchanged, the padding stays zero."""
    ps, opt, ref = run_schedule([FED] * STEPS, wd=wd)
    assert len(opt._touched_ranges()) == 2
    assert sorted(len(opt._bucket_ranges(b)) for b in opt.buckets) == [1, 1, 2]
    assert ref.t == STEPS and ref.count[UNTOUCHED] == 0
    for i in FED:       # the parameters did move by about lr per step (the bounds above are far below that)
        moved = np.abs(ps[i].data.cpu().numpy() - start_values()[i])
        assert float(moved.max()) > LR


# ---------------------------------------------------------------------------------------------- c. early update
def test_early_update_is_bit_identical_to_late_update():
    """The default mode (overlap, early_update: buckets leave from inside grad_ready from step 2 on, on the update stream)
    against overlap=False (everything in step()): the arenas and opt_state are bit-identical after every step, also when one
    step's gradients arrive in another order (another bucket then makes the step's first launch)."""
    start = start_values()
    ps_e, early = build(start, weight_decay=1e-2)
    ps_l, late = build(start, weight_decay=1e-2, overlap=False, wgrad_stream=False)
    assert early.early_update and not late.early_update
    for k in range(1, STEPS + 1):
        grads = grads_of(k)
        order = sorted(grads) if k == 3 else None
        feed(early, ps_e, grads, order)
        feed(late, ps_l, grads, order)
        left_early = [b["updated"] for b in early.buckets]
        assert left_early == [k >= 2] * 3, (k, left_early)
        assert not any(b["updated"] for b in late.buckets)
        early.step()
        late.step()
        torch.cuda.synchronize()
        assert early.opt_state[0].item() == k
        for name in ("flat_p", "flat_m", "flat_v", "opt_state"):
            assert torch.equal(bits(getattr(early, name)), bits(getattr(late, name))), (k, name)
        check_layout(early, ps_e)


# ---------------------------------------------------------------------------------------------- d, e. who takes part
def test_parameter_without_gradient_in_a_later_step_is_updated_with_zero():
    """A parameter that received a gradient in step 1 and none in step 2 is updated in step 2 with g = 0 (its moments decay, it
    keeps moving): the gradient arena is zeroed and the parameter stays in the touched ranges.  This is torch.optim.Adam after
    ``zero_grad(set_to_none=False)``; pinned against the reference."""
    skip = 3
    ps, opt, ref = run_schedule([FED, [i for i in FED if i != skip], FED, FED])
    assert ref.count[skip] == STEPS


def test_parameter_first_touched_in_step_three_uses_the_global_step():
    """A parameter whose first gradient arrives in step 3 is updated with the GLOBAL t = 3 in its bias corrections (one device
    step counter for the arena); torch.optim.Adam would start that parameter's own counter at 1.  No step body of this project
    does this; the test pins the current behaviour (dvf/engine.py's module docstring states the difference)."""
    late = 4
    others = [i for i in FED if i != late]
    ps, opt, ref = run_schedule([others, others, FED, FED])
    assert ref.count[late] == 2 and ref.t == STEPS
    # the difference is not small: from a zero state the first update is step_size * bc2_sqrt * 0.1 / sqrt(0.001) -- lr exactly
    # with the parameter's own t = 1, about 0.64 lr with the global t = 3
    ss1, bc1 = R.prep_ref(1, LR, BETAS)
    ss3, bc3 = R.prep_ref(3, LR, BETAS)
    assert abs((ss3 * bc3) / (ss1 * bc1) - 1.0) > 1000 * R.BOUND_UPDATE


# ---------------------------------------------------------------------------------------------- f. set_lr
def test_set_lr_takes_effect_in_the_next_step():
    run_schedule([FED] * STEPS, wd=1e-2, lr_at={3: LR / 4})


def test_set_lr_reaches_a_captured_step():
    """A GraphedStep of zero_grad + feed from static tensors + step(): the learning rate is read from opt_state[1] on the device,
    so the replay after set_lr follows the new value."""
    from dvf.engine import GraphedStep
    start = start_values()
    ps, opt = build(start, weight_decay=1e-2, overlap=False, wgrad_stream=False)
    ref = R.FlatAdamRef(start, LR, BETAS, EPS, 1e-2)
    order = sorted(FED, reverse=True)
    to_dev = lambda grads: [torch.from_numpy(grads[i]).to(DEV) for i in order]       # noqa: E731
    g1 = grads_of(1, wd=1e-2)
    static = to_dev(g1)

    def fn(*inputs):
        opt.zero_grad()
        for i, g in zip(order, inputs):
            ps[i]._dvf_grad.copy_(g)
            opt.grad_ready(ps[i])
        opt.step()
        return (opt.opt_state,)

    runner = GraphedStep(fn, static, warmup=2)         # two eager steps with g1, then the capture (which does not execute)
    ref.step(g1)
    ref.step(g1)
    torch.cuda.synchronize()
    assert opt.opt_state[0].item() == 2
    for k, lr in ((3, None), (4, LR / 4), (5, None)):
        if lr is not None:
            opt.set_lr(lr)
            ref.lr = lr
        grads = grads_of(k, wd=1e-2)
        runner(*to_dev(grads))
        ref.step(grads)
        torch.cuda.synchronize()
        st = opt.opt_state.cpu().numpy()
        assert st[0] == k and st[1] == np.float32(ref.lr) and opt.lr == ref.lr
        for i in FED:
            err = np.abs(ps[i].data.cpu().numpy().astype(np.float64) - ref.p[i])
            assert np.all(err <= ref.budget[i]), (i, k)
        assert torch.equal(ps[UNTOUCHED].data.cpu(), torch.from_numpy(start[UNTOUCHED]))


# ---------------------------------------------------------------------------------------------- g. state_dict round trip
def test_state_dict_round_trip():
    """Two steps, save, two more steps; a fresh optimizer over fresh parameters holding the saved values, load_state_dict, the
    same two steps: bit-identical arenas.  The saved tensors are clones: the optimizer's later steps do not change them."""
    start = start_values()
    ps, opt = build(start, weight_decay=1e-2, overlap=False, wgrad_stream=False)
    for k in (1, 2):
        feed(opt, ps, grads_of(k))
        opt.step()
    torch.cuda.synchronize()
    sd = opt.state_dict()
    saved_p = opt.flat_p.clone()
    copies = {k: sd[k].clone() for k in ("opt_state", "exp_avg", "exp_avg_sq")}
    assert sd["opt_state"][0].item() == 2 and (sd["lr"], sd["betas"], sd["eps"], sd["weight_decay"]) == (LR, BETAS, EPS, 1e-2)
    assert float(sd["exp_avg"].abs().max()) > 0 and float(sd["exp_avg_sq"].abs().max()) > 0
    for k in (3, 4):
        feed(opt, ps, grads_of(k))
        opt.step()
    torch.cuda.synchronize()
    for k, c in copies.items():
        assert torch.equal(bits(sd[k]), bits(c)), k + " of the saved state changed with the optimizer"
    assert not torch.equal(opt.flat_m, sd["exp_avg"])

    resumed_start = [saved_p[p._dvf_offset:p._dvf_offset + p.numel()].view(s).cpu().numpy() for p, s in zip(ps, SHAPES)]
    ps2, opt2 = build(resumed_start, weight_decay=1e-2, overlap=False, wgrad_stream=False)
    assert torch.equal(bits(opt2.flat_p), bits(saved_p))
    opt2.load_state_dict(sd)
    for k in (3, 4):
        g = grads_of(k)
        # the resumed optimizer has not seen a gradient yet: every parameter that took part before the save is fed
        feed(opt2, ps2, g)
        opt2.step()
    torch.cuda.synchronize()
    for name in ("flat_p", "flat_m", "flat_v", "opt_state"):
        assert torch.equal(bits(getattr(opt, name)), bits(getattr(opt2, name))), name
