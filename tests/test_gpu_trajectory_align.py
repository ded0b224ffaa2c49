"""dvf.odometry.align / trajectory_errors / snippet_errors (dvf_trajectory_align, dvf_trajectory_apply, dvf_trajectory_errors,
dvf_snippet_errors) on the GPU against the numpy definition (odometry_eval.py: trajectory_alignment, apply_alignment,
trajectory_errors, snippet_errors; inputs from tests/align_ref.py).

Bound: conftest.rel_err < 1e-9 unless stated.  It is derived: fp64 sums over n <= 4541 frames and the polar factor of a 3x3
matrix whose conditioning tests/test_trajectory_align.py asserts ((sv1 +- sv2) / sv0 >= 5e-4) err by about 1e-13, an fp32 slip
by about 1e-5; angles compared relatively are >= 1e-4 rad (asserted there as well), where the atan2 form loses nothing.  Every
case runs twice and the two results are compared bit for bit; every case prints its figure (pytest -s).
Measured worst values over the cases of this file: transform record c 1.7e-15, R 9.4e-15 (2.1e-14 on mirrored input), sv
2.1e-15, t 3.0e-12 (a difference of two ~100 m means), aligned poses 2.0e-15; c under the (3e5, 0, 5.7e6) m offset 9.0e-16;
ate 1.5e-16, rpe_trans 1.8e-13, rpe_rot 1.7e-14; snippet re 5.4e-13, snippet ate 1.2e-10 (n = 1500, length 5: the definition's
own inv(first) @ each subtracts two ~1e3 m translations, rounded at 1e-13 m, for a row of ~1e-3 m; 1.6e-11 at n = 256);
summary mean / std / mean angle 6.0e-13 / 1.3e-12 / 3.6e-14; the ~0 columns stay below 1e-13 (bound 1e-12, absolute)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import align_ref as A
import odometry_eval as oe
import odometry_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-9
ZERO = 1e-12          # absolute bound of a column that is ~0 in the definition


def _bits(x):
    return x.contiguous().view(torch.int64)


def _dev(traj):
    return torch.from_numpy(np.array(np.asarray(traj)[:, :3, :4], dtype=np.float64)).to(DEV)      # (a writable copy)


def _twice(fn):
    """fn() -> tuple of tensors, run twice: asserts bit equality, returns the first result as numpy arrays."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.dtype == torch.float64 and _bits(x).equal(_bits(y)), "a second run differs"
    return [x.cpu().numpy() for x in a]


def _align(gt, res, mode):
    from dvf.odometry import align
    g, r = _dev(gt), _dev(res)
    return _twice(lambda: align(g, r, mode))


def _record(transform):
    return transform[0], transform[1:10].reshape(3, 3), transform[10:13], transform[13:16]


def _check_alignment(gt, res, mode, tag):
    aligned, transform = _align(gt, res, mode)
    c, rot, t, sv = _record(transform)
    wc, wrot, wt, wsv = oe.trajectory_alignment(gt, res, mode)
    want = oe.apply_alignment(np.asarray(res)[:, :3], wc, wrot, wt)
    assert aligned.shape == want.shape and np.all(np.isfinite(transform))
    errs = {"c": abs(c - wc) / abs(wc), "R": rel_err(rot, wrot), "sv": rel_err(sv, wsv), "aligned": rel_err(aligned, want)}
    if np.any(wt != 0.0):
        errs["t"] = rel_err(t, wt)
    else:
        assert np.all(t == 0.0)
    print(f"{tag} {mode}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < TOL, (tag, mode, k, v)
    assert abs(np.linalg.det(rot) - 1.0) < 1e-12 and np.abs(rot @ rot.T - np.eye(3)).max() < 1e-12      # never a reflection
    if mode == "none":
        assert np.array_equal(aligned, np.asarray(res)[:, :3]) and c == 1.0                              # a copy
    if mode in ("none", "scale", "scale_7dof"):
        assert np.array_equal(rot, np.eye(3)) and np.all(t == 0.0)
    if mode in ("none", "scale"):
        assert np.all(sv == 0.0)
    if mode == "6dof":
        assert c == 1.0
    return errs


@pytest.mark.parametrize("n", A.ALIGN_SIZES)
def test_alignment_all_modes(n):
    gt, res = A.pair(n)
    for mode in oe.ALIGN_MODES:
        _check_alignment(gt, res, mode, f"n={n}")


@pytest.mark.parametrize("n", A.MIRROR_SIZES)
def test_alignment_of_mirrored_input_is_a_rotation(n):
    gt, res = A.pair(n)
    for mode in ("6dof", "7dof", "scale_7dof"):
        _check_alignment(gt, A.mirrored(res), mode, f"mirrored n={n}")


def test_similarity_is_recovered():
    gt, res = A.similar()
    aligned, transform = _align(gt, res, "7dof")
    ate = oe.trajectory_errors(gt, aligned)[0]
    print(f"similarity: c - 1.7 = {transform[0] - 1.7:.3e}, ATE {ate:.3e}")
    assert abs(transform[0] - 1.7) < 1e-12 and ate < 1e-9


def test_large_common_offset_needs_the_second_pass():
    gt, res = A.pair(1500)
    gt, res = A.shifted(gt), A.shifted(res)
    _, transform = _align(gt, res, "7dof")
    want = oe.trajectory_alignment(gt, res, "7dof")[0]
    err = abs(transform[0] - want) / want
    print(f"offset {A.OFFSET}: c rel_err {err:.3e}")
    assert err < TOL                                    # (a one-pass moment formula is off by 3e-7 here: test_trajectory_align.py)


def test_straight_line_gives_a_finite_proper_rotation():
    gt, res = R.straight(400, 1.0), R.straight(400, 1.1)
    aligned, transform = _align(gt, res, "7dof")
    c, rot, t, sv = _record(transform)
    assert np.all(np.isfinite(transform))
    assert abs(np.linalg.det(rot) - 1.0) < 1e-12 and np.abs(rot @ rot.T - np.eye(3)).max() < 1e-12
    assert sv[0] > 0.0 and sv[1] == 0.0 and sv[2] == 0.0
    ate = oe.trajectory_errors(gt, aligned)[0]
    print(f"straight line: c {c!r}, aligned ATE {ate:.3e}")
    assert ate < 1e-9 * 399.0


def test_zero_translations_keep_scale_one():
    gt, res = A.pair(60)
    aligned, transform = _align(gt, A.zero_translations(res), "scale")
    assert transform[0] == 1.0 and np.all(aligned[:, :, 3] == 0.0)


def _errors(gt, res):
    from dvf.odometry import trajectory_errors
    g, r = _dev(gt), _dev(res)
    return _twice(lambda: (trajectory_errors(g, r),))[0]


def _error_cases():
    return [(f"n={n}", A.pair(n)) for n in A.ERROR_SIZES] + [("aligned n=1500", A.aligned_pair(1500))]


@pytest.mark.parametrize("case", range(len(A.ERROR_SIZES) + 1))
def test_ate_and_rpe(case):
    tag, (gt, res) = _error_cases()[case]
    got = _errors(gt, res)
    want = oe.trajectory_errors(gt, res)
    assert got[3] == len(gt)
    for name, g, w in zip(("ate", "rpe_trans", "rpe_rot"), got, want):
        err = abs(g - w) / abs(w)
        print(f"{tag}: {name} {g!r} rel_err {err:.3e}")
        assert err < TOL, (tag, name, g, w)


def test_ate_and_rpe_of_identical_trajectories_are_zero_and_one_frame_has_no_pair():
    gt, res = R.error_case("identical")
    got = _errors(gt, res)
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 0.0 and got[3] == 1200
    gt, res = A.pair(3)
    got = _errors(gt[:1], res[:1])
    assert got[0] == 0.0 and math.isnan(got[1]) and math.isnan(got[2]) and got[3] == 1


def _snippets(gt, res, length, summary=None):
    from dvf.odometry import snippet_errors
    g, r = _dev(gt), _dev(res)
    if summary is None:
        return _twice(lambda: snippet_errors(g, r, length))
    return snippet_errors(g, r, length, summary)


def _check_summary(summary, rows, tag, zero_ate=False):
    """summary [5] against numpy's mean / population std / mean of the definition's rows; ``zero_ate``: the ate column is ~0 in
    the definition, its two figures get the absolute bound ZERO."""
    assert summary[3] == len(rows) and summary[4] == 0.0
    k = summary[3]
    mean, std, re = summary[0] / k, math.sqrt(max(summary[1] / k - (summary[0] / k) ** 2, 0.0)), summary[2] / k
    for name, g, w in zip(("mean ate", "std ate", "mean re"), (mean, std, re), A.snippet_stats(rows)):
        if zero_ate and name != "mean re":
            print(f"{tag}: {name} {g:.3e} (definition {w:.3e})")
            assert abs(g) < ZERO and abs(w) < ZERO, (tag, name, g, w)
            continue
        # (the std of a single row is 0 on both sides)
        err = abs(g - w) / abs(w) if w != 0.0 else abs(g)
        print(f"{tag}: {name} rel_err {err:.3e}")
        assert err < TOL, (tag, name, g, w)


@pytest.mark.parametrize("n", A.SNIPPET_SIZES)
def test_snippets(n):
    gt, res = A.pair(n)
    for length in A.SNIPPET_LENGTHS:
        rows, summary = _snippets(gt, res, length)
        want = oe.snippet_errors(gt, res, length)
        assert rows.shape == want.shape == (max(n - length + 1, 0), 2)
        if len(want) == 0:
            assert np.all(summary == 0.0)
            continue
        # A two-frame snippet holds ONE step, and a step of the drifted walk is the curved walk's times 1.03: the snippet's own
        # scale removes the factor and the ate column is 0 up to rounding on both sides (asserted on the definition alone in
        # tests/test_trajectory_align.py), so it gets the absolute bound of the other ~0 columns, not a relative one.
        zero_ate = length == 2
        for col, name in ((0, "ate"), (1, "re")):
            if zero_ate and col == 0:
                print(f"n={n} length={length}: max |ate| {np.abs(rows[:, 0]).max():.3e} (definition {np.abs(want[:, 0]).max():.3e})")
                assert np.abs(rows[:, 0]).max() < ZERO and np.abs(want[:, 0]).max() < ZERO
                continue
            err = rel_err(rows[:, col], want[:, col])
            print(f"n={n} length={length}: {name} rel_err {err:.3e}")
            assert err < TOL, (n, length, name, err)
        _check_summary(summary, want, f"n={n} length={length}", zero_ate)


def test_snippets_accumulate_over_two_sequences():
    from dvf.odometry import snippet_errors
    a, b = A.pair(1500), A.pair(800, 12)

    def both():
        _, summary = snippet_errors(_dev(a[0]), _dev(a[1]), 5)
        _, same = snippet_errors(_dev(b[0]), _dev(b[1]), 5, summary)
        assert same is summary
        return (summary,)
    summary = _twice(both)[0]
    pooled = np.concatenate([oe.snippet_errors(*a), oe.snippet_errors(*b)])
    _check_summary(summary, pooled, "accumulated")


def test_snippets_of_a_short_sequence_and_of_a_scaled_straight_line():
    gt, res = A.pair(5)
    rows, summary = _snippets(gt[:4], res[:4], 5)
    assert rows.shape == (0, 2) and np.all(summary == 0.0)
    gt, res = R.error_case("scale")
    rows, summary = _snippets(gt, res, 5)
    print(f"scaled straight line: max |ate| {np.abs(rows[:, 0]).max():.3e}, max |re| {np.abs(rows[:, 1]).max():.3e}")
    assert rows.shape == (396, 2) and np.abs(rows).max() < 1e-12 and summary[3] == 396     # ~0 columns: an absolute bound
    assert abs(summary[0]) / 396 < 1e-12 and abs(summary[2]) / 396 < 1e-12
    gt, res = R.error_case("yaw")
    rows, _ = _snippets(gt, res, 5)
    assert np.abs(rows[:, 1] - 0.004).max() < 1e-12


def test_python_errors_before_any_launch():
    from dvf.odometry import align, snippet_errors, trajectory_errors
    gt, res = A.pair(60)
    g, r = _dev(gt), _dev(res)
    for fn in (lambda a, b: align(a, b, "7dof"), trajectory_errors, snippet_errors):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(g.cpu(), r)
        with pytest.raises(TypeError):
            fn(g, r.float())
        with pytest.raises(ValueError):
            fn(g, r[:59])
    with pytest.raises(ValueError):
        align(g, r, "sim3")
    with pytest.raises(ValueError):
        snippet_errors(g, r, 9)
    with pytest.raises(ValueError):
        snippet_errors(g, r, 1)
    with pytest.raises(ValueError):
        align(g[:2].contiguous(), r[:2].contiguous(), "6dof")
    align(g[:2].contiguous(), r[:2].contiguous(), "scale")             # two frames carry a scale
    torch.cuda.synchronize()


def test_c_entries_reject_short_scratch_unknown_modes_and_lengths():
    from dvf import lib as L
    lib = L.lib()
    n = 300
    gt, res = A.pair(n)
    g, r = _dev(gt), _dev(res)
    out = torch.zeros(16, device=DEV, dtype=torch.float64)
    rows = torch.zeros(n, 2, device=DEV, dtype=torch.float64)
    ws = torch.zeros(64, device=DEV, dtype=torch.float64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                         # noqa: E731
    need = lib.dvf_trajectory_align_ws_doubles(n)
    assert need == 2 * 18 and lib.dvf_trajectory_errors_ws_doubles(n) == 6 and lib.dvf_snippet_errors_ws_doubles(n) == 6
    assert lib.dvf_trajectory_align_ws_doubles(0) == 0
    assert lib.dvf_trajectory_align(p(g), p(r), n, 4, p(out), p(ws), need - 1, None) != 0
    assert lib.dvf_trajectory_errors(p(g), p(r), n, p(out), p(ws), 5, None) != 0
    assert lib.dvf_snippet_errors(p(g), p(r), n, 5, p(rows), p(out), 0, p(ws), 5, None) != 0
    assert lib.dvf_trajectory_align(p(g), p(r), n, 5, p(out), p(ws), 64, None) != 0       # unknown mode
    assert lib.dvf_trajectory_align(p(g), p(r), n, -1, p(out), p(ws), 64, None) != 0
    assert lib.dvf_trajectory_align(p(g), p(r), 2, 3, p(out), p(ws), 64, None) != 0       # 6dof needs three frames
    assert lib.dvf_trajectory_align(p(g), p(r), 0, 1, p(out), p(ws), 64, None) != 0
    assert lib.dvf_trajectory_apply(p(r), p(out), 0, 0, p(rows), None) != 0
    assert lib.dvf_trajectory_errors(p(g), p(r), 0, p(out), p(ws), 64, None) != 0
    assert lib.dvf_snippet_errors(p(g), p(r), n, 9, p(rows), p(out), 0, p(ws), 64, None) != 0
    assert lib.dvf_snippet_errors(p(g), p(r), n, 1, p(rows), p(out), 0, p(ws), 64, None) != 0
    assert lib.dvf_snippet_errors(p(g), p(r), 0, 5, p(rows), p(out), 0, p(ws), 64, None) != 0
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and float(rows.abs().sum()) == 0.0      # nothing was launched
