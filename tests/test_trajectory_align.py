"""The numpy definition of trajectory alignment and of the errors of an aligned trajectory (odometry_eval.py:
trajectory_alignment, apply_alignment, trajectory_errors, snippet_errors), pinned by known answers, and the input conditions
under which tests/test_gpu_trajectory_align.py compares the device code with it at 1e-9.  No GPU here."""
import math

import numpy as np
import pytest

import align_ref as A
import odometry_eval as oe
import odometry_ref as R

CONDITION_SIZES = (1500, 800, 257, 60, 5, 3)


def _ate(gt, res, mode):
    c, rot, t, sv = oe.trajectory_alignment(gt, res, mode)
    return c, rot, sv, oe.trajectory_errors(gt, oe.apply_alignment(res, c, rot, t))[0]


def test_similarity_is_recovered_by_7dof_and_not_by_6dof():
    gt, res = A.similar()
    c, rot, sv, ate = _ate(gt, res, "7dof")
    print(f"7dof: c - 1.7 = {c - 1.7:.3e}, ATE {ate:.3e}")
    assert abs(c - 1.7) < 1e-12 and ate < 1e-9
    assert np.abs(rot - R._euler(*A.SIMILARITY[1]).T).max() < 1e-12
    c6, _, _, ate6 = _ate(gt, res, "6dof")
    assert c6 == 1.0 and ate6 > 10.0                                   # a 1.7x smaller path cannot be laid onto the other
    c7, rot7, _, _ = _ate(gt, res, "scale_7dof")
    assert c7 == c and np.array_equal(rot7, np.eye(3))
    assert oe.trajectory_alignment(gt, res, "none")[0] == 1.0
    with pytest.raises(ValueError):
        oe.trajectory_alignment(gt, res, "sim3")
    with pytest.raises(ValueError):
        oe.trajectory_alignment(gt[:2], res[:2], "6dof")


def test_scale_about_the_origin():
    gt, res = R.straight(400, 1.0), R.straight(400, 1.1)
    c, rot, sv, ate = _ate(gt, res, "scale")
    assert abs(c - 1.0 / 1.1) < 1e-15 and np.array_equal(rot, np.eye(3)) and np.all(sv == 0.0)
    assert ate < 1e-12
    assert oe.trajectory_alignment(gt, A.zero_translations(res), "scale")[0] == 1.0      # 0 / 0: the scale stays 1


def test_apply_alignment_maps_rotation_and_translation():
    gt, res = A.pair(60)
    rot, t = R._euler(0.2, 0.1, -0.3), np.array([1.0, 2.0, 3.0])
    out = oe.apply_alignment(res, 2.0, rot, t)
    assert out.shape == res.shape
    for i in (0, 17, 59):
        assert np.allclose(out[i, :3, :3], rot @ res[i, :3, :3], rtol=0, atol=1e-15)
        assert np.allclose(out[i, :3, 3], 2.0 * rot @ res[i, :3, 3] + t, rtol=0, atol=1e-12)
    assert np.array_equal(oe.apply_alignment(res[:, :3], 1.0, np.eye(3), np.zeros(3)), res[:, :3])


@pytest.mark.parametrize("n", A.MIRROR_SIZES)
def test_mirrored_input_takes_the_reflection_branch_and_stays_a_rotation(n):
    gt, res = A.pair(n)
    res = A.mirrored(res)
    x, y = res[:, :3, 3], gt[:, :3, 3]
    U, sv, Vt = np.linalg.svd((y - y.mean(0)).T @ (x - x.mean(0)) / n)
    assert np.linalg.det(U) * np.linalg.det(Vt) < 0                    # the branch S = diag(1, 1, -1)
    c, rot, t, sv = oe.trajectory_alignment(gt, res, "7dof")
    assert abs(np.linalg.det(rot) - 1.0) < 1e-12 and np.abs(rot @ rot.T - np.eye(3)).max() < 1e-12
    assert (sv[1] - sv[2]) / sv[0] >= A.CONDITION
    assert abs(c - (sv[0] + sv[1] - sv[2]) / ((x - x.mean(0)) ** 2).sum() * n) < 1e-12 * c


def test_trajectory_errors_known_answers():
    gt, res = R.error_case("identical")
    assert oe.trajectory_errors(gt, res) == (0.0, 0.0, 0.0)
    gt, res = R.error_case("yaw")                                      # res_i = rot_y(YAW i) gt_i: every pair turns by YAW
    ate, rpe_t, rpe_r = oe.trajectory_errors(gt, res)
    assert abs(rpe_r - R.YAW) < 1e-15
    gt, res = R.error_case("scale")                                    # 1.0 m against 1.1 m steps
    ate, rpe_t, rpe_r = oe.trajectory_errors(gt, res)
    assert abs(rpe_t - 0.1) < 1e-12 and rpe_r == 0.0
    assert abs(ate - 0.1 * math.sqrt(np.mean(np.arange(400.0) ** 2))) < 1e-9
    ate, rpe_t, rpe_r = oe.trajectory_errors(gt[:1], res[:1])
    assert ate == 0.0 and math.isnan(rpe_t) and math.isnan(rpe_r)


def test_snippet_errors_known_answers():
    gt, res = R.error_case("scale")
    rows = oe.snippet_errors(gt, res)
    assert rows.shape == (396, 2) and np.abs(rows).max() < 1e-12       # the snippet's own scale removes the factor 1.1
    gt, res = R.error_case("yaw")
    rows = oe.snippet_errors(gt, res)
    # re-based to its first frame, frame k of a snippet is turned by YAW k: (0 + 1 + 2 + 3 + 4) YAW / 5 = 0.004 rad
    assert rows.shape == (296, 2) and np.abs(rows[:, 1] - 0.004).max() < 1e-12
    assert oe.snippet_errors(gt[:4], res[:4]).shape == (0, 2)
    assert oe.snippet_errors(gt[:5], res[:5]).shape == (1, 2)
    for length in (1, 9):
        with pytest.raises(ValueError):
            oe.snippet_errors(gt, res, length)
    # a row IS compute_pose_error of the re-based, scaled snippet
    gt, res = A.pair(60)
    row = oe.snippet_errors(gt, res, 5)[7]
    g = np.linalg.inv(gt[7]) @ gt[7:12]
    p = np.linalg.inv(res[7]) @ res[7:12]
    p[:, :3, 3] *= (g[:, :3, 3] * p[:, :3, 3]).sum() / (p[:, :3, 3] ** 2).sum()
    assert tuple(row) == tuple(oe.compute_pose_error(g[:, :3], p[:, :3]))


def _conditions():
    worst = {"plain": math.inf, "mirrored": math.inf}
    for n in sorted(set(CONDITION_SIZES + A.ALIGN_SIZES)):
        gt, res = A.pair(n)
        sv = oe.trajectory_alignment(gt, res, "7dof")[3]
        worst["plain"] = min(worst["plain"], (sv[1] + sv[2]) / sv[0])
    for n in A.MIRROR_SIZES:
        gt, res = A.pair(n)
        sv = oe.trajectory_alignment(gt, A.mirrored(res), "7dof")[3]
        worst["mirrored"] = min(worst["mirrored"], (sv[1] - sv[2]) / sv[0])
    gt, res = A.shifted(A.pair(1500)[0]), A.shifted(A.pair(1500)[1])
    sv = oe.trajectory_alignment(gt, res, "7dof")[3]
    worst["plain"] = min(worst["plain"], (sv[1] + sv[2]) / sv[0])
    return worst


def test_input_conditions_of_the_gpu_alignment_cases():
    worst = _conditions()
    print(f"(sv1 + sv2) / sv0 >= {worst['plain']:.3e}; mirrored (sv1 - sv2) / sv0 >= {worst['mirrored']:.3e}")
    assert worst["plain"] >= A.CONDITION and worst["mirrored"] >= A.CONDITION


def test_end_to_end_ground_truth_is_not_collinear():
    gt = A.end_to_end_gt()
    y = gt[:, :3, 3] - gt[:, :3, 3].mean(0)
    sv = np.linalg.svd(y, compute_uv=False)
    assert gt.shape == (20, 4, 4) and sv[1] / sv[0] > 0.05                # (an arc: two directions fix the rotation)
    assert oe.trajectory_distances(R.as_dict(gt))[-1] == pytest.approx(19 * 12.0, abs=1e-9)
    line = R.end_to_end_gt()[:, :3, 3]                                   # the straight line it stands in for: rank 1
    assert np.linalg.svd(line - line.mean(0), compute_uv=False)[1] == 0.0


def test_input_conditions_of_the_gpu_angle_cases():
    """Every angle compared relatively is >= 1e-4 rad: the per-pair RPE angles, and in a snippet row the sum of its frames'
    angles (re * length; the first frame of a re-based snippet is the identity on both sides)."""
    worst = math.inf
    for n in sorted(set(A.ERROR_SIZES + A.SNIPPET_SIZES)):
        gt, res = A.pair(n)
        worst = min(worst, float(A.pair_angles(gt, res).min()))
        for length in A.SNIPPET_LENGTHS:
            rows = oe.snippet_errors(gt, res, length)
            if len(rows):
                worst = min(worst, float(rows[:, 1].min()) * length)
    print(f"smallest angle compared relatively: {worst:.3e} rad")
    assert worst >= A.MIN_ANGLE


def test_input_conditions_of_the_gpu_snippet_ate_columns():
    """A two-frame snippet of (curved, drifted) holds one step, and the drifted step is the curved one times 1.03: after the
    snippet's own scale its ate is 0 up to rounding, so the GPU test bounds that column absolutely (1e-12).  From three frames
    on the drift turns the later steps and the largest ate of a case, which conftest.rel_err divides by, is far above rounding."""
    zero, floor = 0.0, math.inf
    for n in A.SNIPPET_SIZES:
        gt, res = A.pair(n)
        zero = max(zero, float(oe.snippet_errors(gt, res, 2)[:, 0].max()))
        for length in (5, 8):
            rows = oe.snippet_errors(gt, res, length)
            if len(rows):
                floor = min(floor, float(rows[:, 0].max()))
    print(f"length 2: max ate {zero:.3e}; length 5, 8: the largest ate of a case >= {floor:.3e}")
    assert zero < 1e-12 and floor > 1e-5


def test_large_offset_moves_the_two_pass_definition_by_rounding_only():
    gt, res = A.pair(1500)
    c = oe.trajectory_alignment(gt, res, "7dof")[0]
    c_off = oe.trajectory_alignment(A.shifted(gt), A.shifted(res), "7dof")[0]
    x, y = A.shifted(res)[:, :3, 3], A.shifted(gt)[:, :3, 3]
    n = len(x)
    mx, my = x.mean(0), y.mean(0)
    sig = y.T @ x / n - np.outer(my, mx)                               # the one-pass moment form the definition rules out
    var = (x * x).sum() / n - mx @ mx
    U, d, Vt = np.linalg.svd(sig)
    one_pass = (d[0] + d[1] + math.copysign(d[2], np.linalg.det(U) * np.linalg.det(Vt))) / var
    print(f"c moves by {abs(c_off - c) / c:.3e} (two passes), {abs(one_pass - c) / c:.3e} (one pass)")
    assert abs(c_off - c) < 1e-12 * c
    assert abs(one_pass - c) > 1e-9 * c                                # the GPU test at 1e-9 tells the two apart


def test_horn_quaternion_solver_agrees_with_the_svd_definition():
    worst_r = worst_c = 0.0
    cases = [A.pair(n) for n in sorted(set(CONDITION_SIZES + A.ALIGN_SIZES))]
    cases += [(A.pair(n)[0], A.mirrored(A.pair(n)[1])) for n in A.MIRROR_SIZES] + [A.similar()]
    for gt, res in cases:
        c, rot, _, _ = oe.trajectory_alignment(gt, res, "7dof")
        hc, hrot = A.horn(gt, res)
        worst_r = max(worst_r, float(np.abs(hrot - rot).max()))
        worst_c = max(worst_c, abs(hc - c) / c)
    print(f"Horn against SVD: R {worst_r:.3e}, c {worst_c:.3e}")
    assert worst_r < 1e-12 and worst_c < 1e-12
