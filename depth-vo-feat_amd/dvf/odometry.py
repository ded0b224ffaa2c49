"""Odometry evaluation on the device (csrc/odometry.hip, ``dvf_pose_chain`` / ``dvf_odometry_errors`` of include/dvf_hip.h):
the chained camera-to-world trajectory of relative poses and the KITTI segment errors against ground truth, in fp64.

The definition is odometry_eval.py's numpy ``se3_cam2world`` / ``sequence_errors`` / ``overall_error`` for dense trajectories
(frame i = row i of both).  ``align`` / ``trajectory_errors`` / ``snippet_errors`` (``dvf_trajectory_*`` / ``dvf_snippet_errors``)
bring the chained trajectory onto the ground truth (scale, 6-DoF, 7-DoF) and score it with ATE, RPE and the scale-aligned
snippet errors of inference.py:72-88; their definition is odometry_eval.py's trajectory_alignment / apply_alignment /
trajectory_errors / snippet_errors.  Nothing here synchronises; every result is ordered on the current stream."""
import torch

# (ALIGN_MODES: index = DVF_ALIGN_* of include/dvf_hip.h)
from odometry_eval import ALIGN_MODES, FIRST_FRAME, FRAME_STEP, SEGMENT_LENGTHS
from . import lib as L

SNIPPET_LENGTHS = (2, 8)                                           # inclusive


def _dev64(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the HIP path needs a CUDA/HIP tensor, got {t.device}; there is no CPU fallback")
    if t.dtype != torch.float64:
        raise TypeError(f"{name}: expected float64, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    return t.data_ptr()


def n_starts(n):
    """Number of start frames 9, 19, ... below n."""
    return len(range(FIRST_FRAME, n, FRAME_STEP))


def chain_poses(rel, offsets=None):
    """Camera-to-world poses [N+S,3,4] fp64 of the relative poses ``rel`` [N,4,4] fp32 on the device: per sequence the
    identity, then T_k = T_{k-1} @ rel_k.  ``offsets`` (host ints, S+1 of them, offsets[0] = 0, non-decreasing, offsets[S] = N;
    default one sequence) splits ``rel`` into S <= 32 sequences; sequence s starts at row offsets[s] + s of the result."""
    L.dev(rel, "rel")
    if rel.dim() != 3 or tuple(rel.shape[1:]) != (4, 4):
        raise ValueError(f"chain_poses: rel must be [N,4,4], got {tuple(rel.shape)}")
    N = rel.shape[0]
    offsets = [0, N] if offsets is None else [int(o) for o in offsets]
    S = len(offsets) - 1
    if S < 1 or offsets[-1] != N:
        raise ValueError(f"chain_poses: offsets must hold S + 1 >= 2 entries ending at N = {N}, got {offsets}")
    world = torch.empty(N + S, 3, 4, device=rel.device, dtype=torch.float64)
    src = rel if N > 0 else torch.empty(16, device=rel.device, dtype=torch.float32)    # an empty tensor has no address
    L.check(L.lib().dvf_pose_chain(src.data_ptr(), L.int_array(offsets), S, world.data_ptr(), L.stream()), "dvf_pose_chain")
    return world


def _pair(gt, res, what, n_min=1):
    """The checks every (gt, res) entry shares, before any launch; returns n."""
    _dev64(gt, "gt")
    _dev64(res, "res")
    if gt.dim() != 3 or tuple(gt.shape[1:]) != (3, 4) or gt.shape != res.shape or gt.shape[0] < n_min:
        raise ValueError(f"{what}: gt and res must be [n,3,4] of one size, n >= {n_min}, got {tuple(gt.shape)} and "
                         f"{tuple(res.shape)}")
    return gt.shape[0]


def sequence_errors(gt, res, summary=None):
    """KITTI segment errors of the trajectory ``res`` against ``gt``, both [n,3,4] fp64 on the device.  Returns (rows,
    summary): rows [n_starts(n)*8, 6] = [first, r_err/len, t_err/len, len, speed, valid] (start-major, lengths ascending,
    all zero where the segment does not end inside the sequence) and summary [4] = [sum t_err/len, sum r_err/len, valid
    rows, path length of gt].  A ``summary`` passed in has the first three added to it in place (several sequences, one
    pass)."""
    n = _pair(gt, res, "sequence_errors")
    accumulate = summary is not None
    if accumulate:
        _dev64(summary, "summary")
        if summary.numel() != 4:
            raise ValueError("sequence_errors: summary must hold 4 doubles")
    else:
        summary = torch.empty(4, device=gt.device, dtype=torch.float64)
    rows = torch.empty(n_starts(n) * len(SEGMENT_LENGTHS), 6, device=gt.device, dtype=torch.float64)
    m = int(L.lib().dvf_odometry_errors_ws_doubles(n))
    ws = L.workspace(("dvf_odometry_errors", n), m, torch.float64, gt.device)
    L.check(L.lib().dvf_odometry_errors(gt.data_ptr(), res.data_ptr(), n, rows.data_ptr() if rows.numel() else None,
                                        summary.data_ptr(), int(accumulate), ws.data_ptr(), m, L.stream()), "dvf_odometry_errors")
    return rows, summary


def align(gt, res, mode):
    """The trajectory ``res`` brought onto ``gt`` (both [n,3,4] fp64 on the device, dense, not re-based) by ``mode`` out of
    ALIGN_MODES: none, scale (least squares about the origin), 6dof (rigid), 7dof (similarity, Umeyama) or scale_7dof (the
    scale of 7dof alone); the fit reads the translations only.  Returns (aligned [n,3,4], transform [16] = c, R[9], t[3],
    sv[3]): pose [R_i | t_i] becomes [R R_i | c R t_i + t], sv are the singular values of the cross-covariance (a straight line
    has sv[1] = sv[2] = 0 and no unique rotation).  Definition: odometry_eval.trajectory_alignment / apply_alignment."""
    if mode not in ALIGN_MODES:
        raise ValueError(f"align: mode must be one of {ALIGN_MODES}, got {mode!r}")
    m = ALIGN_MODES.index(mode)
    n = _pair(gt, res, f"align ({mode})", 3 if m >= 2 else 1)
    transform = torch.empty(16, device=gt.device, dtype=torch.float64)
    aligned = torch.empty_like(res)
    size = int(L.lib().dvf_trajectory_align_ws_doubles(n))
    ws = L.workspace(("dvf_trajectory_align", n), size, torch.float64, gt.device)
    L.check(L.lib().dvf_trajectory_align(gt.data_ptr(), res.data_ptr(), n, m, transform.data_ptr(), ws.data_ptr(), size, L.stream()),
            "dvf_trajectory_align")
    L.check(L.lib().dvf_trajectory_apply(res.data_ptr(), transform.data_ptr(), n, int(m == 0), aligned.data_ptr(), L.stream()),
            "dvf_trajectory_apply")
    return aligned, transform


def trajectory_errors(gt, res):
    """[4] = [ate, rpe_trans, rpe_rot (radians), n] of the trajectory ``res`` against ``gt`` as they come (align first), both
    [n,3,4] fp64 on the device; NaN for the two RPE values when n = 1.  Definition: odometry_eval.trajectory_errors."""
    n = _pair(gt, res, "trajectory_errors")
    out = torch.empty(4, device=gt.device, dtype=torch.float64)
    size = int(L.lib().dvf_trajectory_errors_ws_doubles(n))
    ws = L.workspace(("dvf_trajectory_errors", n), size, torch.float64, gt.device)
    L.check(L.lib().dvf_trajectory_errors(gt.data_ptr(), res.data_ptr(), n, out.data_ptr(), ws.data_ptr(), size, L.stream()),
            "dvf_trajectory_errors")
    return out


def snippet_errors(gt, res, length=5, summary=None):
    """The scale-aligned snippet errors of inference.py:72-88 over every ``length``-frame window of the trajectories (both
    [n,3,4] fp64 on the device).  Returns (rows [max(n - length + 1, 0), 2] = [ate, re (radians)], summary [5] = [sum ate,
    sum ate^2, sum re, rows, 0]).  A ``summary`` passed in has the first four added to it in place.  Definition:
    odometry_eval.snippet_errors."""
    if not SNIPPET_LENGTHS[0] <= length <= SNIPPET_LENGTHS[1]:
        raise ValueError(f"snippet_errors: length must be within {SNIPPET_LENGTHS[0]}..{SNIPPET_LENGTHS[1]}, got {length}")
    n = _pair(gt, res, "snippet_errors")
    accumulate = summary is not None
    if accumulate:
        _dev64(summary, "summary")
        if summary.numel() != 5:
            raise ValueError("snippet_errors: summary must hold 5 doubles")
    else:
        summary = torch.empty(5, device=gt.device, dtype=torch.float64)
    rows = torch.empty(max(n - length + 1, 0), 2, device=gt.device, dtype=torch.float64)
    size = int(L.lib().dvf_snippet_errors_ws_doubles(n))
    ws = L.workspace(("dvf_snippet_errors", n), size, torch.float64, gt.device)
    L.check(L.lib().dvf_snippet_errors(gt.data_ptr(), res.data_ptr(), n, int(length), rows.data_ptr() if rows.numel() else None,
                                       summary.data_ptr(), int(accumulate), ws.data_ptr(), size, L.stream()), "dvf_snippet_errors")
    return rows, summary


def overall(summary):
    """(mean t_err/len, mean r_err/len) of a summary, on the device; NaN when it counts no row (odometry_eval.overall_error)."""
    return summary[0] / summary[2], summary[1] / summary[2]
