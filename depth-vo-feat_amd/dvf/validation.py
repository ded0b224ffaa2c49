"""Validation passes against ground truth, their printed lines and their pose files: what train.py runs after every epoch
(through the validators of dvf/cli.py::run_training) and what depth_eval.py / odometry_eval.py run on a checkpoint.  Every pass
puts its network into eval mode, keeps its sums on the device and synchronises once, at its end."""
import contextlib
import math
import os

import torch

from odometry_eval import pose_line


@contextlib.contextmanager
def eval_mode(net):
    """``net`` in eval mode inside the block; the mode it had comes back afterwards, also when the block raises."""
    was_training = net.training
    net.eval()
    try:
        yield net
    finally:
        net.train(was_training)


@torch.no_grad()
def validate(pose_net, val_loader, device):
    """Reference train.py:220-247: mean over the validation SAMPLES of the per-batch L1 between the predicted relative
    pose (network output 0 through the se(3) exponential map, se3_generate.py) and the ground-truth 4x4 transform.
    The pose network runs in eval mode on (later frame, [earlier frame, earlier frame])."""
    from se3_generate import generate_se3
    total = torch.zeros((), device=device)
    with eval_mode(pose_net):
        for data, target in val_loader:
            data, target = data.float().to(device), target.float().to(device)
            tgt, ref = data[:, :3].contiguous(), data[:, 3:].contiguous()
            _, pose = pose_net(tgt, [ref, ref])
            out = generate_se3(pose[:, 0].reshape(-1, 6, 1, 1)).view(-1, 4, 4)
            total += torch.nn.functional.l1_loss(out, target)             # (the reference sums the per-batch means, :232)
    return float(total) / max(len(val_loader.dataset), 1)


def format_depth_metrics(metrics):
    """The line train.py and depth_eval.py print: ``Depth: abs_diff ... a3 ...``."""
    from .metrics import METRICS
    return "Depth: " + " ".join(f"{k} {metrics[k]:.9f}" for k in METRICS)


def raw_ground_truth(batch, device, velodyne_depth=False):
    """(frames, depth [B,Hg,Wg] on the device) of one batch of dataset.kitti_raw_depth_set(...).loader(b) = (frames, points
    [total,4], offsets [B+1] int32, proj [B,3,4] fp64, (Hg, Wg)): the LiDAR sweeps projected by dvf.velodyne.depth_maps."""
    from .velodyne import depth_maps
    img, points, offsets, proj, (hg, wg) = batch
    gt = depth_maps(points.float().to(device).contiguous(), offsets.to(device=device, dtype=torch.int32).contiguous(),
                    proj.to(device=device, dtype=torch.float64).contiguous(), int(hg), int(wg), velodyne_depth=velodyne_depth)
    return img, gt


@torch.no_grad()
def validate_depth(disp_net, loader, device, crop=True, median_scaling=True, velodyne_depth=False):
    """Depth validation against ground truth: the mean over the validation images (those with a valid pixel) of the eight
    metrics of dvf.metrics.depth_metrics, as a dict.  ``loader`` yields (frames [B,3,h,w], depth [B,Hg,Wg]) batches
    (dataset.depth_validation_set(...).loader(b)), or the five-part batches of dataset.kitti_raw_depth_set(...).loader(b),
    whose ground truth is then built on the device from the LiDAR sweeps (raw_ground_truth; ``velodyne_depth`` applies to
    these only).  The network runs in eval mode; its finest disparity is brought to the
    ground truth's size bilinearly (dvf_resize_bilinear_fwd, scale h/Hg, w/Wg) and inverted, then one depth_metrics call per
    batch; sums and the image count accumulate on the device (dvf.metrics.sum_rows / mean_rows, the two halves of
    reduce_rows) and the pass synchronises once, at its end."""
    from . import lib as L
    from .metrics import METRICS, depth_metrics, mean_rows, sum_rows
    total = torch.zeros(len(METRICS), device=device)
    count = torch.zeros((), device=device)
    with eval_mode(disp_net):
        for batch in loader:
            img, gt = batch if len(batch) == 2 else raw_ground_truth(batch, device, velodyne_depth)
            img, gt = img.float().to(device).contiguous(), gt.float().to(device).contiguous()
            disp = disp_net(img)
            disp = (disp[0] if type(disp) in (list, tuple) else disp).contiguous()
            b, _, h, w = disp.shape
            hg, wg = gt.shape[1:]
            up = torch.empty(b, hg, wg, device=device, dtype=torch.float32)
            L.check(L.lib().dvf_resize_bilinear_fwd(L.dev(disp, "disparity"), L.dev(up), b, h, w, hg, wg, h / hg, w / wg,
                                                    L.stream()), "dvf_resize_bilinear_fwd")
            depth = torch.empty_like(up)
            L.check(L.lib().dvf_recip_fwd(L.dev(up), L.dev(depth), 0.0, up.numel(), L.stream()), "dvf_recip_fwd")
            batch_total, batch_count = sum_rows(depth_metrics(gt, depth, crop=crop, median_scaling=median_scaling))
            total += batch_total
            count += batch_count
    return dict(zip(METRICS, mean_rows(total, count).tolist()))          # the pass's one synchronisation


def export_depth_tree(loader_or_set, out_root, device="cuda", velodyne_depth=False, batch_size=4):
    """Write the depth validation tree of a KITTI raw set (dataset.kitti_raw_depth_set(...) or its ``.loader(b)``) under
    ``out_root``: ``val.txt`` (one stem per line, ``<drive>_<id>``), ``image/<stem>.png`` (the original file, copied, not
    re-encoded) and ``depth/<stem>.npy`` (the map dvf.velodyne.depth_maps builds on the device, float32 [Hg,Wg] in metres, 0 =
    no measurement).  This is the layout dataset.depth_validation_set / --val-depth-root reads.  Returns the stems.  A loader
    brings its own batches; a set is walked in batches of ``batch_size``.  No frame is decoded here.  The export is a pass of
    its own: depth_eval.py --export-depth-root reads and projects every sweep once here and once more in validate_depth."""
    import shutil
    import numpy as np
    if isinstance(loader_or_set, torch.utils.data.DataLoader):           # set.loader(b): its dataset lists the set's batches
        source, batches = loader_or_set.dataset.source, loader_or_set.dataset.batches
    else:
        source, batches = loader_or_set, loader_or_set.batches(batch_size)
    if len(set(source.stems)) != len(source.stems):
        raise ValueError("export_depth_tree: the split lists a frame twice")
    for sub in ("image", "depth"):
        os.makedirs(os.path.join(out_root, sub), exist_ok=True)
    for indices in batches:
        _, gt = raw_ground_truth(source.collate(indices, frames=False), device, velodyne_depth)
        for i, depth in zip(indices, gt.cpu().numpy()):
            stem = source.stems[i]
            shutil.copyfile(source.images[i], os.path.join(out_root, "image", stem + os.path.splitext(source.images[i])[1]))
            np.save(os.path.join(out_root, "depth", stem + ".npy"), depth)
    with open(os.path.join(out_root, "val.txt"), "w") as f:
        f.write("".join(stem + "\n" for stem in source.stems))
    return list(source.stems)


def pose_epoch_lines(loss, is_best):
    """The line train.py prints after an epoch's validate() (a ``lines`` of dvf/cli.py::Validator, as the two below)."""
    return ["Test set: Average loss: {:.6f} [BEST:{}]".format(loss, is_best)]


def depth_epoch_lines(metrics, is_best):
    """The line train.py prints after an epoch's validate_depth()."""
    return [format_depth_metrics(metrics) + " [BEST:{}]".format(is_best)]


def odometry_epoch_lines(metrics, is_best):
    """The lines train.py prints after an epoch's validate_odometry(): the ``Trajectory:`` line follows when the pass aligned."""
    lines = [format_odometry(metrics) + " [BEST:{}]".format(is_best)]
    return lines + [format_trajectory(metrics)] if "align" in metrics else lines


POSE_CONVENTIONS = ("se3", "euler")


def format_odometry(metrics, name=None):
    """The line train.py and odometry_eval.py print: ``Odometry: t_err <%> r_err <deg/100m> segments <count>``, with
    ``seq <name>`` appended for one sequence of a pass."""
    line = f"Odometry: t_err {metrics['t_err']:.12g} r_err {metrics['r_err']:.12g} segments {metrics['segments']}"
    return line if name is None else f"{line} seq {name}"


TRAJECTORY_FIELDS = ("scale", "ate", "rpe_trans", "rpe_rot", "snippet_ate", "snippet_ate_std", "snippet_re", "snippets")


def format_trajectory(metrics, name=None):
    """The line train.py and odometry_eval.py print after the ``Odometry:`` line of an aligned pass: ``Trajectory: align <mode>
    scale <c> ATE <m> RPE_t <m> RPE_r <deg> snippet_ATE <mean> +- <std> snippets <count>``, with ``seq <name>`` appended for one
    sequence of a pass."""
    line = (f"Trajectory: align {metrics['align']} scale {metrics['scale']:.12g} ATE {metrics['ate']:.12g} "
            f"RPE_t {metrics['rpe_trans']:.12g} RPE_r {metrics['rpe_rot']:.12g} snippet_ATE {metrics['snippet_ate']:.12g} +- "
            f"{metrics['snippet_ate_std']:.12g} snippets {metrics['snippets']}")
    return line if name is None else f"{line} seq {name}"


@torch.no_grad()
def relative_poses(pose_net, sequences, device, batch_size, convention="se3"):
    """(rel [N,4,4] fp32 on the device, offsets) as dvf.odometry.chain_poses takes them: per sequence of ``sequences`` =
    dataset.odometry_sequences(...), batches of consecutive frame pairs go through the network as in ``validate()`` (eval mode,
    ``pose_net(later, [earlier, earlier])``, output 0) and dvf_pose_vec2mat_fwd writes every batch's matrices into the one
    buffer.  No synchronisation.  ``convention`` names how the six outputs are read, because the reference disagrees with
    itself: "se3" = (w, u) through the se(3) exponential map, what ``validate()`` scores (train.py:229-231); "euler" =
    (t, r-euler), what train.py's photometric loss trains them as (inverse_warp.py:141-157)."""
    from . import lib as L
    if convention not in POSE_CONVENTIONS:
        raise ValueError(f"convention must be one of {POSE_CONVENTIONS}, got {convention!r}")
    flags = L.POSE_SE3 if convention == "se3" else 0
    offsets = [0]
    for _, pairs, _ in sequences:
        offsets.append(offsets[-1] + len(pairs))
    N = offsets[-1]
    rel = torch.zeros(N, 4, 4, device=device, dtype=torch.float32)
    mats = torch.empty(N, 3, 4, device=device, dtype=torch.float32)
    k = 0
    with eval_mode(pose_net):
        for _, pairs, _ in sequences:
            for data, _ in torch.utils.data.DataLoader(pairs, batch_size=batch_size, shuffle=False, num_workers=0):
                data = data.float().to(device)
                tgt, ref = data[:, :3].contiguous(), data[:, 3:].contiguous()
                _, pose = pose_net(tgt, [ref, ref])
                vec = pose[:, 0].reshape(-1, 6).contiguous()
                b = vec.shape[0]
                # (the kernel's rows are 12 floats apart: the batches land side by side in mats, rel gets its fourth row below)
                L.check(L.lib().dvf_pose_vec2mat_fwd(L.dev(vec, "pose"), mats.data_ptr() + k * 48, b, flags, L.stream()),
                        "dvf_pose_vec2mat_fwd")
                k += b
    rel[:, :3] = mats
    rel[:, 3, 3] = 1.0
    return rel, offsets


# One row of score_trajectories' records: the KITTI segment sums of a sequence (dvf.odometry.sequence_errors), then, of an
# aligned pass, the fit (dvf.odometry.align), ATE / RPE (trajectory_errors) and the 5-frame snippet sums (snippet_errors).
SEGMENT_COLUMNS = ("t_sum", "r_sum", "segments", "path_length")
ALIGNED_COLUMNS = ("scale", "sv0", "sv1", "sv2", "ate", "rpe_trans", "rpe_rot", "snippet_ate_sum", "snippet_ate_sq_sum",
                   "snippet_re_sum", "snippets")
RECORD_COLUMNS = SEGMENT_COLUMNS + ALIGNED_COLUMNS


def score_trajectories(world, offsets, gts, align=None):
    """(records, aligned) of the chained trajectories ``world`` / ``offsets`` (dvf.odometry.chain_poses) against ``gts``, one
    [n,3,4] ground truth per sequence.  ``records``: fp64 [S + 1, len(RECORD_COLUMNS)] on the device, one row per sequence and a
    last row whose first three columns are the summary accumulated over all sequences, in sequence order; the ALIGNED_COLUMNS
    stay 0 when ``align`` is None.  With ``align`` (a mode of dvf.odometry.ALIGN_MODES) every sequence is brought onto its ground
    truth first and scored as aligned; ``aligned`` is laid out as ``world`` (None without).  Everything stays on the device: no
    synchronisation."""
    from . import odometry as O
    S, nseg = len(gts), len(SEGMENT_COLUMNS)
    records = torch.zeros(S + 1, len(RECORD_COLUMNS), device=world.device, dtype=torch.float64)
    summary = torch.zeros(4, device=world.device, dtype=torch.float64)
    aligned = torch.empty_like(world) if align is not None else None
    for s, gt in enumerate(gts):
        gt = torch.as_tensor(gt).to(device=world.device, dtype=torch.float64).contiguous()
        res = world[offsets[s] + s:offsets[s + 1] + s + 1]
        if align is not None:
            res, transform = O.align(gt, res, align)
            aligned[offsets[s] + s:offsets[s + 1] + s + 1] = res
            # transform = c, R[9], t[3], sv[3]; trajectory_errors = ate, rpe_trans, rpe_rot, n; the summary of snippet_errors =
            # sum ate, sum ate^2, sum re, snippets, 0
            records[s, nseg:] = torch.cat([transform[:1], transform[13:], O.trajectory_errors(gt, res)[:3],
                                           O.snippet_errors(gt, res)[1][:4]])
        rows, _ = O.sequence_errors(gt, res, summary)
        records[s, :nseg] = torch.stack([rows[:, 2].sum(), rows[:, 1].sum(), rows[:, 5].sum(), summary[3]])
    records[S, :3] = summary[:3]
    return records, aligned


def _segment_metrics(row):
    count, nan = row["segments"], float("nan")
    return {"t_err": 100.0 * row["t_sum"] / count if count else nan,
            "r_err": row["r_sum"] / count * 180.0 / math.pi * 100.0 if count else nan, "segments": int(count)}


def decode_records(rows, names, align=None):
    """The dict validate_odometry returns, from ``rows`` = score_trajectories' records on the host (``records.tolist()``) and
    the sequence names: NaN wherever a count is 0."""
    rows = [dict(zip(RECORD_COLUMNS, row)) for row in rows]
    out = _segment_metrics(rows[-1])
    out["per_sequence"] = {name: dict(_segment_metrics(row), path_length=row["path_length"]) for name, row in zip(names, rows)}
    if align is None:
        return out
    deg, nan = 180.0 / math.pi, float("nan")
    for name, row in zip(names, rows):
        count = row["snippets"]
        mean = row["snippet_ate_sum"] / count if count else nan
        out["per_sequence"][name].update(
            align=align, scale=row["scale"], singular_values=[row["sv0"], row["sv1"], row["sv2"]], ate=row["ate"],
            rpe_trans=row["rpe_trans"], rpe_rot=row["rpe_rot"] * deg, snippet_ate=mean,
            snippet_ate_std=math.sqrt(max(row["snippet_ate_sq_sum"] / count - mean * mean, 0.0)) if count else nan,
            snippet_re=row["snippet_re_sum"] / count * deg if count else nan, snippets=int(count))
    out["align"] = align
    for k in TRAJECTORY_FIELDS[:-1]:
        out[k] = sum(m[k] for m in out["per_sequence"].values()) / len(names)
    out["snippets"] = sum(m["snippets"] for m in out["per_sequence"].values())
    return out


def write_trajectories(output_dir, names, poses, offsets, suffix=""):
    """<name><suffix>.txt under ``output_dir`` for every sequence of ``poses`` / ``offsets`` (laid out as chain_poses returns
    them): one KITTI pose line per frame (odometry_eval.pose_line)."""
    os.makedirs(output_dir, exist_ok=True)
    host = poses.cpu().numpy()
    for s, name in enumerate(names):
        with open(os.path.join(output_dir, f"{name}{suffix}.txt"), "w") as f:
            f.writelines(pose_line(p) for p in host[offsets[s] + s:offsets[s + 1] + s + 1])


def validate_odometry(pose_net, sequences, device, batch_size, convention="se3", output_dir=None, keep=False, align=None):
    """Trajectory validation against ground truth: the KITTI odometry errors (tools/evaluation_tools.py:452-508) of the pose
    network's chained trajectory over ``sequences`` = dataset.odometry_sequences(...), as
    {"t_err": percent, "r_err": degrees per 100 m, "segments": count, "per_sequence": {name: the same three + "path_length"}}.

    relative_poses (``convention``), one dvf.odometry.chain_poses over all sequences, score_trajectories (one sequence_errors
    per sequence that accumulates into one summary) and decode_records.  Everything stays on the device and the pass
    synchronises once, before any file is written.  ``output_dir``: writes <name>.txt, one KITTI pose line per frame
    (write_trajectories).  ``keep``: the result also carries "rel" ([N,4,4] fp32), "world" ([N+S,3,4] fp64) and "offsets" as
    chain_poses takes and returns them.

    ``align``: a mode out of dvf.odometry.ALIGN_MODES ("none" included; None = no alignment, the dict above).  Each sequence's
    chained trajectory is brought onto its ground truth first (dvf.odometry.align: the fit reads the translations only, nothing
    is re-based) and t_err / r_err / segments are those of the aligned trajectory.  Every per_sequence entry then also carries
    "align", "scale" (c), "singular_values" (of the cross-covariance: two zeros mean a straight line, no unique rotation), "ate"
    and "rpe_trans" (m), "rpe_rot" (degrees per frame), and of the 5-frame snippets of inference.py:72-88 "snippet_ate" (mean),
    "snippet_ate_std" (population), "snippet_re" (mean, degrees) and "snippets" (count).  The top level carries "align", the
    plain mean over the sequences of scale, ate, rpe_trans, rpe_rot, snippet_ate, snippet_ate_std and snippet_re, and the total
    "snippets".  ``output_dir`` also gets <name>_aligned.txt (<name>.txt stays the raw chain) and ``keep`` also returns
    "aligned", laid out as "world"."""
    from .odometry import ALIGN_MODES, chain_poses
    if align is not None and align not in ALIGN_MODES:
        raise ValueError(f"align must be None or one of {ALIGN_MODES}, got {align!r}")
    if not sequences:
        raise ValueError("validate_odometry: no sequence to evaluate")
    names = [name for name, _, _ in sequences]
    rel, offsets = relative_poses(pose_net, sequences, device, batch_size, convention)
    world = chain_poses(rel, offsets)
    records, aligned = score_trajectories(world, offsets, [poses for _, _, poses in sequences], align)
    out = decode_records(records.tolist(), names, align)                 # the pass's one synchronisation
    if output_dir is not None:
        write_trajectories(output_dir, names, world, offsets)
        if align is not None:
            write_trajectories(output_dir, names, aligned, offsets, "_aligned")
    if keep:
        out.update(rel=rel, world=world, offsets=offsets)
        if align is not None:
            out["aligned"] = aligned
    return out
