"""The host halves of validation, no GPU: the end-of-epoch rule of dvf/cli.py (epoch_end_entries / end_epoch) with stub
validators, dvf/validation.py's eval_mode, record decoder and pose-file writer, and the constants that exist once."""
import math
import os

import numpy as np
import pytest
import torch

import depth_eval
import odometry_eval as oe
from dvf import cli, validation

DEPTH_LINE = ("Depth: abs_diff 0.500000000 abs_rel {} sq_rel 0.500000000 rmse 0.500000000 rmse_log 0.500000000 a1 0.500000000 "
              "a2 0.500000000 a3 0.500000000 [BEST:{}]")
VO, DEPTH, ODO = "best_vo_checkpoint.pth.tar", "best_depth_checkpoint.pth.tar", "best_odometry_checkpoint.pth.tar"
CKPTS = [(VO, "pose net"), (DEPTH, "disp net")]


def _depth(abs_rel):
    return dict({k: 0.5 for k in ("abs_diff", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")}, abs_rel=abs_rel)


def _epochs(capsys, validators, train_losses):
    """Per epoch (printed lines, checkpoint lists handed to save) of end_epoch over the entries of ``validators``."""
    entries = cli.epoch_end_entries(CKPTS, validators)
    best = [float("inf")] * len(entries)
    out = []
    for loss in train_losses:
        saved = []
        cli.end_epoch(entries, best, loss, saved.append)
        out.append((capsys.readouterr().out.splitlines(), saved))
    return out


def test_without_a_validator_the_training_loss_decides_and_nothing_is_printed(capsys):
    assert _epochs(capsys, (), [3.0, 2.0, 2.5, 2.0, 1.0]) == [([], [CKPTS]), ([], [CKPTS]), ([], []), ([], []), ([], [CKPTS])]


def test_three_validators_each_print_their_lines_and_save_their_own_files_on_their_own_best(capsys):
    pose = iter([0.5, 0.25, 0.3])
    depth = iter([0.2, 0.3, 0.1])
    aligned = dict(align="scale", scale=2.0, ate=0.5, rpe_trans=0.25, rpe_rot=0.125, snippet_ate=1.5, snippet_ate_std=0.75, snippets=16)
    odo = iter([dict(t_err=5.0, r_err=1.5, segments=7), dict(t_err=float("nan"), r_err=float("nan"), segments=0),
                dict(aligned, t_err=4.0, r_err=1.25, segments=7)])
    validators = [cli.Validator(lambda _: next(pose), float, validation.pose_epoch_lines, None),
                  cli.Validator(lambda _: _depth(next(depth)), lambda m: m["abs_rel"], validation.depth_epoch_lines, [(DEPTH, "disp net")]),
                  cli.Validator(lambda _: next(odo), lambda m: m["t_err"], validation.odometry_epoch_lines, [(ODO, "pose net")])]
    got = _epochs(capsys, validators, [9.0, 1.0, 0.5])                   # (the training loss decides nothing here)
    assert got[0] == (["Test set: Average loss: 0.500000 [BEST:True]", DEPTH_LINE.format("0.200000000", True),
                       "Odometry: t_err 5 r_err 1.5 segments 7 [BEST:True]"],
                      [[(VO, "pose net")], [(DEPTH, "disp net")], [(ODO, "pose net")]])
    assert got[1] == (["Test set: Average loss: 0.250000 [BEST:True]", DEPTH_LINE.format("0.300000000", False),
                       "Odometry: t_err nan r_err nan segments 0 [BEST:False]"], [[(VO, "pose net")]])
    assert got[2] == (["Test set: Average loss: 0.300000 [BEST:False]", DEPTH_LINE.format("0.100000000", True),
                       "Odometry: t_err 4 r_err 1.25 segments 7 [BEST:True]",
                       "Trajectory: align scale scale 2 ATE 0.5 RPE_t 0.25 RPE_r 0.125 snippet_ATE 1.5 +- 0.75 snippets 16"],
                      [[(DEPTH, "disp net")], [(ODO, "pose net")]])


def test_a_file_claimed_by_a_validator_leaves_the_training_loss_entry(capsys):
    depth = iter([0.2, 0.3])
    validators = [cli.Validator(lambda _: _depth(next(depth)), lambda m: m["abs_rel"], validation.depth_epoch_lines, [(DEPTH, "disp net")])]
    entries = cli.epoch_end_entries(CKPTS, validators)
    assert [v.ckpts for v in entries] == [[(VO, "pose net")], [(DEPTH, "disp net")]] and CKPTS == [(VO, "pose net"), (DEPTH, "disp net")]
    assert _epochs(capsys, validators, [2.0, 1.0]) == [
        ([DEPTH_LINE.format("0.200000000", True)], [[(VO, "pose net")], [(DEPTH, "disp net")]]),
        ([DEPTH_LINE.format("0.300000000", False)], [[(VO, "pose net")]])]


def test_eval_mode_restores_the_mode_after_a_body_that_raises():
    net = torch.nn.Linear(2, 2)
    for mode in (True, False):
        net.train(mode)
        with pytest.raises(KeyError):
            with validation.eval_mode(net) as inside:
                assert inside is net and not net.training
                raise KeyError("the pass failed")
        assert net.training is mode
    with validation.eval_mode(net.train()):
        assert not net.training
    assert net.training


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return type(a) is type(b) and a == b


def _records(**columns):
    """A records tensor of two sequences and the summary row: every named column's three values, the others 0."""
    rec = torch.zeros(3, len(validation.RECORD_COLUMNS), dtype=torch.float64)
    for name, values in columns.items():
        rec[:, validation.RECORD_COLUMNS.index(name)] = torch.tensor(values, dtype=torch.float64)
    return rec


def test_decode_records_by_column_name_with_nan_where_a_count_is_zero():
    nan, deg = float("nan"), 180.0 / math.pi
    rec = _records(t_sum=[0.5, 0.0, 0.5], r_sum=[0.25, 0.0, 0.25], segments=[4.0, 0.0, 4.0], path_length=[123.5, 7.25, 0.0])
    plain = validation.decode_records(rec.tolist(), ["09", "10"])
    seq09 = {"t_err": 12.5, "r_err": 0.0625 * 180.0 / math.pi * 100.0, "segments": 4, "path_length": 123.5}
    seq10 = {"t_err": nan, "r_err": nan, "segments": 0, "path_length": 7.25}
    assert _same(plain, {"t_err": 12.5, "r_err": seq09["r_err"], "segments": 4, "per_sequence": {"09": seq09, "10": seq10}})
    assert sorted(plain) == ["per_sequence", "r_err", "segments", "t_err"]
    assert sorted(plain["per_sequence"]["09"]) == ["path_length", "r_err", "segments", "t_err"]

    rec = _records(t_sum=[0.5, 0.0, 0.5], r_sum=[0.25, 0.0, 0.25], segments=[4.0, 0.0, 4.0], path_length=[123.5, 7.25, 0.0],
                   scale=[2.0, 1.0, 0.0], sv0=[3.0, 0.5, 0.0], sv1=[2.0, 0.0, 0.0], sv2=[1.0, 0.0, 0.0], ate=[0.5, 0.25, 0.0],
                   rpe_trans=[0.25, nan, 0.0], rpe_rot=[0.125, nan, 0.0], snippet_ate_sum=[6.0, 0.0, 0.0],
                   snippet_ate_sq_sum=[20.0, 0.0, 0.0], snippet_re_sum=[0.5, 0.0, 0.0], snippets=[4.0, 0.0, 0.0])
    got = validation.decode_records(rec.tolist(), ["09", "10"], "7dof")
    seq09 = dict(seq09, align="7dof", scale=2.0, singular_values=[3.0, 2.0, 1.0], ate=0.5, rpe_trans=0.25, rpe_rot=0.125 * deg,
                 snippet_ate=1.5, snippet_ate_std=math.sqrt(2.75), snippet_re=0.125 * deg, snippets=4)
    seq10 = dict(seq10, align="7dof", scale=1.0, singular_values=[0.5, 0.0, 0.0], ate=0.25, rpe_trans=nan, rpe_rot=nan,
                 snippet_ate=nan, snippet_ate_std=nan, snippet_re=nan, snippets=0)
    assert _same(got, {"t_err": 12.5, "r_err": seq09["r_err"], "segments": 4, "per_sequence": {"09": seq09, "10": seq10},
                       "align": "7dof", "scale": 1.5, "ate": 0.375, "rpe_trans": nan, "rpe_rot": nan, "snippet_ate": nan,
                       "snippet_ate_std": nan, "snippet_re": nan, "snippets": 4})


def test_the_shared_constants_exist_once():
    from dvf import metrics, odometry
    for name in ("ALIGN_MODES", "SEGMENT_LENGTHS", "FIRST_FRAME", "FRAME_STEP"):
        assert getattr(odometry, name) is getattr(oe, name)
    assert metrics.garg_rect is depth_eval.garg_rect
    y1, y2, x1, x2 = depth_eval.garg_rect(375, 1242)
    assert (y1, y2, x1, x2) == (153, 371, 44, 1197)                      # int() of loss_functions_sfm.py:92-93's products
    want = np.zeros((375, 1242), dtype=bool)
    want[y1:y2, x1:x2] = True
    assert np.array_equal(depth_eval.garg_crop_mask(375, 1242), want)


def test_write_trajectories_files_load_back_exactly_and_match_save_result_poses(tmp_path):
    poses = torch.randn(7, 3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(5)) * 1e3
    offsets, names = [0, 2, 5], ["09", "10"]                             # 2 and 3 relative poses: 3 and 4 frames
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    validation.write_trajectories(a, names, poses, offsets)
    validation.write_trajectories(a, names, poses * 2.0, offsets, "_aligned")
    assert sorted(os.listdir(a)) == ["09.txt", "09_aligned.txt", "10.txt", "10_aligned.txt"]
    os.makedirs(b)
    for name, rows in (("09", poses[0:3]), ("10", poses[3:7])):
        back = oe.load_poses(os.path.join(a, f"{name}.txt"))
        assert np.array_equal(np.stack([back[i] for i in range(len(rows))])[:, :3], rows.numpy())
        back = oe.load_poses(os.path.join(a, f"{name}_aligned.txt"))
        assert np.array_equal(np.stack([back[i] for i in range(len(rows))])[:, :3], (rows * 2.0).numpy())
        for p in rows.numpy():
            oe.save_result_poses(p, b, f"{name}.txt")
        with open(os.path.join(a, f"{name}.txt"), "rb") as f, open(os.path.join(b, f"{name}.txt"), "rb") as g:
            assert f.read() == g.read()
