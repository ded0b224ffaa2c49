"""Shared plumbing of the entry scripts (train.py / unsupervise.py / unsupervise_dvo.py): process-group setup,
synthetic data stream, the step loop with device-side loss accumulation, checkpoints in the reference's format.

Data: the seeded synthetic stream that the benchmark uses by default; with ``--data-root`` the stereo-sequence listing
of the reference's un_dataset.py is read through this build's PIL-based ``un_dataset.dataset``."""
import math
import os
import time

import torch
import torch.distributed as dist

from . import augment
from .engine import FlatAdam, GraphedStep
from .synthetic import synthetic_batch


def _augment_ops(text):
    """argparse type of --augment: a comma list of op names -> tuple of ops."""
    import argparse
    try:
        return augment.parse_ops(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def add_common_flags(parser):
    g = parser.add_argument_group("MI355X build extensions")
    g.add_argument("--synthetic", action="store_true", default=True,
                   help="seeded synthetic KITTI-shaped data (used when no --data-root listing is given)")
    g.add_argument("--data-root", default=None,
                   help="directory laid out like the reference's data/kitti_eigen (train.txt, intrinsics/, train_K/, "
                        "train_T_R2L/): read through un_dataset.dataset; each rank takes every world-th sample")
    g.add_argument("--height", type=int, default=256)
    g.add_argument("--width", type=int, default=832)
    g.add_argument("--steps-per-epoch", type=int, default=50, help="synthetic iterations per epoch")
    g.add_argument("--no-graph", action="store_true", help="eager launches instead of HIP-graph replay")
    g.add_argument("--deterministic", action="store_true",
                   help="weight / bias gradients summed in a fixed order (no float atomics): runs from identical state are "
                        "bit-identical, as on the reference's CPU path, except the gradients of the FeatExtractor's "
                        "parameters when the feature term is on (the photometric backward scatters the source-feature "
                        "gradients, and the depthwise up-convolutions sum their weight gradients, with float atomics); "
                        "costs ~5 %% of a step")
    g.add_argument("--ssim-weight", type=float, default=0.0, metavar="A",
                   help="A > 0: the image photometric term becomes A * DSSIM + (1 - A) * L1 (monodepth2 form, 3x3 reflected "
                        "windows; 0.85 is the usual choice); 0 = the reference's L1.  The reference has no SSIM: parity unpinned")
    g.add_argument("--ssim-c1", type=float, default=1e-4, metavar="C1",
                   help="SSIM luminance constant, 0.01^2 for a unit value range (train.py feeds [-1, 1], unsupervise.py 0.004 * img)")
    g.add_argument("--ssim-c2", type=float, default=9e-4, metavar="C2", help="SSIM contrast constant, 0.03^2 for a unit value range")
    g.add_argument("--min-reprojection", action="store_true",
                   help="the image appearance term (A * DSSIM + (1 - A) * L1, A = --ssim-weight, 0 allowed) takes the per-pixel "
                        "minimum over the reference views instead of their sum (monodepth2 form); the explainability mask is "
                        "not used in this mode (train.py: needs -m 0).  Not in the reference: parity unpinned")
    g.add_argument("--auto-mask", action="store_true",
                   help="with --min-reprojection: the unwarped reference views compete in the minimum, so pixels that do not "
                        "move between frames are won by an identity candidate; the logged 'automask' is their share")
    g.add_argument("--full-res-multiscale", action="store_true",
                   help="train.py only: every scale's disparity (and explainability mask) is upsampled bilinearly to the input "
                        "resolution and its photometric term is taken there, against the full-resolution images (monodepth2 "
                        "form), instead of at the scale's own resolution; smoothness and the mask regulariser stay at the "
                        "native scales.  Not in the reference: parity unpinned.  The single-scale entry points refuse it")
    g.add_argument("--normalized-smoothness", action="store_true",
                   help="the smoothness term becomes the edge-aware first-order smoothness of the mean-normalised disparity, "
                        "against the target image (monodepth2 form), instead of the second-order smoothness of depth; it keeps "
                        "the entry point's smoothness weight, which was chosen for the other term: monodepth2 uses 1e-3, so "
                        "train.py -s 0.001, unsupervise.py / unsupervise_dvo.py --smooth-weight 0.001.  Not in the reference: "
                        "parity unpinned, tests/normsmooth_ref.py is the definition")
    g.add_argument("--reference-stereo-pose", action="store_true",
                   help="feed the dataset's T_R2L file vector (0,0,0,Tx,0,0) unchanged into pose_vec2mat / the stereo-pose "
                        "MSE target, exactly as the reference does (unsupervise.py:101, train.py:201); default: convert it "
                        "to the (t, r-euler) order those functions read (un_dataset.to_batch)")
    g.add_argument("--augment", nargs="?", type=_augment_ops, const=augment.OPS, default=None, metavar="OPS",
                   help="training augmentation on the GPU, one draw per sample applied to all its frames (seeded by --seed and the "
                        "rank); OPS is a comma list out of flip,zoom,colour (no value: all three).  flip: horizontal mirror "
                        "with probability 0.5, the stereo baseline changes sign; zoom: zoom by U[1, 1.15] per axis to an integer "
                        "size, then a random crop back to the input size (bilinear); colour: with probability 0.5 gamma "
                        "U[0.8, 1.2], brightness U[0.5, 2.0] and per-channel gains U[0.8, 1.2].  An extension in place of the "
                        "reference's custom_transforms.py (parity unpinned, tests/augment_ref.py is the definition), with two "
                        "departures: the intrinsics follow the exact pixel map (integer zoomed size, half-pixel term) instead "
                        "of the untruncated factor, and a flip mirrors cx as W - 1 - cx instead of w - cx")


def ssim_kwargs(args):
    """The --ssim-* flags as keywords of the step bodies (dvf/steps.py)."""
    return {"ssim_weight": args.ssim_weight, "ssim_c1": args.ssim_c1, "ssim_c2": args.ssim_c2}


def minreproj_kwargs(args):
    """The --min-reprojection / --auto-mask flags as keywords of the step bodies (dvf/steps.py)."""
    return {"min_reprojection": args.min_reprojection, "auto_mask": args.auto_mask}


def normsmooth_kwargs(args):
    """The --normalized-smoothness flag as a keyword of the step bodies (dvf/steps.py)."""
    return {"normalized_smoothness": args.normalized_smoothness}


FULLRES_SINGLE_SCALE = ("--full-res-multiscale needs a multi-scale loss: this entry point has a single scale, already at the "
                        "input resolution (use train.py)")


def fullres_kwargs(args, multiscale=True):
    """The --full-res-multiscale flag as a keyword of the multi-scale step body (dvf/steps.py::train_sfm_losses).  An entry
    point whose loss has one scale calls this with ``multiscale=False``: it gets no keyword, and the flag raises ValueError
    there instead of being ignored."""
    if not multiscale:
        if args.full_res_multiscale:
            raise ValueError(FULLRES_SINGLE_SCALE)
        return {}
    return {"full_res_multiscale": args.full_res_multiscale}


def init_distributed():
    """One process per GPU; RANK/LOCAL_RANK/WORLD_SIZE from torchrun.  Returns (rank, world, device)."""
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no CUDA/HIP device visible and there is no CPU fallback")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    return rank, world, device


def load_pretrained(module, path, strict=True):
    """Reference checkpoint convention (train.py:129-141): a dict with key 'state_dict', or a bare state_dict."""
    weights = torch.load(path, map_location="cpu", weights_only=True)
    module.load_state_dict(weights["state_dict"] if "state_dict" in weights else weights, strict=strict)


def save_best(output_dir, named_modules):
    """Reference file names (train.py:242-247, unsupervise.py:156-163): bare state_dicts."""
    os.makedirs(output_dir, exist_ok=True)
    for fname, module in named_modules:
        # parameters are views into FlatAdam's single arena: clone, or torch.save would serialise the whole arena
        # (every network's weights) into each file
        torch.save({k: v.detach().cpu().clone() for k, v in module.state_dict().items()}, os.path.join(output_dir, fname))


@torch.no_grad()
def validate(pose_net, val_loader, device):
    """Reference train.py:220-247: mean over the validation SAMPLES of the per-batch L1 between the predicted relative
    pose (network output 0 through the se(3) exponential map, se3_generate.py) and the ground-truth 4x4 transform.
    The pose network runs in eval mode on (later frame, [earlier frame, earlier frame])."""
    from se3_generate import generate_se3
    was_training = pose_net.training
    pose_net.eval()
    total = torch.zeros((), device=device)
    for data, target in val_loader:
        data, target = data.float().to(device), target.float().to(device)
        tgt, ref = data[:, :3].contiguous(), data[:, 3:].contiguous()
        _, pose = pose_net(tgt, [ref, ref])
        out = generate_se3(pose[:, 0].reshape(-1, 6, 1, 1)).view(-1, 4, 4)
        total += torch.nn.functional.l1_loss(out, target)                 # (the reference sums the per-batch means, :232)
    pose_net.train(was_training)
    return float(total) / max(len(val_loader.dataset), 1)


def format_depth_metrics(metrics):
    """The line train.py and depth_eval.py print: ``Depth: abs_diff ... a3 ...``."""
    from .metrics import METRICS
    return "Depth: " + " ".join(f"{k} {metrics[k]:.9f}" for k in METRICS)


@torch.no_grad()
def validate_depth(disp_net, loader, device, crop=True, median_scaling=True):
    """Depth validation against ground truth: the mean over the validation images (those with a valid pixel) of the eight
    metrics of dvf.metrics.depth_metrics, as a dict.  ``loader`` yields (frames [B,3,h,w], depth [B,Hg,Wg]) batches
    (dataset.depth_validation_set(...).loader(b)).  The network runs in eval mode; its finest disparity is brought to the
    ground truth's size bilinearly (dvf_resize_bilinear_fwd, scale h/Hg, w/Wg) and inverted, then one depth_metrics call per
    batch; rows and the image count accumulate on the device and the pass synchronises once, at its end."""
    from . import lib as L
    from .metrics import METRICS, depth_metrics
    was_training = disp_net.training
    disp_net.eval()
    total = torch.zeros(len(METRICS), device=device)
    count = torch.zeros((), device=device)
    for img, gt in loader:
        img, gt = img.float().to(device).contiguous(), gt.float().to(device).contiguous()
        disp = disp_net(img)
        disp = (disp[0] if type(disp) in (list, tuple) else disp).contiguous()
        b, _, h, w = disp.shape
        hg, wg = gt.shape[1:]
        up = torch.empty(b, hg, wg, device=device, dtype=torch.float32)
        L.check(L.lib().dvf_resize_bilinear_fwd(L.dev(disp, "disparity"), L.dev(up), b, h, w, hg, wg, h / hg, w / wg, L.stream()),
                "dvf_resize_bilinear_fwd")
        depth = torch.empty_like(up)
        L.check(L.lib().dvf_recip_fwd(L.dev(up), L.dev(depth), 0.0, up.numel(), L.stream()), "dvf_recip_fwd")
        rows = depth_metrics(gt, depth, crop=crop, median_scaling=median_scaling)
        keep = (rows[:, 8] > 0).float()
        total += (rows[:, :len(METRICS)] * keep[:, None]).sum(0)
        count += keep.sum()
    means = (total / count.clamp(min=1.0)).tolist()                     # the pass's one synchronisation
    disp_net.train(was_training)
    return dict(zip(METRICS, means))


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
def validate_odometry(pose_net, sequences, device, batch_size, convention="se3", output_dir=None, keep=False, align=None):
    """Trajectory validation against ground truth: the KITTI odometry errors (tools/evaluation_tools.py:452-508) of the pose
    network's chained trajectory over ``sequences`` = dataset.odometry_sequences(...), as
    {"t_err": percent, "r_err": degrees per 100 m, "segments": count, "per_sequence": {name: the same three + "path_length"}}.

    Per sequence, batches of consecutive frame pairs go through the network as in ``validate()`` (eval mode, ``pose_net(later,
    [earlier, earlier])``, output 0); dvf_pose_vec2mat_fwd writes every batch's matrices into one device buffer for all
    sequences, then one dvf.odometry.chain_poses and one sequence_errors per sequence that accumulates into one summary.
    Everything stays on the device and the pass synchronises once, at its end.  No scale alignment unless ``align`` is given.

    ``convention`` names how the six outputs are read, because the reference disagrees with itself: "se3" = (w, u) through the
    se(3) exponential map, what ``validate()`` scores (train.py:229-231); "euler" = (t, r-euler), what train.py's photometric
    loss trains them as (inverse_warp.py:141-157).  ``output_dir``: writes <name>.txt, one KITTI pose line per frame
    (odometry_eval.save_result_poses' format), after the synchronisation.  ``keep``: the result also carries "rel" ([N,4,4]
    fp32), "world" ([N+S,3,4] fp64) and "offsets" as chain_poses takes and returns them.

    ``align``: a mode out of dvf.odometry.ALIGN_MODES ("none" included; None = everything above, unchanged).  Each sequence's
    chained trajectory is brought onto its ground truth first (dvf.odometry.align: the fit reads the translations only, nothing
    is re-based) and t_err / r_err / segments are those of the aligned trajectory.  Every per_sequence entry then also carries
    "align", "scale" (c), "singular_values" (of the cross-covariance: two zeros mean a straight line, no unique rotation), "ate"
    and "rpe_trans" (m), "rpe_rot" (degrees per frame), and of the 5-frame snippets of inference.py:72-88 "snippet_ate" (mean),
    "snippet_ate_std" (population), "snippet_re" (mean, degrees) and "snippets" (count).  The top level carries "align", the
    plain mean over the sequences of scale, ate, rpe_trans, rpe_rot, snippet_ate, snippet_ate_std and snippet_re, and the total
    "snippets".  Still one synchronisation.  ``output_dir`` also gets <name>_aligned.txt (<name>.txt stays the raw chain) and
    ``keep`` also returns "aligned", laid out as "world"."""
    from . import lib as L
    from . import odometry as O
    from .odometry import chain_poses, sequence_errors
    if align is not None and align not in O.ALIGN_MODES:
        raise ValueError(f"align must be None or one of {O.ALIGN_MODES}, got {align!r}")
    if convention not in POSE_CONVENTIONS:
        raise ValueError(f"convention must be one of {POSE_CONVENTIONS}, got {convention!r}")
    if not sequences:
        raise ValueError("validate_odometry: no sequence to evaluate")
    flags = L.POSE_SE3 if convention == "se3" else 0
    was_training = pose_net.training
    pose_net.eval()
    offsets = [0]
    for _, pairs, _ in sequences:
        offsets.append(offsets[-1] + len(pairs))
    N = offsets[-1]
    rel = torch.zeros(N, 4, 4, device=device, dtype=torch.float32)
    mats = torch.empty(N, 3, 4, device=device, dtype=torch.float32)
    k = 0
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
    world = chain_poses(rel, offsets)
    summary = torch.zeros(4, device=device, dtype=torch.float64)
    per, extra = [], []
    aligned = torch.empty_like(world) if align is not None else None
    for s, (_, _, poses) in enumerate(sequences):
        gt = torch.from_numpy(poses).to(device=device, dtype=torch.float64).contiguous()
        res = world[offsets[s] + s:offsets[s + 1] + s + 1]
        if align is not None:
            res, transform = O.align(gt, res, align)
            aligned[offsets[s] + s:offsets[s + 1] + s + 1] = res
            # [c, sv (3), ate, rpe_trans, rpe_rot, n, sum ate, sum ate^2, sum re, snippets, 0]
            extra.append(torch.cat([transform[:1], transform[13:], O.trajectory_errors(gt, res), O.snippet_errors(gt, res)[1]]))
        rows, _ = sequence_errors(gt, res, summary)
        per.append(torch.stack([rows[:, 2].sum(), rows[:, 1].sum(), rows[:, 5].sum(), summary[3]]))
    flat = torch.cat([summary[:3]] + per + extra).tolist()              # the pass's one synchronisation
    pose_net.train(was_training)

    def metrics(t_sum, r_sum, count):
        nan = float("nan")
        return {"t_err": 100.0 * t_sum / count if count else nan, "r_err": r_sum / count * 180.0 / math.pi * 100.0 if count else nan,
                "segments": int(count)}

    out = metrics(*flat[:3])
    out["per_sequence"] = {}
    for s, (name, _, _) in enumerate(sequences):
        out["per_sequence"][name] = dict(metrics(*flat[3 + 4 * s:6 + 4 * s]), path_length=flat[6 + 4 * s])
    if align is not None:
        deg, nan = 180.0 / math.pi, float("nan")
        for s, (name, _, _) in enumerate(sequences):
            c, sv0, sv1, sv2, ate, rpe_t, rpe_r, _, s_ate, s_ate2, s_re, count, _ = flat[3 + 4 * len(sequences) + 13 * s:][:13]
            mean = s_ate / count if count else nan
            out["per_sequence"][name].update(
                align=align, scale=c, singular_values=[sv0, sv1, sv2], ate=ate, rpe_trans=rpe_t, rpe_rot=rpe_r * deg,
                snippet_ate=mean, snippet_ate_std=math.sqrt(max(s_ate2 / count - mean * mean, 0.0)) if count else nan,
                snippet_re=s_re / count * deg if count else nan, snippets=int(count))
        out["align"] = align
        for k in TRAJECTORY_FIELDS[:-1]:
            out[k] = sum(m[k] for m in out["per_sequence"].values()) / len(sequences)
        out["snippets"] = sum(m["snippets"] for m in out["per_sequence"].values())
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        host = world.cpu().numpy()
        for s, (name, _, _) in enumerate(sequences):
            with open(os.path.join(output_dir, f"{name}.txt"), "w") as f:
                for p in host[offsets[s] + s:offsets[s + 1] + s + 1]:
                    f.write(" ".join(str(v) for v in p.reshape(12)) + "\n")
        if align is not None:
            host = aligned.cpu().numpy()
            for s, (name, _, _) in enumerate(sequences):
                with open(os.path.join(output_dir, f"{name}_aligned.txt"), "w") as f:
                    for p in host[offsets[s] + s:offsets[s + 1] + s + 1]:
                        f.write(" ".join(str(v) for v in p.reshape(12)) + "\n")
    if keep:
        out.update(rel=rel, world=world, offsets=offsets)
        if align is not None:
            out["aligned"] = aligned
    return out


def run_training(args, nets, loss_fn, lr, betas, weight_decay, term_names, ckpt_names, n_views=2, val_fn=None,
                 depth_val_fn=None, depth_ckpt=None, odometry_val_fn=None, odometry_ckpt=None):
    """Epoch loop.  ``loss_fn(batch) -> (loss, terms)``; ``nets``: list of modules in optimizer-group order.
    ``depth_val_fn`` (rank 0, optional): returns the dict of ``validate_depth`` after every epoch; its line is printed and
    ``depth_ckpt`` = (file name, module) is then saved on the best abs_rel instead of on the criterion of the other
    checkpoints, which stays as it is.  ``odometry_val_fn`` (rank 0, optional): returns the dict of ``validate_odometry``
    after every epoch; its line is printed (and the ``Trajectory:`` line of an aligned pass) and ``odometry_ckpt`` = (file
    name, module), a file of its own, is saved on the best t_err, the aligned one when the pass aligns."""
    rank, world, device = args._rank, args._world, args._device
    if getattr(args, "deterministic", False):
        from . import conv as _conv
        _conv.set_deterministic(True)
    params = [p for net in nets for p in net.parameters()]
    opt = FlatAdam(params, lr=lr, betas=betas, weight_decay=weight_decay, world_size=world, overlap=True)
    batch = synthetic_batch(args.batch_size, args.height, args.width, seed=1234 + args.seed, rank=rank, n_views=n_views,
                            device=device)
    # real data: un_dataset.dataset -> DataLoader (sharded by rank); every step copies the next batch INTO the static
    # input tensors, so the step (eager or graph replay) always reads the same addresses
    feed = None
    if getattr(args, "data_root", None):
        import un_dataset
        ds = un_dataset.dataset(img_height=args.height, img_width=args.width, root=args.data_root, seed=args.seed)
        idx = list(range(rank, len(ds), world))
        loader = torch.utils.data.DataLoader(torch.utils.data.Subset(ds, idx), batch_size=args.batch_size, shuffle=True,
                                             num_workers=getattr(args, "workers", 0), drop_last=True, pin_memory=True)
        args.steps_per_epoch = max(1, len(loader))

        def feed():
            while True:
                for sample in loader:
                    yield un_dataset.to_batch(sample, device, getattr(args, "reference_stereo_pose", False))
        feed = feed()
    KEYS = ("img_R2", "img_R1", "img_L2", "K", "Kinv", "T_R2L", "T_R2L_se3")
    aug_ops = getattr(args, "augment", None)
    if aug_ops is not None:
        aug_gen = torch.Generator().manual_seed(977 * args.seed + rank + 31)
        pristine = None if feed is not None else \
            {k: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for k, v in batch.items()}

        def next_records():
            rec = augment.sample_params(aug_gen, args.batch_size, args.height, args.width, aug_ops)
            augment.validate_params(rec, args.height, args.width)
            # a fresh pinned tensor per step: a staging buffer whose copy may still be in flight is never rewritten
            return rec.pin_memory().to(device, non_blocking=True)

    def load_next():
        nxt = next(feed)
        if aug_ops is not None:
            # loader tensor -> static tensor in one pass, in place of the copies below
            augment.augment_batch({k: nxt[k].reshape(batch[k].shape) for k in KEYS}, batch, next_records())
            return
        for k in KEYS:
            batch[k].copy_(nxt[k].reshape(batch[k].shape), non_blocking=True)

    if feed is not None:
        load_next()              # the warm-up / capture steps below already train: they must see real data, not noise
    elif aug_ops is not None:
        augment.augment_batch(pristine, batch, next_records())
    acc = torch.zeros(len(term_names), device=device)            # device-side running sums: no per-step .item()

    def step():
        loss, terms = loss_fn(batch)
        opt.zero_grad()
        loss.backward()
        opt.step()
        acc.add_(torch.stack([terms[k] for k in term_names]))
        return (terms["total"],)

    runner = step
    if world == 1 and not args.no_graph:
        step()                                                   # one eager step sizes every workspace
        runner = GraphedStep(step, [], warmup=1)
    best = best_abs_rel = best_t_err = float("inf")
    if depth_val_fn is not None:
        ckpt_names = [c for c in ckpt_names if c[0] != depth_ckpt[0]]
    for epoch in range(args.epochs):
        acc.zero_()
        t0 = time.perf_counter()
        for it in range(args.steps_per_epoch):
            if feed is not None and (epoch, it) != (0, 0):
                load_next()
            elif feed is None and aug_ops is not None:
                augment.augment_batch(pristine, batch, next_records())    # a new view of the synthetic batch every step
            runner()
            if getattr(args, "log_interval", 0) and rank == 0 and (it + 1) % args.log_interval == 0:
                # (one host sync per log interval; the reference syncs on five .item() calls every step, train.py:205-209)
                print(f"  epoch {epoch} [{it + 1}/{args.steps_per_epoch}] {term_names[0]}: "
                      f"{float(acc[0]) / (it + 1):.6f}", flush=True)
            # a fresh synthetic batch every step would only change values, not the work; new data is copied into the
            # static input tensors in place (graph replay reads the same addresses)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        means = (acc / args.steps_per_epoch).tolist()
        if world > 1:
            tt = torch.tensor(means, device=device)
            dist.all_reduce(tt)
            means = (tt / world).tolist()
        if rank == 0:
            msg = " ".join(f"{k}: {v:.9f}" for k, v in zip(term_names, means))
            print(f"Train epoch {epoch}: {msg}  [{args.batch_size * world * args.steps_per_epoch / dt:.1f} samples/s]", flush=True)
            # checkpoint criterion: the reference's validate() (train.py:238-247) when a validation set is given,
            # else the best training loss
            score = means[0]
            if val_fn is not None:
                score = val_fn()
                print("Test set: Average loss: {:.6f} [BEST:{}]".format(score, score < best), flush=True)
            if score < best:
                best = score
                save_best(args.output_dir, ckpt_names)
            if depth_val_fn is not None:
                # eager launches between graph replays; a geometry first seen here gets its packed weights like any other
                depth = depth_val_fn()
                print(format_depth_metrics(depth) + " [BEST:{}]".format(depth["abs_rel"] < best_abs_rel), flush=True)
                if depth["abs_rel"] < best_abs_rel:
                    best_abs_rel = depth["abs_rel"]
                    save_best(args.output_dir, [depth_ckpt])
            if odometry_val_fn is not None:
                odo = odometry_val_fn()
                print(format_odometry(odo) + " [BEST:{}]".format(odo["t_err"] < best_t_err), flush=True)
                if "align" in odo:
                    print(format_trajectory(odo), flush=True)
                if odo["t_err"] < best_t_err:
                    best_t_err = odo["t_err"]
                    save_best(args.output_dir, [odometry_ckpt])
    if world > 1:
        dist.destroy_process_group()
