"""Shared plumbing of the entry scripts (train.py / unsupervise.py / unsupervise_dvo.py): process-group setup,
synthetic data stream, the step loop with device-side loss accumulation, checkpoints in the reference's format.

Data: the seeded synthetic stream that the benchmark uses by default; with ``--data-root`` the stereo-sequence listing
of the reference's un_dataset.py is read through this build's PIL-based ``un_dataset.dataset``."""
import collections
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


def require_gpu():
    """Every entry script's first step: exit when no GPU is visible."""
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no CUDA/HIP device visible and there is no CPU fallback")


def init_distributed():
    """One process per GPU; RANK/LOCAL_RANK/WORLD_SIZE from torchrun.  Returns (rank, world, device)."""
    require_gpu()
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


# One end-of-epoch criterion of run_training.  run(mean training loss of the epoch) -> metrics; score(metrics) -> a number, lower
# is better; lines(metrics, whether this epoch is the best so far) -> the lines to print; ckpts: the (file name, module) pairs
# saved on a new best, or None for the entry point's own list, in place of the training-loss criterion.
Validator = collections.namedtuple("Validator", "run score lines ckpts")
TRAINING_LOSS = Validator(lambda loss: loss, lambda loss: loss, lambda loss, is_best: (), None)


def epoch_end_entries(ckpt_names, validators=()):
    """The entries end_epoch runs, in order.  The first one saves ``ckpt_names``: a validator with ``ckpts=None`` at the head of
    the list (the reference's validate(), train.py:238-247), else the best training loss, which prints nothing.  A file name
    that a later entry claims leaves the first entry's list: it is saved on that entry's criterion alone."""
    entries = list(validators)
    if not entries or entries[0].ckpts is not None:
        entries.insert(0, TRAINING_LOSS)
    claimed = {fname for v in entries[1:] for fname, _ in v.ckpts}
    entries[0] = entries[0]._replace(ckpts=[c for c in ckpt_names if c[0] not in claimed])
    return entries


def end_epoch(entries, best, train_loss, save):
    """Run every entry once: print its lines, and on a score below ``best[i]`` (one per entry, updated in place) hand its
    checkpoints to ``save``.  Needs no GPU of its own."""
    for i, v in enumerate(entries):
        metrics = v.run(train_loss)
        score = v.score(metrics)
        is_best = score < best[i]
        for line in v.lines(metrics, is_best):
            print(line, flush=True)
        if is_best:
            best[i] = score
            save(v.ckpts)


def run_training(args, nets, loss_fn, lr, betas, weight_decay, term_names, ckpt_names, n_views=2, validators=()):
    """Epoch loop.  ``loss_fn(batch) -> (loss, terms)``; ``nets``: list of modules in optimizer-group order.
    ``validators`` (rank 0, optional): Validator entries run after every epoch (epoch_end_entries / end_epoch); without one
    ``ckpt_names`` are saved on the best training loss."""
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
    entries = epoch_end_entries(ckpt_names, validators)
    best = [float("inf")] * len(entries)
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
            # (eager launches between graph replays; a geometry first seen here gets its packed weights like any other)
            end_epoch(entries, best, means[0], lambda ckpts: save_best(args.output_dir, ckpts))
    if world > 1:
        dist.destroy_process_group()
