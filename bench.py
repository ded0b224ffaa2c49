#!/usr/bin/env python3
"""Headline benchmark: KITTI 256x832 stereo-sequence training samples/sec (forward + backward + Adam) on synthetic data.

    python bench.py --gpus N --steps K --warmup W [--config {2,3,4,5}] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        bench.py --gpus N --steps K --warmup W

Default workload = BASELINE.json configs[1] (SURVEY.md section 8d cfg 2): DispNetS + PoseExpNet joint step, spatial +
temporal photometric loss + 10*smooth, 256x832, batch 4 per GPU.  --config selects the other single-GPU-sized cases:
  3  + FeatExtractor on the three frames and 0.1 * feature reconstruction (C=32 warps, all gradients), batch 8
  4  train.py's 4-scale body (masks, smooth, stereo-pose MSE) + the feature term, batch 4 per GPU (32 on 8 GPUs)
  5  384x1280, five-frame window (nb_ref_imgs = 4), 4 scales, batch 8 per GPU (64 on 8 GPUs)

One process per GPU (RCCL = torch.distributed backend "nccl"); weak scaling: every rank runs the per-GPU batch, gradients
are sum-all-reduced over flat arena buckets during backward and averaged inside the fused Adam.  Started WITHOUT a
launcher, `--gpus N` (N > 1) spawns the N rank processes itself before any GPU call.  Rank 0 prints ONE JSON line:
`value` counts samples of all ranks over the slowest rank's time; `roofline*` objects come from HIP-event brackets around
every kernel call of one serialised step measured live (`roofline` = the calls whose plan ran conv_pipe_kernel, attributed
through the library's plan log; `conv_calls_by_kernel` lists every kernel family); `host_enqueue_ms` is the host time to
enqueue one step; `cpu_baseline` is the CPU oracle timed on this host.  `ms_per_step` is the wall time of one of the K
timed steps.  Inputs and initial weights are seeded, so the same arguments give the same inputs in every run;
`--dump-outputs DIR` writes the loss terms, weight gradients and updated weights of one more step from that seeded
state, through the eager step on the timed loop's streams, there after the timed steps (see dump_outputs)."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "depth-vo-feat_amd"))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_HBM_GBPS = 8000.0             # MI355X_MICROARCH.md: HBM3E spec (6.3 TB/s achievable)

CONFIGS = {
    2: dict(batch=4, height=256, width=832, body="unsupervise", feat=False, nb_ref=2,
            name="cfg2: DispNetS+PoseExpNet joint step, spatial+temporal photometric (V=2) + 10*smooth, Adam"),
    3: dict(batch=8, height=256, width=832, body="unsupervise", feat=True, nb_ref=2,
            name="cfg3: cfg2 + FeatExtractor on 3 frames + 0.1*feature reconstruction (C=32, V=2, all gradients), Adam"),
    4: dict(batch=4, height=256, width=832, body="train_sfm", feat=True, nb_ref=2,
            name="cfg4: DispNetS+PoseExpNet_sfm+FeatExtractor, 4-scale photometric with masks + 0.1*smooth + stereo-pose "
                 "MSE + 0.1*feature reconstruction, Adam"),
    5: dict(batch=8, height=384, width=1280, body="train_sfm", feat=False, nb_ref=4,
            name="cfg5: DispNetS+PoseExpNet_sfm(nb_ref_imgs=4), five-frame window, 4-scale photometric with masks (V=4) + "
                 "0.1*smooth + stereo-pose MSE, Adam"),
}


REAL_STDOUT = sys.stdout


def count_gpus_sysfs():
    """GPUs of this host counted WITHOUT touching the HIP/HSA runtime: KFD topology nodes with SIMDs (CPU nodes have
    simd_count 0).  Returns None when the topology is not readable (then the rank processes find out for themselves)."""
    base = "/sys/class/kfd/kfd/topology/nodes"
    try:
        n = 0
        for node in os.listdir(base):
            with open(os.path.join(base, node, "properties")) as f:
                for line in f:
                    k, _, v = line.partition(" ")
                    if k == "simd_count" and int(v) > 0:
                        n += 1
        return n
    except OSError:
        return None


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N rank processes (one per GPU) ourselves.  This parent
    makes NO GPU-runtime call -- not even a device count through torch, which loads HIP/HSA: on this pool a process that
    has initialised the GPU must not exec another program, and the ranks are fork+exec'd from here.  It polls all ranks:
    the first one to fail takes the others down (a crashed rank would otherwise leave its peers in the rendezvous or in a
    collective until their timeout); it relays rank 0's JSON line and exits with the worst return code."""
    import time
    have = count_gpus_sysfs()
    if have is not None and have < n:
        sys.exit(f"bench.py: --gpus {n} but this host exposes {have} GPU(s)")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    out_path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"dvf_bench_rank0_{os.getpid()}.json")
    with open(out_path, "wb") as out0:
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=out0 if r == 0 else subprocess.DEVNULL))
    rcs = [None] * n
    failed = False
    while any(rc is None for rc in rcs):
        for i, p in enumerate(procs):
            if rcs[i] is None:
                rcs[i] = p.poll()
                if rcs[i] not in (None, 0) and not failed:
                    failed = True
                    for q in procs:                     # exactly the processes started above
                        if q.poll() is None:
                            q.terminate()
        time.sleep(0.05)
    with open(out_path, "rb") as f:
        REAL_STDOUT.write(f.read().decode())
    REAL_STDOUT.flush()
    os.unlink(out_path)
    sys.exit(max(abs(rc) for rc in rcs))


def build(args, cfg, device, world, rank):
    import torch
    import DispNetS
    from dvf.engine import FlatAdam
    from dvf import steps as S
    from dvf.synthetic import synthetic_batch
    torch.manual_seed(args.seed)
    nets = []
    disp_net = DispNetS.DispNetS()
    if cfg["body"] == "unsupervise":
        import PoseExpNet
        pose_net = PoseExpNet.PoseExpNet(output_exp=True)
    else:
        import PoseExpNet_sfm
        pose_net = PoseExpNet_sfm.PoseExpNet(nb_ref_imgs=cfg["nb_ref"], output_exp=True)
    feat_net = None
    if cfg["feat"]:
        import feat_extractor
        feat_net = feat_extractor.FeatExtractor()
    nets = [pose_net, disp_net] + ([feat_net] if feat_net is not None else [])
    for n in nets:
        n.init_weights()
        n.to(device).train()
    batch = synthetic_batch(args.batch, args.height, args.width, seed=1234, rank=rank, device=device, n_views=cfg["nb_ref"])
    ddp = world > 1 or args.force_ddp
    params = [p for n in nets for p in n.parameters()]
    if cfg["body"] == "unsupervise":      # unsupervise.py:241  Adam(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-8)
        opt = FlatAdam(params, lr=1e-3, weight_decay=1e-8, world_size=world, overlap=args.no_graph, always_reduce=ddp,
                       collective=getattr(args, "collective", "all_reduce"))
    else:                                 # train.py:150-156  Adam(lr=2e-4, betas=(0.9, 0.999), weight_decay=0)
        opt = FlatAdam(params, lr=2e-4, weight_decay=0.0, world_size=world, overlap=args.no_graph, always_reduce=ddp,
                       collective=getattr(args, "collective", "all_reduce"))

    def fwd_bwd():
        if cfg["body"] == "unsupervise":
            loss, terms = S.unsupervise_losses(disp_net, pose_net, batch, feat_extractor=feat_net)
        else:
            loss, terms = S.train_sfm_losses(disp_net, pose_net, batch, feat_extractor=feat_net)
        opt.zero_grad()
        loss.backward()
        opt.join_wgrad()                # weight-gradient stream joins the main stream
        return terms["total"], terms    # detached loss terms

    def step():
        out = fwd_bwd()
        opt.step()                      # (gradient all-reduce +) fused Adam
        return out

    named_nets = {"pose": pose_net, "disp": disp_net}
    if feat_net is not None:
        named_nets["feat"] = feat_net
    return step, fwd_bwd, opt, ddp, named_nets


DUMP_SAMPLE = 1 << 18                   # elements kept of a larger tensor by --dump-outputs (<= 51 MB in all)
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, terms, nets):
    """--dump-outputs: what one training step computed -- every loss term, and of every network parameter its weight
    gradient and its value after the Adam update -- as <path>/<name>.npy in float32.  A tensor of more than DUMP_SAMPLE
    elements is represented by DUMP_SAMPLE of them, at sorted indices drawn from a fixed seed (flattened, the same for
    the value and the gradient), so that two builds compare element for element and every config stays under 64 MB.
    main() runs that step after the timed steps, from the seeded initial state, as the eager step on the timed loop's streams
    with ordered weight-gradient and bias reductions (dvf.conv.set_deterministic): its inputs are
    the same in every run and so are these arrays.  The last timed step's own arrays are not written: they start from
    weights that the float-atomic rounding of all earlier steps has moved differently in every run."""
    import numpy as np
    import torch
    arrays = {"loss_" + k: v.detach().float().cpu().numpy() for k, v in terms.items()}
    for net_name, net in nets.items():
        for k, p in net.named_parameters():
            idx = None
            if p.numel() > DUMP_SAMPLE:
                g = torch.Generator().manual_seed(0)
                idx = torch.randperm(p.numel(), generator=g)[:DUMP_SAMPLE].sort().values.to(p.device)
            for kind, v in (("param", p.detach()), ("grad", p._dvf_grad)):    # _dvf_grad: its slice of the gradient arena
                arrays[f"{kind}_{net_name}.{k}"] = (v if idx is None else v.reshape(-1)[idx]).float().cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return len(arrays), total


def pmc_traffic(kernel):
    """HBM-side bytes per launch of `kernel` from the committed PMC summary (separate rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE passes over this same command; corrections as calibrated in that file).  PMC passes cannot run inside the
    timed process, so the bench line QUOTES the committed measurement (see `traffic_source`)."""
    try:
        with open(os.path.join(ROOT, "profiles", TRAFFIC_FILE)) as f:
            ks = json.load(f)["kernels"]
        names = {"conv_fwd_dgrad": ["conv_pipe", "conv_gather"], "conv_wgrad": ["wgrad_pipe", "conv_wgrad"]}.get(kernel, [kernel])
        ks = [ks[n] for n in names if n in ks]
        if not ks:
            return None
        return sum(k["read_bytes_per_step"] + k["write_bytes_per_step"] for k in ks) / sum(k["launches_per_step"] for k in ks)
    except (OSError, KeyError, ValueError):
        return None


TRAFFIC_FILE = next((f for f in ("r03_traffic.json", "r02b_traffic.json", "r02_traffic.json", "r01_traffic.json") if os.path.exists(os.path.join(ROOT, "profiles", f))), "r01_traffic.json")


def measure_kernels(step):
    """One eager step with HIP-event brackets around every C-ABI call (dvf.lib.KernelTimer), SERIALISED: the weight-
    gradient side stream and the pose-network stream are switched off for this pass, so a bracket times the kernels of
    one call alone (in the timed region they overlap, which is why `value` is better than the sum of these times)."""
    from dvf import lib as L
    L.SERIALIZE = True
    step()                              # (first serialised pass: allocator warm-up, not recorded)
    # (the brackets measure the GPU side: enqueueing the recorded pass behind a 25 ms device-side delay, so that every kernel
    # is dispatched back to back, changed no quotient by more than 2 % -- a bracket costs ~6 us of marker processing, which
    # is the difference to rocprofv3's per-kernel durations in profiles/)
    L.TIMER = L.KernelTimer()
    step()
    summ = L.TIMER.summary()
    if os.environ.get("DVF_CALL_LOG"):
        # calls of the recorded pass in launch order (tools/r3/launch_table.py joins them with a rocprofv3 kernel trace)
        with open(os.environ["DVF_CALL_LOG"], "w") as f:
            for kind, ea, eb, fl, by, tag, fam, kernels in L.TIMER.records_with_kernels():
                f.write(json.dumps({"kind": kind, "tag": tag, "family": fam, "flops": fl, "bytes": by, "event_ms": ea.elapsed_time(eb),
                                    "kernels": kernels}) + "\n")
    L.SERIALIZE = False
    if os.environ.get("DVF_LAYER_TABLE"):
        for ms, kind, tag, tf, gb in L.TIMER.table()[:int(os.environ["DVF_LAYER_TABLE"])]:
            print(f"  {ms:8.3f} ms  {kind:11s} {tf:7.2f} TF/s {gb:8.1f} GB/s  {tag}", file=sys.stderr)
    L.TIMER = None
    return summ


def host_cores():
    """Cores this process may actually use: the cgroup CPU quota when there is one (the GPU box exposes 256
    logical CPUs but grants a 16-CPU share), else the affinity mask."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline():
    """the CPU oracle (plain torch CPU restatement of the reference path, pinned to the reference by
    tests/golden) on this host's cores -- config 1 EXACTLY (DispNetS depth-only, stereo photometric L1 + 10*smooth,
    128x416, batch 1, forward + backward + Adam), min of >= 5 iterations after 2 warm-ups, plus the config-2 loss-only
    micro-benchmark (2 image warps + smooth, 256x832, batch 4, forward + backward).  Bounded to ~10-20 s."""
    import torch
    from oracle import nets as onets
    from oracle import steps as osteps
    nthreads = host_cores()
    torch.set_num_threads(nthreads)
    dsd = onets.fill_params(onets.dispnet_layers(), seed=1)
    batch = osteps.synthetic_batch(1, 128, 416, seed=1234)
    st = None
    for _ in range(2):
        _, _, st = osteps.step_depth_only(dsd, batch, st)
    times, t_all = [], time.perf_counter()
    while len(times) < 5 or (time.perf_counter() - t_all < 8.0 and len(times) < 30):
        t0 = time.perf_counter()
        _, _, st = osteps.step_depth_only(dsd, batch, st)
        times.append(time.perf_counter() - t0)
    # loss-only micro-benchmark
    b4 = osteps.synthetic_batch(4, 256, 832, seed=1234)
    g = torch.Generator().manual_seed(7)
    depth = torch.rand(4, 256, 832, generator=g) * 20 + 2
    T = torch.randn(4, 6, generator=g) * 0.01
    osteps.loss_only(b4, depth, T)
    lt = []
    for _ in range(5):
        t0 = time.perf_counter()
        osteps.loss_only(b4, depth, T)
        lt.append(time.perf_counter() - t0)
    return {"value": 1.0 / min(times), "unit": "samples/s", "cores": nthreads, "kind": "port", "cpu": cpu_model(),
            "sample": f"config 1 exactly: DispNetS depth-only, stereo photometric L1 + 10*smooth, 128x416, batch 1, "
                      f"fwd+bwd+Adam, torch CPU fp32, {nthreads} threads; min of {len(times)} iterations after 2 warm-ups "
                      f"({1e3 * min(times):.0f} ms)",
            "loss_only": {"value": 4.0 / min(lt), "unit": "samples/s",
                          "sample": f"config-2 loss only: 2 image warps (C=3) + smooth, 256x832, batch 4, fwd+bwd, min of 5 "
                                    f"({1e3 * min(lt):.0f} ms)"}}


def main():
    # stdout carries exactly ONE JSON line (the driver's contract).  The GPU boxes export NCCL_DEBUG=VERSION, which makes RCCL
    # printf its version banner to stdout at the first collective (NCCL_DEBUG_FILE does not move it): file descriptor 1 is
    # pointed at stderr for the whole run and the JSON line goes to a saved copy of the real stdout.
    global REAL_STDOUT
    sys.stdout.flush()
    REAL_STDOUT = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", type=int, default=2, choices=sorted(CONFIGS), help="workload (SURVEY.md section 8d); default 2 = the headline")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default: the config's)")
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--graph", action="store_true", help="replay the whole step from one HIP graph")
    ap.add_argument("--no-graph", action="store_true", help="eager launches on three streams")
    # default (neither flag, one GPU): both are built, each is timed for a few untimed steps, the faster one is used --
    # which of the two wins depends on how fast the host enqueues the ~360 launches of a step
    ap.add_argument("--force-ddp", action="store_true", help="run the multi-GPU exchange path even with one rank")
    ap.add_argument("--collective", choices=("all_reduce", "rs_ag"), default="all_reduce",
                    help="bucket exchange: one RCCL all-reduce, or reduce-scatter + all-gather in place (the direct all-links "
                         "form of SURVEY section 8e) -- to be A/B'd on an 8-GPU node")
    ap.add_argument("--graph-ddp", action="store_true",
                    help="multi-GPU: replay forward+backward from a HIP graph and all-reduce afterwards (no overlap); "
                         "default for N>1 is eager launches with the all-reduce overlapped with backward")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--serialize", action="store_true",
                    help="no side streams (weight gradients, pose network) -- for per-kernel profiles; not the headline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after an eager timed loop, run one more eager step from the seeded initial state on the timed loop's "
                         "streams, with ordered gradient reductions, and write its loss terms, weight gradients and "
                         "updated weights (a fixed sample of the large ones) to DIR/<name>.npy, to compare two builds "
                         "output for output")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    cfg = CONFIGS[args.config]
    for k in ("batch", "height", "width"):
        if getattr(args, k) is None:
            setattr(args, k, cfg[k])

    if args.gpus > 1 and "RANK" not in os.environ:
        spawn_ranks(args.gpus)            # (does not return)

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus} or without a launcher")
    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X: the product path has no CPU fallback")
    if local_rank >= torch.cuda.device_count():
        sys.exit(f"bench.py: rank {rank} wants GPU {local_rank}, this host exposes {torch.cuda.device_count()}")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1 or args.force_ddp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    def log(msg):
        if rank == 0:
            print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    if args.serialize:
        from dvf import lib as _L
        _L.SERIALIZE = True
    log("building models (config %d)" % args.config)
    auto = not args.graph and not args.no_graph and world == 1 and not args.force_ddp and not args.serialize
    if world > 1 or args.force_ddp:
        args.no_graph = not args.graph_ddp
    elif not args.graph:
        args.no_graph = True
    step, fwd_bwd, opt, ddp, nets = build(args, cfg, device, world, rank)
    if args.dump_outputs:                 # the seeded state the --dump-outputs step starts from
        initial_params, initial_opt = opt.flat_p.clone(), opt.state_dict()
    use_graph = not args.no_graph
    from dvf.engine import GraphedStep
    if auto:
        def clock(fn, k=6):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(k):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / k
        # eager is probed before AND after the graph (a fresh process / cold clocks made the first probe read slow once, and
        # the graph -- ~10 % slower in steady state -- was picked); the graph must win by 5 %
        t_eager = min(clock(step), clock(step))
        graphed = GraphedStep(step, [], warmup=1)
        t_graph = min(clock(graphed), clock(graphed))
        t_eager = min(t_eager, clock(step))
        use_graph = t_graph < 0.95 * t_eager
        log("launch mode: eager %.2f ms/step, HIP graph %.2f ms/step -> %s" % (1e3 * t_eager, 1e3 * t_graph,
                                                                            "graph" if use_graph else "eager"))
        run = graphed if use_graph else step
    elif use_graph:
        log("eager step 1")
        step()
        torch.cuda.synchronize()
        log("capturing HIP graph")
        if not ddp:
            run = GraphedStep(step, [], warmup=1)              # whole step: forward + backward + Adam
        else:
            # forward + backward replay from the graph; the RCCL all-reduce of the gradient arena and the fused
            # Adam are enqueued behind it on the same stream (collectives are not captured)
            graph = GraphedStep(fwd_bwd, [], warmup=0)

            def run():
                out = graph()
                opt.step()
                return out
    else:
        run = step
    if args.dump_outputs and use_graph:
        # the seeded step does not repeat after a graph-timed loop (its gradients differ from run to run and from the
        # eager step's): no dump rather than a wrong one
        sys.exit("bench.py: --dump-outputs needs an eager timed loop (--no-graph, or the default launch mode picking eager)")
    log("warm-up")
    for _ in range(args.warmup):
        out = run()
    torch.cuda.synchronize()
    log("timing")

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    fence()
    t0 = time.perf_counter()
    host = 0.0
    for _ in range(args.steps):
        h0 = time.perf_counter()
        out = run()
        host += time.perf_counter() - h0       # host time to ENQUEUE the step (no synchronisation inside run())
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    loss = float(out[0])
    if args.dump_outputs:
        # One more step, from the seeded initial state, through the eager step on the timed loop's streams (side streams,
        # early per-bucket Adam on the update stream).  After the timed steps the weights depend on how each step's
        # float-atomic weight-gradient and bias sums happened to round, and Adam carries that into them, so the last timed
        # step's arrays differ from run to run by up to their whole range.  This step differs from an eager timed one only
        # in using the library's ordered reductions for those sums, so that it writes the same arrays in every run.  Every
        # rank runs it (it holds the gradient exchange).
        from dvf import conv as _C
        from dvf import lib as _L
        _C.set_deterministic(True)
        try:
            opt.flat_p.copy_(initial_params)
            opt.load_state_dict(initial_opt)
            _L.PACK_EPOCH += 1                                 # packed weight copies are rebuilt from the restored weights
            dumped = step()
            fence()
        finally:
            _C.set_deterministic(False)
        if rank == 0:
            n, nbytes = dump_outputs(args.dump_outputs, dumped[1], nets)
            log("dumped %d arrays (%.1f MB) to %s" % (n, nbytes / 2**20, args.dump_outputs))

    # the data-parallel exchange on its own: the gradient arena all-reduced in the step's buckets, nothing overlapping it
    allreduce_ms = None
    if ddp:
        fence()
        t1 = time.perf_counter()
        for _ in range(5):
            for b in opt.buckets:
                opt._exchange(b, opt.flat_g[b["start"]:b["end"]])
        fence()
        allreduce_ms = 1e3 * (time.perf_counter() - t1) / 5

    result = None
    if rank == 0:
        samples = args.batch * world * args.steps
        result = {
            "metric": "KITTI 256x832 stereo-seq samples/sec fwd+bwd", "value": samples / dt, "unit": "samples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s; %dx%d, batch %d per GPU" % (cfg["name"], args.height, args.width, args.batch),
                       "global_batch": args.batch * world, "parallelism": "dp%d" % world,
                       "launch": ("hipgraph" if use_graph else "eager") + ("+rccl-allreduce" if ddp else "")},
            "final_loss": loss,
            # host time spent enqueueing a step (Python + ctypes + launches, main thread; autograd's thread runs beside it):
            # when it approaches ms_per_step the run is host-bound -- at N ranks on a shared CPU quota this is the number to watch
            "host_enqueue_ms": 1e3 * host / args.steps,
        }
        if ddp:
            result["rccl_world_size"] = dist.get_world_size()
            result["config"]["collective"] = opt.collective
            result["allreduce_ms_per_step"] = allreduce_ms
            result["allreduce_bytes_per_step"] = 4 * int(opt.total)
            result["allreduce_note"] = ("gradient arena in %d buckets, measured alone after the timed region; inside a step it "
                                        "runs on the communication stream under backward" % len(opt.buckets))
    log("timed region done: %.2f ms/step" % (1e3 * dt / args.steps))
    ks = None
    if not args.no_kernel_timing:
        # every rank runs the extra eager steps (they contain the gradient all-reduce); rank 0 records
        if rank == 0:
            ks = measure_kernels(step)
        else:                               # the same two serialised steps (same schedule, same collective order) on every rank
            from dvf import lib as _Lr
            _Lr.SERIALIZE = True
            step()
            step()
            _Lr.SERIALIZE = False
    if rank == 0 and ks is not None:
        def fam_sum(keys):
            ms = sum(ks.get(k, {}).get("ms", 0) for k in keys)
            fl = sum(ks.get(k, {}).get("flops", 0) for k in keys)
            calls = sum(ks.get(k, {}).get("calls", 0) for k in keys)
            return ms, fl, calls

        # the dominant kernel: conv_pipe_kernel (every forward / dgrad call whose plan ran it; a call = the launch plus its
        # split-K reduce where the plan splits K).  The 1-2 channel disparity heads and the <=16-channel layers run other,
        # HBM-bound kernels: they are listed beside it, not inside its MFMA quotient.
        g_ms, g_fl, g_calls = fam_sum(["conv_fwd/pipe", "conv_dgrad/pipe"])
        a_ms, a_fl, a_calls = fam_sum(["conv_fwd", "conv_dgrad"])
        ach = g_fl / (g_ms * 1e-3) / 1e12 if g_ms > 0 else 0.0
        quoted = args.config == 2 and args.batch == 4
        result["roofline"] = {"kernel": "conv_pipe_kernel (Conv2d/ConvTranspose2d forward + dgrad; a call = the launch plus its "
                                        "split-K reduce where used)",
                              "bound": "mfma", "achieved": ach, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                              "frac": ach / PEAK_FP32_MFMA_TFLOPS, "traffic": pmc_traffic("conv_pipe") if quoted else None,
                              "traffic_source": ("profiles/%s: HBM-side bytes per launch from separate rocprofv3 --pmc passes of "
                                                 "this command (committed; not measured in this run)" % TRAFFIC_FILE) if quoted else None,
                              "calls_per_step": g_calls, "ms_per_step": g_ms,
                              "all_fwd_dgrad_calls": {"calls_per_step": a_calls, "ms_per_step": a_ms,
                                                      "achieved": a_fl / (a_ms * 1e-3) / 1e12 if a_ms > 0 else 0.0,
                                                      "note": "every forward + dgrad call, the head / narrow-layer kernels "
                                                              "included (round 1-2 definition of this object)"},
                              }
        result["conv_calls_by_kernel"] = {k: {"calls": v["calls"], "ms": round(v["ms"], 4),
                                              "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 else 0.0}
                                          for k, v in sorted(ks.items()) if "/" in k}
        w = ks.get("conv_wgrad", {})
        if w.get("ms", 0) > 0:
            a = w["flops"] / (w["ms"] * 1e-3) / 1e12
            wp = ks.get("conv_wgrad/wgrad_pipe", {})
            result["roofline_wgrad"] = {"kernel": "every weight-gradient call: wgrad_pipe_kernel (+ head_wgrad_kernel for the 1-2 channel heads); "
                                                  "wgrad_pipe_kernel alone: %.1f TFLOP/s over %d calls"
                                                  % (wp.get("flops", 0) / max(wp.get("ms", 0), 1e-9) / 1e9, wp.get("calls", 0)),
                                        "bound": "mfma", "achieved": a,
                                        "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": a / PEAK_FP32_MFMA_TFLOPS,
                                        "traffic": pmc_traffic("conv_wgrad") if quoted else None, "calls_per_step": w["calls"],
                                        "ms_per_step": w["ms"]}
        p_ms = ks.get("photo_fwd", {}).get("ms", 0) + ks.get("photo_bwd", {}).get("ms", 0)
        p_by = ks.get("photo_fwd", {}).get("bytes", 0) + ks.get("photo_bwd", {}).get("bytes", 0)
        if p_ms > 0:
            a = p_by / (p_ms * 1e-3) / 1e9
            result["roofline_warp"] = {"kernel": "photo_fwd_kernel + photo_bwd_kernel (fused warp + photometric L1, all "
                                                 "scales and the feature term of the step)",
                                       "bound": "hbm", "achieved": a, "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                                       "frac": a / PEAK_HBM_GBPS,
                                       "traffic": ((pmc_traffic("photo_fwd") or 0) + (pmc_traffic("photo_bwd") or 0) or None) if quoted else None,
                                       "algorithmic_bytes": p_by, "ms_per_step": p_ms,
                                       "note": "algorithmic bytes assume every target pixel samples inside the source images; a "
                                               "pixel projected out of view reads no source bytes, so on degenerate (random-"
                                               "init) geometry the quotient overstates the traffic and can exceed the HBM peak "
                                               "-- profiles/r02_photo_bench.txt has the kernels on KITTI-like geometry",
                                       "calls_per_step": ks.get("photo_fwd", {}).get("calls", 0) + ks.get("photo_bwd", {}).get("calls", 0)}
        result["kernel_ms_per_step"] = {k: round(v["ms"], 4) for k, v in sorted(ks.items()) if "/" not in k and not k.startswith("_")}
    if world > 1:
        dist.barrier()
    if rank == 0 and world == 1 and not args.force_ddp and not args.no_cpu_baseline:
        log("cpu baseline")
        result["cpu_baseline"] = cpu_baseline()
    if rank == 0:
        print(json.dumps(result), file=REAL_STDOUT)
        REAL_STDOUT.flush()
    if world > 1 or args.force_ddp:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
