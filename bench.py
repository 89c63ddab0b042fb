#!/usr/bin/env python3
"""Headline benchmark: images/sec of the U-Net 256x256 forward+backward (seg loss included, optimiser
step and data loading excluded) on N MI355X, one process per GPU.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N ...        # no launcher: this process (which never touches a GPU) starts the N ranks itself
    python bench.py --gpus 2 --backend gloo --dry    # CPU rehearsal of the launcher / rendezvous / reducer plumbing only

Workload (BASELINE.json configs[1]): unet.UNet(n_channels=1, n_classes=2), 256x256, batch 32 PER GPU
(weak scaling), synthetic images/masks resident in HBM, random-init weights, loss = CrossEntropy +
multiclass Dice (the n_classes=2 form of train_end2end_jsrt.py:181-183).  Data parallel: RCCL all-reduce
(average) of the 31 M gradients, bucketed and overlapped with backward.

One JSON line on rank 0.  A plain run sets up, warms up, times the K steps and prints the headline figures
(`value`, `ms_per_step`, ...); everything else is measured only with --full (null in a plain run):
`roofline` and `kernels` are for the MFMA kernels, measured live with HIP events on the launch stream inside
the timed region: achieved = algorithmic FLOPs (2*M*N*K of the convolutions it ran) / its summed launch time.
`fast_mode` is a second timed leg in the fast 16-bit mode (N=1).  `cpu_baseline` is the CPU oracle (a port,
oracle/oracle.py) timed on the host cores of this box on a bounded sample (batch 4), N=1 only.  N>1 adds the
un-overlapped all-reduce time and a leg without the gradient exchange.

--dump-outputs DIR writes what the last timed step computed (rank 0): logits.npy, loss.npy and one
grad.<parameter>.npy per parameter (float32, the loss float64; logits above DUMP_MAX_LOGITS and gradients above
DUMP_MAX_ELEMS elements as a fixed seeded sample; DUMP_MAX_BYTES in all).
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# numerics modes: (description, asserted bound on max |logit - fp32 reference logit|, where it is asserted)
PARITY_MODES = {
    "fast": ("fast (single 16-bit storage; UNet(precise=False) / GSSEG_PRECISE=0)", 5e-3, "tests/test_unet_gpu.py::test_unet_step_vs_golden"),
    "mixed": ("mixed = what UNet() builds (hi/lo pairs everywhere, correction MFMA segments on the 9 stages that make the 16-bit error)", 1e-3,
              "tests/test_unet_gpu.py::test_mixed_mode_meets_1e3_*, test_config2_bs32_256_vs_reference_fixture[mixed]"),
    "full": ("precise (hi/lo 16-bit pairs, three MFMA segments everywhere)", 3e-5,
             "tests/test_unet_gpu.py::test_precise_mode_meets_the_north_star_bound_vs_golden"),
}
GF_PER_IMG_FWDBWD = {1: 288.48, 2: 288.50}     # conv/convT 2*MACs, 256x256
MFMA_PEAK_TFLOPS = 2500.0                      # dense bf16/fp16, MI355X_MICROARCH.md
MFMA_SUSTAINED_TFLOPS = 1560.0                 # tools/mfma_peak.hip on this part: 32x32x16 f16, random operands
HBM_PEAK_GBS = 8000.0
DUMP_MAX_ELEMS = 1 << 18                       # per dumped gradient: 1 MiB of float32 (the U-Net's 64 gradients: 19 MiB)
DUMP_MAX_LOGITS = 1 << 23                      # dumped logits: 32 MiB of float32 (the default 32x2x256x256 are written whole)
DUMP_MAX_BYTES = 64 << 20


# KernelTimer class -> kernel-name prefix in the committed rocprofv3 PMC summary (tools/profile_step.sh)
PMC_PREFIX = {"conv3x3_halo": "conv3x3_", "wgrad3x3_halo": "wgrad3x3_", "igemm_fwd": "igemm_fwd_kernel",
              "igemm_wgrad": "igemm_wgrad_kernel"}


def source_sha16():
    """sha256 over the kernel sources (csrc/*.hip, *.hpp, *.cpp): tools/pmc_summary.py stamps it into the PMC summaries, so a
    `roofline.traffic` taken from a profile of OTHER kernels is flagged (traffic_current: false) instead of going stale silently."""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "semantic_segmentation_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")) + glob.glob(os.path.join(csrc, "*.cpp"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(kind):
    """HBM bytes per launch of a kernel class, from the newest committed PMC summary under profiles/
    (FETCH_SIZE x2 + WRITE_SIZE, launch-weighted over the class's template instances).  PMC counters cannot be
    collected from inside this process, so this is the figure of the profiled run of the same command."""
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_traffic.json")),      # newest by name, numbers compared as numbers (r04_v10 > r04_v2)
                   key=lambda p: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", os.path.basename(p))])
    pre = PMC_PREFIX.get(kind)
    if not files or pre is None:
        return None, None, None
    # a summary taken with exactly these kernel sources wins over a newer-named one of other sources
    cur = source_sha16()
    pick = files[-1]
    for p in reversed(files):
        try:
            with open(p) as f:
                if json.load(f).get("_source_sha16") == cur:
                    pick = p
                    break
        except (OSError, ValueError):
            continue
    files = [pick]
    with open(files[-1]) as f:
        d = json.load(f)
    sha = d.get("_source_sha16")
    n, b = 0.0, 0.0
    for k, v in d.items():
        if k.startswith(pre) and isinstance(v, dict) and v.get("write_MB_per_launch") is not None:
            n += v["launches_per_step"]
            b += v["launches_per_step"] * (v["fetch_MB_per_launch_corrected"] + v["write_MB_per_launch"]) * 1e6
    return (round(b / n, 0), os.path.relpath(files[-1], ROOT), sha) if n else (None, None, None)


def kernel_table(ksum, steps):
    """Per kernel class of ops.KernelTimer: launches, time, algorithmic TFLOP/s and bytes per launch.  The pair forward's conv
    launches (class conv3x3_halo_precise: the same kernel with K = the stage's segment concatenation) belong to the conv3x3
    family: they are merged into `conv3x3_halo` -- achieved = the convolution's ALGORITHMIC 2*M*N*K over the family's summed time,
    however many MFMA segments a launch executed -- and listed once more as the sub-entry `conv3x3_halo.pair_forward`."""
    merged = {}
    for kind, d in ksum.items():
        fam = "conv3x3_halo" if kind == "conv3x3_halo_precise" else ("igemm_fwd" if kind == "igemm_fwd_precise" else kind)
        m = merged.setdefault(fam, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
        for k in m:
            m[k] += d[k]
        if fam != kind:
            merged[fam + ".pair_forward"] = dict(d)
    kern = {}
    for kind, d in merged.items():
        tf = d["flops"] / (d["ms"] * 1e-3) / 1e12 if d["ms"] > 0 else 0.0
        kern[kind] = {"launches_per_step": d["launches"] / steps, "ms_per_step": round(d["ms"] / steps, 4),
                      "avg_launch_us": round(d["ms"] / d["launches"] * 1e3, 2), "tflops": round(tf, 1),
                      "tflop_per_step": round(d["flops"] / steps / 1e12, 4),
                      "algorithmic_bytes_per_launch": round(d["bytes"] / d["launches"], 0)}
    return kern


def family_summary(ksum, steps):
    k = kernel_table(ksum, steps).get("conv3x3_halo")
    return None if k is None else dict(k, frac_of_mfma_peak=round(k["tflops"] / MFMA_PEAK_TFLOPS, 4))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="per-GPU batch")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--dtype", default=os.environ.get("GSSEG_DTYPE", "f16"), choices=["f16", "bf16"])
    ap.add_argument("--precise", nargs="?", const="full", default="mixed", choices=["full", "mixed", "fast"],
                    help="numerics mode of the headline leg (`value`, `ms_per_step`, `roofline`, `kernels`).  Default 'mixed': what "
                         "UNet() builds and the mode whose asserted bound meets the north star's 1e-3 on logits; 'full': three MFMA "
                         "segments everywhere (~1e-5); 'fast': single 16-bit storage (~4e-3, outside the tolerance)")
    ap.add_argument("--full", action="store_true",
                    help="measure everything besides the headline: per-kernel table and roofline (HIP events around the kernels of "
                         "the timed steps), the fast_mode leg, the CPU baseline, and at N>1 the un-overlapped all-reduce and a leg "
                         "without the gradient exchange")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (logits, loss, parameter gradients) as DIR/<name>.npy")
    ap.add_argument("--fast-leg", default="fast", choices=["fast", "none"],
                    help="with --full: second timed leg at N=1 in the fast 16-bit mode, reported as \"fast_mode\" with its own "
                         "(out-of-tolerance) bound next to the headline value (none: skip it, e.g. under rocprofv3)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--global-dice", action="store_true",
                    help="exact global-batch Dice across ranks (all-reduce of three scalars); default: per-rank Dice")
    ap.add_argument("--host-input", action="store_true",
                    help="PCIe-inclusive variant: copy the batch from pinned host memory inside every timed step")
    ap.add_argument("--cpu-batch", type=int, default=4)
    ap.add_argument("--cpu-steps", type=int, default=2)
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="gloo only with --dry")
    ap.add_argument("--rehearse-dp", action="store_true",
                    help="N = 1 only: run the N > 1 code path on ONE rank (a 1-rank RCCL process group, reducer attached and detached "
                         "legs, the back-to-back bucket all-reduce) -- a rehearsal of what the driver's scaling run executes, on a "
                         "one-GPU box; the JSON line carries \"rehearse_dp\": true")
    ap.add_argument("--dry", action="store_true",
                    help="plumbing rehearsal without kernels: launcher, rendezvous, barrier/max-over-ranks timing and the "
                         "bucketed GradReducer on a small CPU stand-in model; the JSON line says \"dry\": true and is NOT a "
                         "measurement")
    return ap.parse_args()


def host_cores() -> int:
    """CPU share of this process: cgroup quota if set, else affinity; a 1-GPU box gives 16 cores."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        pass
    return int(os.environ.get("GSSEG_CPU_THREADS", min(n, 16)))


def cpu_baseline(args):
    """The oracle (CPU port of the reference path) timed on this box's host cores: fp32, fwd+loss+bwd."""
    from oracle import oracle
    cores = host_cores()
    torch.set_num_threads(cores)
    sd = oracle.unet_state_dict(1, args.classes, seed=0)
    x, mask = oracle.synthetic_batch(args.cpu_batch, args.size, seed=1234)
    oracle.unet_step(sd, x, mask, train=True)                       # warm-up (oneDNN primitive creation)
    t0 = time.perf_counter()
    for _ in range(args.cpu_steps):
        oracle.unet_step(sd, x, mask, train=True)
    dt = (time.perf_counter() - t0) / args.cpu_steps
    ips = args.cpu_batch / dt
    return {"value": round(ips, 4), "unit": "images/sec", "cores": cores, "kind": "port",
            "sample": f"oracle.unet_step fp32, UNet(1,{args.classes}) {args.size}x{args.size} batch {args.cpu_batch}, "
                      f"{args.cpu_steps} timed steps after 1 warm-up, torch {torch.__version__} CPU",
            "gflops": round(ips * GF_PER_IMG_FWDBWD.get(args.classes, 288.5) * (args.size / 256.0) ** 2, 1)}


def dump_sample(t, n, seed):
    """t as float32 numpy; with more than n elements, the same n of its flattened values in every run (sorted indices drawn from
    a fixed seed), so that two builds compare element for element."""
    import numpy as np
    t = t.detach()
    if t.numel() > n:
        idx = np.sort(np.random.default_rng(seed).choice(t.numel(), n, replace=False))
        t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
    return t.float().cpu().numpy()


def dump_outputs(out_dir, logits, loss, net):
    """What a caller of the timed step receives, as .npy files: the logits and every parameter's gradient, flattened (float32,
    sampled above DUMP_MAX_LOGITS / DUMP_MAX_ELEMS elements), and the loss (float64)."""
    import numpy as np
    arrays = {"logits": dump_sample(logits, DUMP_MAX_LOGITS, 0),
              "loss": np.asarray(loss.detach().double().item(), dtype=np.float64)}
    for i, (name, p) in enumerate(net.named_parameters()):
        arrays[f"grad.{name}"] = dump_sample(p.grad.reshape(-1), DUMP_MAX_ELEMS, 1 + i)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_MAX_BYTES}-byte budget")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(args) -> int:
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes of this script (one per GPU) with the
    torch.distributed environment, relay rank 0's JSON line, fail if any rank fails.  This parent never initialises a
    GPU (no HIP call, no torch.cuda.is_available()), and nothing is exec'ed: children are ordinary subprocesses."""
    port = free_port()
    import tempfile
    procs = []
    with tempfile.TemporaryFile("w+") as out0:
        for r in range(args.gpus):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus),
                       LOCAL_WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                       HSA_ENABLE_IPC_MODE_LEGACY="0")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=out0 if r == 0 else subprocess.DEVNULL))
        # a rank that dies leaves the others waiting in the rendezvous / a collective: stop exactly those PIDs
        while any(p.poll() is None for p in procs):
            if any(p.poll() not in (None, 0) for p in procs):
                for p in procs:
                    if p.poll() is None:
                        p.terminate()
                break
            time.sleep(0.2)
        codes = []
        for p in procs:
            try:
                codes.append(p.wait(timeout=30))
            except subprocess.TimeoutExpired:
                p.kill()
                codes.append(p.wait())
        out0.seek(0)
        text = out0.read()
    line = next((ln for ln in reversed(text.splitlines()) if ln.startswith("{")), None)
    if any(codes) or line is None:
        sys.stderr.write(f"bench.py: rank exit codes {codes}; rank-0 output:\n{text}\n")
        return 1
    print(line, flush=True)
    return 0


def dry_main(args, world, rank):
    """--dry: everything of the multi-rank bench except the kernels (CPU, gloo): rendezvous, replica broadcast, the bucketed
    GradReducer driven in backward order by a stand-in model, barrier + max-over-ranks timing, one JSON line on rank 0."""
    import torch.distributed as dist
    from semantic_segmentation_amd.parallel import GradReducer, broadcast_module_state
    if world > 1:
        dist.init_process_group(args.backend, rank=rank, world_size=world)
    torch.manual_seed(1234 + rank)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 8, 3, padding=1), torch.nn.BatchNorm2d(8), torch.nn.ReLU(),
                              torch.nn.Conv2d(8, 2, 1))
    broadcast_module_state(net)
    reducer = GradReducer(net.named_parameters(), bucket_bytes=256) if world > 1 else None
    x = torch.randn(args.batch, 1, 16, 16)
    names = [n for n, _ in net.named_parameters()][::-1]
    params = dict(net.named_parameters())

    def step():
        net.zero_grad(set_to_none=True)
        loss = net(x).square().mean()
        loss.backward()
        if reducer is not None:
            reducer.begin()
            for n in names:
                reducer.ready(n, params[n].grad)
            reducer.finish()
        return loss

    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        g = [torch.zeros_like(reducer.flat) for _ in range(world)]
        dist.all_gather(g, reducer.flat)
        assert all(torch.equal(g[0], q) for q in g), "averaged gradients differ across ranks"
    if rank == 0:
        print(json.dumps({"metric": "images/sec (fwd+bwd) U-Net 256x256 bs=32 per GPU", "dry": True,
                          "value": round(world * args.batch * args.steps / elapsed, 2), "unit": "images/sec",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / args.steps * 1e3, 3), "scaling": "weak",
                          "ranks": dist.get_world_size() if world > 1 else 1, "backend": args.backend,
                          "data": "stand-in model on CPU: plumbing rehearsal, not a measurement"}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.dry:
        return dry_main(args, world, rank)
    if args.backend != "nccl":
        raise SystemExit("--backend gloo is only for --dry (the product path has no CPU fallback)")
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no GPU visible (there is no CPU fallback for the product path)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    multi = world > 1 or args.rehearse_dp          # the data-parallel code path (rehearsal: one rank, the same calls)
    if multi:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # RCCL's kernels on a high-priority stream: the persistent compute grids hold every CU until a kernel boundary; at the
        # boundary a bucket's all-reduce must win the CUs against the next compute launch that is already queued
        pg_opts = None
        if os.environ.get("GSSEG_RCCL_HIGH_PRIORITY", "1") != "0" and hasattr(dist, "ProcessGroupNCCL"):
            pg_opts = dist.ProcessGroupNCCL.Options()
            pg_opts.is_high_priority_stream = True
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(free_port()))
            dist.init_process_group("nccl", device_id=dev, rank=0, world_size=1, pg_options=pg_opts)
        else:
            dist.init_process_group("nccl", device_id=dev, pg_options=pg_opts)

    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd.harness import synthetic_batch
    from semantic_segmentation_amd.losses import seg_loss
    from semantic_segmentation_amd.parallel import GradReducer, broadcast_module_state
    from semantic_segmentation_amd.unet import UNet

    x, mask = synthetic_batch(args.batch, args.size, seed=1234 + rank)
    if args.host_input:
        x_host, mask_host = x.pin_memory(), mask.pin_memory()
    x, mask = x.to(dev), mask.to(dev)

    def timed_leg(precise, with_reducer):
        """W warm-up steps, then exactly K timed steps of forward + loss + backward in the given numerics mode, bracketed by a
        barrier + synchronize on both sides; returns (elapsed seconds, per-step ms, per-kernel summary (None without --full),
        last logits, last loss, reducer, net)."""
        torch.manual_seed(1234)
        net = UNet(1, args.classes, compute_dtype=args.dtype, precise={"full": True, "mixed": "mixed", "fast": False}[precise]).to(dev)
        net.train()
        broadcast_module_state(net)
        reducer = None
        if multi and with_reducer:
            reducer = GradReducer(net.named_parameters()).attach(net.engine)

        def step():
            for p in net.parameters():
                p.grad = None
            net.engine.invalidate_packs()      # weights change every step in training: re-pack inside the timed region
            xs, ms_ = x, mask
            if args.host_input:
                xs, ms_ = x_host.to(dev, non_blocking=True), mask_host.to(dev, non_blocking=True)
            logits = net(xs)
            loss = seg_loss(logits, ms_, global_dice=True if (args.global_dice and multi) else None)
            loss.backward()
            return logits, loss

        # one untimed step first (with --full it counts the bracketed launches, so every event exists beforehand)
        probe = ops.KernelTimer() if args.full else None
        ops.TIMER = probe
        step()
        ops.TIMER = None
        timer = None
        if args.full:
            timer = ops.KernelTimer(pool=2 * len(probe.records) * (args.steps + args.warmup) + 64)
        # the W warm-up steps come AFTER the event pool is built (thousands of hipEventCreate calls: milliseconds of idle GPU) and
        # run with the timer attached, so the timed region starts from the steady state it measures (the first timed step used to
        # read 14.0 ms against 12.3 for the other nineteen: clocks ramping back up)
        ops.TIMER = timer
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        if timer is not None:
            timer.reset()
        if multi:
            dist.barrier()
        torch.cuda.synchronize()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]    # on the launch (= current) stream
        t0 = time.perf_counter()
        marks[0].record()
        for i in range(args.steps):
            logits, loss = step()
            marks[i + 1].record()
        if multi:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        ops.TIMER = None
        step_ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
        return elapsed, step_ms, None if timer is None else timer.summary(), logits, loss, reducer, net

    elapsed, step_ms, ksum, logits, loss, reducer, net = timed_leg(args.precise, True)
    if os.environ.get("GSSEG_BENCH_VERBOSE"):
        sys.stderr.write("step ms: " + " ".join(f"{v:.2f}" for v in step_ms) + "\n")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, logits, loss, net)
    del logits, net
    # the gradient exchange on its own (not overlapped with anything), for the scaling discussion: all buckets back to back
    allreduce_ms = None
    if args.full and reducer is not None:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 5
        dist.barrier()
        e0.record()
        for _ in range(reps):
            for b in reducer.buckets:
                lo, hi = b["range"]
                dist.all_reduce(reducer.flat[lo:hi], op=reducer.op)
        e1.record()
        torch.cuda.synchronize()
        allreduce_ms = e0.elapsed_time(e1) / reps
    if multi:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # N > 1: the same K steps once more WITHOUT the gradient exchange (reducer detached: every rank steps on its own shard), same
    # barrier + max-over-ranks timing: ms_per_step - ms_per_step_no_exchange = what the exchange costs after overlap ("exposed"),
    # next to `allreduce_ms_per_step_unoverlapped` (all buckets back to back with nothing to hide behind)
    no_exchange_ms = None
    if args.full and multi:
        ne_elapsed = timed_leg(args.precise, False)[0]
        t = torch.tensor([ne_elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        no_exchange_ms = float(t.item()) / args.steps * 1e3
    # second leg, N = 1 only (like the CPU baseline): the fast 16-bit mode, whose logits are OUTSIDE the north star's tolerance
    fast = None
    if args.full and world == 1 and not multi and args.fast_leg != "none" and args.precise == "mixed":
        p_elapsed, p_step_ms, p_ksum, _, p_loss, _, _ = timed_leg("fast", False)
        fast = {"mode": PARITY_MODES["fast"][0], "value": round(args.batch * args.steps / p_elapsed, 2),
                "unit": "images/sec", "ms_per_step": round(p_elapsed / args.steps * 1e3, 3),
                "ms_per_step_median": round(statistics.median(p_step_ms), 3),
                "max_abs_dlogit_bound": PARITY_MODES["fast"][1], "bound_asserted_in": PARITY_MODES["fast"][2],
                "meets_north_star_tolerance": False,
                "loss": float(p_loss.item()), "steps": args.steps, "warmup": args.warmup,
                "conv3x3_family": family_summary(p_ksum, args.steps)}
    if rank != 0:
        if multi:
            dist.destroy_process_group()
        return

    ms = elapsed / args.steps * 1e3
    value = world * args.batch * args.steps / elapsed
    gf = GF_PER_IMG_FWDBWD.get(args.classes, 288.5) * (args.size / 256.0) ** 2
    kern = kernel_table(ksum, args.steps) if args.full else None
    # the dominant kernel FAMILY (sub-entries "x.y" are parts of family "x" and are not candidates)
    dom = max((k for k in kern if "." not in k), key=lambda k: kern[k]["ms_per_step"]) if kern else None
    roof = None
    if dom:
        traffic, traffic_src, traffic_sha = pmc_traffic(dom)
        cur_sha = source_sha16()
        roof = {"kernel": dom, "bound": "mfma", "achieved": kern[dom]["tflops"], "peak": MFMA_PEAK_TFLOPS,
                "unit": "TFLOP/s", "frac": round(kern[dom]["tflops"] / MFMA_PEAK_TFLOPS, 4), "traffic": traffic,
                "traffic_source": traffic_src, "traffic_source_sha16": traffic_sha, "kernel_source_sha16": cur_sha,
                "traffic_current": None if traffic_sha is None else traffic_sha == cur_sha,
                "algorithmic_bytes_per_launch": kern[dom]["algorithmic_bytes_per_launch"],
                "measured_sustained_mfma_tflops": MFMA_SUSTAINED_TFLOPS,
                "frac_of_sustained": round(kern[dom]["tflops"] / MFMA_SUSTAINED_TFLOPS, 4),
                "avg_launch_us": kern[dom]["avg_launch_us"],
                "flop_per_launch": round(kern[dom]["tflop_per_step"] * 1e12 / kern[dom]["launches_per_step"], 0)}
    out = {
        "metric": "images/sec (fwd+bwd) U-Net 256x256 bs=32 per GPU", "value": round(value, 2), "unit": "images/sec",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"unet.UNet(1,{args.classes}) {args.size}x{args.size} fwd+bwd, CE+Dice loss, "
                               f"batch {args.batch}/GPU (BASELINE configs[1])",
                   "global_batch": world * args.batch, "parallelism": f"dp{world}", "loss": float(loss.item()),
                   "dice": "global-batch (3-scalar all-reduce)" if (args.global_dice and world > 1) else "per-rank"},
        "mode": PARITY_MODES[args.precise][0], "max_abs_dlogit_bound": PARITY_MODES[args.precise][1],
        "bound_asserted_in": PARITY_MODES[args.precise][2], "meets_north_star_tolerance": PARITY_MODES[args.precise][1] <= 1e-3,
        "fast_mode": fast,
        "input": "pinned host memory, copied every step (PCIe-inclusive)" if args.host_input else "resident in HBM",
        "ms_per_step_median": round(statistics.median(step_ms), 3),
        "ms_per_step_min_max": [round(min(step_ms), 3), round(max(step_ms), 3)],
        "value_at_median_step": round(world * args.batch / statistics.median(step_ms) * 1e3, 2),
        "rccl_ranks": dist.get_world_size() if multi else 1, "rehearse_dp": bool(args.rehearse_dp and world == 1),
        "allreduce_ms_per_step_unoverlapped": None if allreduce_ms is None else round(allreduce_ms, 3),
        "grad_buckets": None if reducer is None else len(reducer.buckets),
        "ms_per_step_no_exchange": None if no_exchange_ms is None else round(no_exchange_ms, 3),
        "exposed_exchange_ms_per_step": None if no_exchange_ms is None else round(ms - no_exchange_ms, 3),
        "whole_step_tflops": round(value * gf / 1e3, 1),
        "whole_step_frac_of_mfma_peak": round(value * gf / 1e3 / (MFMA_PEAK_TFLOPS * world), 4),
        "roofline": roof, "kernels": kern, "full": args.full,
    }
    if args.full and world == 1 and not multi and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args)
    else:
        out["cpu_baseline"] = None
    print(json.dumps(out), flush=True)
    if multi:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
