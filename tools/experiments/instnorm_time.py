"""Pix2Pix under `--norm instance` beside `--norm batch`, from one run: generator (unet_256) and PatchGAN forward + backward at
256 x 256, batch 2 and 32, fp16, and the three InstanceNorm entry points on their own at the generator's level shapes.

Networks: device events around one forward + backward (the engines called directly on a fixed dense gradient, as the replay tests
call them), WARM warm-up steps per variant, then ROUNDS rounds with norm='batch' and norm='instance' alternating inside the one
process; mean, min and spread (max - min over the rounds, relative to the mean) per variant.
Kernels: device events around CALLS back-to-back launches (a single launch of the deep levels is shorter than the launch overhead),
the same warm-up and alternation; bytes = the algorithmic traffic (y read once by gs_in_stats; y read and the outputs written by
gs_in_act_apply; y, dz_a (dz_b) read twice and dy written by gs_in_act_bwd), and those bytes over the mean time.  Tensors below
256 MiB stay in the Infinity Cache between calls: those rates are cache-resident rates, not HBM rates.
Usage: python tools/experiments/instnorm_time.py [output file]      (default profiles/instnorm_time.txt)"""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from semantic_segmentation_amd import ops
from semantic_segmentation_amd._lib import ACT_LEAKY02, ACT_RELU
from semantic_segmentation_amd.models_pix2pix import networks, pix2pix_backward as pb

WARM, ROUNDS, CALLS = 3, 10, 50
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls            # microseconds per call


def alternate(variants, calls):
    for _, fn in variants:
        for _ in range(WARM):
            timed(fn, calls)
    times = {n: [] for n, _ in variants}
    for _ in range(ROUNDS):
        for n, fn in variants:
            times[n].append(timed(fn, calls))
    return {n: (sum(v) / len(v), min(v), (max(v) - min(v)) / (sum(v) / len(v)) * 100) for n, v in times.items()}


torch.manual_seed(0)
dev = torch.device("cuda")
for N in (2, 32):
    x = torch.randn(N, 1, 256, 256, device=dev)
    pair = torch.randn(N, 2, 256, 256, device=dev)
    dout = torch.randn(N, 1, 256, 256, device=dev) / (N * 65536)
    arch = (0.5 * torch.randn(8, 3)).to(dev)
    gens, discs = {}, {}
    for norm in ("batch", "instance"):
        G = networks.define_G(1, 1, 64, "unet_256", norm, True).cuda().train()
        D = networks.define_D(2, 64, "basic", 3, norm).cuda().train()
        G.engine.trust_versions = D.engine.trust_versions = True
        dl = torch.randn(D(pair).shape, device=dev) / (N * 900)

        def g_step(G=G):
            with torch.no_grad():
                _, ctx = G.engine.forward(x, arch, True, True, None)
                pb.generator_backward(G.engine, ctx, arch, dout, False)

        def d_step(D=D, dl=dl):
            with torch.no_grad():
                _, ctx = D.engine.forward(pair, True, True)
                D.engine.backward(ctx, dl, True)
        gens[norm], discs[norm] = g_step, d_step
    for what, steps in (("generator unet_256", gens), ("PatchGAN basic", discs)):
        res = alternate([(n, f) for n, f in steps.items()], 1 if N == 32 else 4)
        for n, (mean, mn, spread) in res.items():
            say(f"batch {N:2d}  {what:20s} norm={n:9s} fwd+bwd mean {mean / 1e3:8.3f} ms  min {mn / 1e3:8.3f} ms  spread {spread:5.1f} %")
        say(f"batch {N:2d}  {what:20s} instance / batch = {res['instance'][0] / res['batch'][0]:.3f}")

    # the three entry points at the generator's normed shapes (side, channels): the up outputs of blocks 1..7, of which all but
    # the first are also the down levels 2..7
    for side, C in [(256 >> d, min(64 << (d - 1), 512)) for d in range(1, 8)]:
        y = torch.randn(N, side, side, C, device=dev).half()
        dza = torch.randn(N, side, side, 2 * C, device=dev).half()
        dzb = torch.randn(N, side, side, C, device=dev).half()
        mi = torch.empty(2, N, C, device=dev)
        gm = torch.empty(2, N, C, device=dev)
        ws = ops.in_workspace(N, side, side, C, dev)
        z, z2, dy = torch.empty_like(y), torch.empty_like(dza), torch.empty_like(y)
        ops.in_stats(y, 1e-5, mi[0], mi[1], ws)
        nb = y.numel() * 2
        variants = [("gs_in_stats", lambda: ops.in_stats(y, 1e-5, mi[0], mi[1], ws), nb),
                    ("gs_in_act_apply (2 outputs)", lambda: ops.in_act_apply(y, mi[0], mi[1], ACT_LEAKY02, z, C, 0, z2=z2, act2=ACT_RELU,
                                                                            z2_stride=2 * C, z2_coff=0), 3 * nb),
                    ("gs_in_act_bwd (2 consumers)", lambda: ops.in_act_bwd(y, mi[0], mi[1], dza, 2 * C, 0, ACT_RELU, dy, gm, ws, dz_b=dzb,
                                                                           act_b=ACT_LEAKY02), 7 * nb)]
        res = alternate([(n, f) for n, f, _ in variants], CALLS)
        for n, _, nbytes in variants:
            mean, mn, spread = res[n]
            say(f"batch {N:2d}  {side:3d}x{side:<3d}x{C:3d}  {n:28s} mean {mean:8.2f} us  min {mn:8.2f} us  spread {spread:5.1f} %  "
                f"bytes {nbytes / 1e6:8.2f} MB  {nbytes / mean / 1e6:6.3f} TB/s")
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "instnorm_time.txt")
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
