"""The ResNet generator (`--netG resnet_9blocks`, ngf 64, 1 -> 1 channels and the canonical RGB 3 -> 3) beside unet_256, from one
run: forward + backward at 256 x 256, batch 2 and 32, fp16, under norm='batch' and norm='instance', and the new kernels on their own
at the shapes one step launches them at: the memory-bound passes (csrc/reflect.hip) and the five launches of the two 7x7 ends
(csrc/ends.hip; the stem's data gradient runs only when the input image needs a gradient, and is left out).

Networks: device events around one forward + backward (the engines called directly on a fixed dense gradient, as the replay tests
call them), WARM warm-up steps per variant, then ROUNDS rounds with the four variants alternating inside the one process; mean, min
and spread (max - min over the rounds, relative to the mean) per variant.  unet_256's figures of the same run stand beside them
(profiles/instnorm_time.txt holds the earlier record of those).
Kernels: device events around CALLS back-to-back launches, the same warm-up and alternation; bytes = the algorithmic traffic (every
operand read once, the output written once, padded sizes where a tensor is padded), and those bytes over the mean time.  Tensors
below 256 MiB stay in the Infinity Cache between calls: those rates are cache-resident rates, not HBM rates.
Share of the step: sum over the step's launch list of (launches x mean kernel time) over the step's mean time -- the kernels are
timed back to back on their own, so the share leaves out what the step's launch gaps add.
Usage: python tools/experiments/resnet_time.py [output file]      (default profiles/resnet_time.txt)"""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from semantic_segmentation_amd import ops
from semantic_segmentation_amd._lib import ACT_NONE, ACT_RELU
from semantic_segmentation_amd.models_pix2pix import networks, pix2pix_backward as pb, resnet_engine as re_

WARM, ROUNDS, CALLS = 3, 10, 20
NB = 9
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
    dout = torch.randn(N, 1, 256, 256, device=dev) / (N * 65536)
    x3 = torch.randn(N, 3, 256, 256, device=dev)
    dout3 = torch.randn(N, 3, 256, 256, device=dev) / (N * 3 * 65536)
    arch = (0.5 * torch.randn(8, 3)).to(dev)
    steps = {}
    for norm in ("batch", "instance"):
        R = networks.define_G(1, 1, 64, "resnet_9blocks", norm, True).cuda().train()
        R3 = networks.define_G(3, 3, 64, "resnet_9blocks", norm, True).cuda().train()
        R3.engine.trust_versions = True
        U = networks.define_G(1, 1, 64, "unet_256", norm, True).cuda().train()
        R.engine.trust_versions = U.engine.trust_versions = True

        def r_step(R=R):
            with torch.no_grad():
                _, ctx = R.engine.forward(x, True, True, None)
                re_.resnet_generator_backward(R.engine, ctx, dout, False)

        def r3_step(R=R3):
            with torch.no_grad():
                _, ctx = R.engine.forward(x3, True, True, None)
                re_.resnet_generator_backward(R.engine, ctx, dout3, False)

        def u_step(U=U):
            with torch.no_grad():
                _, ctx = U.engine.forward(x, arch, True, True, None)
                pb.generator_backward(U.engine, ctx, arch, dout, False)
        steps["resnet_9blocks " + norm], steps["unet_256       " + norm] = r_step, u_step
        steps["resnet_9b 3->3 " + norm] = r3_step
    res = alternate(list(steps.items()), 1 if N == 32 else 4)
    for n, (mean, mn, spread) in res.items():
        say(f"batch {N:2d}  generator {n:24s} fwd+bwd mean {mean / 1e3:8.3f} ms  min {mn / 1e3:8.3f} ms  spread {spread:5.1f} %")
    for norm in ("batch", "instance"):
        say(f"batch {N:2d}  resnet_9blocks / unet_256 under norm={norm}: {res['resnet_9blocks ' + norm][0] / res['unet_256       ' + norm][0]:.3f}")

    # ---- the new passes at the shapes of one step (side, channels, pad), with their launch counts per forward + backward
    def t16(*shape):
        return torch.randn(shape, device=dev).half()

    def apply_case(side, C, pad, res, launches, label):
        y = t16(N, side, side, C)
        z = torch.empty(N, side + 2 * pad, side + 2 * pad, C, device=dev, dtype=torch.float16)
        r = t16(N, side + 2, side + 2, C) if res else None
        keep = (torch.rand(N, side, side, C, device=dev) > 0.5).to(torch.uint8) if label.endswith("keep") else None
        sc, sh = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        nbytes = 2 * (y.numel() + z.numel() + (y.numel() if res else 0)) + (y.numel() if keep is not None else 0)
        act = ACT_NONE if res else ACT_RELU
        return (label, lambda: ops.reflect_norm_apply(y, sc, sh, ops.NORM_BATCH, act, z, pad, r, 1, keep, 2.0), nbytes, launches)

    def fold_case(side, C, pad, add, launches, label):
        d = t16(N, side + 2 * pad, side + 2 * pad, C)
        a = t16(N, side, side, C) if add else None
        out = torch.empty(N, side, side, C, device=dev, dtype=torch.float16)
        nbytes = 2 * (d.numel() + out.numel() + (out.numel() if add else 0))
        return (label, lambda: ops.reflect_fold_add(d, out, pad, a), nbytes, launches)

    img, imgp = torch.randn(N, 1, 256, 256, device=dev), torch.empty(N, 1, 262, 262, device=dev)
    t = torch.empty_like(img)
    cases = [
        apply_case(256, 64, 0, False, 1, "apply 256x256x 64 pad 0 (stem)"),
        apply_case(128, 128, 0, False, 2, "apply 128x128x128 pad 0 (down 1, up 1)"),
        apply_case(64, 256, 1, False, 1 + NB, "apply  64x 64x256 pad 1 keep"),
        apply_case(64, 256, 1, True, NB, "apply  64x 64x256 pad 1 + residual"),
        apply_case(256, 64, 3, False, 1, "apply 256x256x 64 pad 3 (head input)"),
        fold_case(64, 256, 1, False, NB, "fold   64x 64x256 pad 1"),
        fold_case(64, 256, 1, True, NB, "fold   64x 64x256 pad 1 + stream"),
        fold_case(256, 64, 3, False, 1, "fold  256x256x 64 pad 3 (head input)"),
        ("image pad 3 + tanh forward + tanh backward", lambda: (ops.reflect_pad_image(img, imgp, 3), ops.tanh_fwd(img, t),
                                                             ops.tanh_bwd(t, img, 1024.0, t)), 4 * (2 * img.numel() + imgp.numel() + 4 * img.numel()), 1),
    ]

    def ends_cases(c):
        xp, ws_, T = torch.randn(N, c, 262, 262, device=dev), 0.05 * torch.randn(64, c, 7, 7, device=dev), t16(N, 262, 262, 64)
        wh, bh, d = 0.05 * torch.randn(c, 64, 7, 7, device=dev), torch.zeros(c, device=dev), torch.randn(N, c, 256, 256, device=dev)
        y, dT, out = t16(N, 256, 256, 64), torch.empty_like(T), torch.empty_like(d)
        part = torch.empty(ops.bn_partials_numel(ops.conv_ends_mtiles(N, 256, 256), 64), device=dev)
        dws, dwh, dbh = torch.empty_like(ws_), torch.empty_like(wh), torch.empty_like(bh)
        b16, bimg, bd = 2 * y.numel(), 4 * xp.numel(), 4 * d.numel()
        return [(f"7x7 stem forward {c} -> 64 (+ BN partials)", lambda: ops.conv_ends_to_c16(xp, ws_, y, part), bimg + b16, 1),
                (f"7x7 stem weight gradient {c} -> 64", lambda: ops.conv_ends_wgrad(y, xp, dws, None), bimg + b16, 1),
                (f"7x7 head forward 64 -> {c}", lambda: ops.conv_ends_to_img(T, wh, bh, out), 2 * T.numel() + bd, 1),
                (f"7x7 head data gradient 64 -> {c}", lambda: ops.conv_ends_to_c16(d, wh, dT, None, pad=6, flip=True, w_img_major=True),
                 2 * T.numel() + bd, 1),
                (f"7x7 head weight + bias gradient 64 -> {c}",
                 lambda: ops.conv_ends_wgrad(T, d, dwh, dbh, pad=6, flip=True, w_img_major=True), 2 * T.numel() + bd, 1)]
    ends = {c: ends_cases(c) for c in (1, 3)}
    cases_all = cases + ends[1] + ends[3]
    kres = alternate([(c[0], c[1]) for c in cases_all], CALLS)
    total = 0.0
    etotal = {1: 0.0, 3: 0.0}
    for c in (1, 3):
        etotal[c] = sum(kres[label][0] for label, _, _, _ in ends[c])
    for label, _, nbytes, launches in cases_all:
        mean, mn, spread = kres[label]
        if not label.startswith("7x7"):
            total += launches * mean
        say(f"batch {N:2d}  {label:44s} x{launches:2d}  mean {mean:8.2f} us  min {mn:8.2f} us  spread {spread:5.1f} %  "
            f"bytes {nbytes / 1e6:8.2f} MB  {nbytes / mean / 1e6:6.3f} TB/s")
    for norm in ("batch", "instance"):
        step = res["resnet_9blocks " + norm][0]
        say(f"batch {N:2d}  new passes of one step, timed on their own: {total / 1e3:7.3f} ms = {100 * total / step:4.1f} % of the "
            f"norm={norm} step ({step / 1e3:.3f} ms)")
        for c, key in ((1, "resnet_9blocks "), (3, "resnet_9b 3->3 ")):
            step = res[key + norm][0]
            say(f"batch {N:2d}  the five 7x7 end launches, {c} channel(s): {etotal[c] / 1e3:7.3f} ms = {100 * etotal[c] / step:4.1f} % of the "
                f"{c} -> {c} norm={norm} step ({step / 1e3:.3f} ms)")
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resnet_time.txt")
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
