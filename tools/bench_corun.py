#!/usr/bin/env python3
"""Co-run gate for the side-stream weight gradients: does the BatchNorm backward of a stage hide beside
the 3x3 weight gradient that is still running on the second stream?

Two co-runners per BatchNorm shape, at batch 32 (128^2 x 128, 64^2 x 256, 32^2 x 512, 16^2 x 1024), with HIP events:
  C->C    the C -> C weight gradient of the stage before it in the same block (same level);
  2C->C   the 2C -> C weight gradient of the Up block one level up (twice the side, half the channels out): the long window
          in which the first stage of the next Up block runs its BatchNorm backward (levels 2-4).
  t_w    the weight gradient alone (slabs + ordered reduction)
  t_bn   BatchNorm backward reduce + coeffs + apply alone
  t_both both started together on two streams of this process
once with the normal BatchNorm kernels and once with the co-resident forms (ops.bn_bwd_set_form).  Hidden fraction =
(t_w + t_bn - t_both) / min(t_w, t_bn): 1 = the shorter part costs nothing, 0 = the two serialise.

Every timed region sits behind a 1 GiB fill on the main stream: the launches are all queued while the fill runs (no host launch
latency inside the region, both streams start on the same event) and the tensors are out of the caches, as in a real step.
Kill rule: the co-resident forms must hide at least a quarter of sum(min(t_w, t_bn)) over the four C->C shapes.

To set two builds side by side on one box, run the tool once per build: GSSEG_LIB=<path to that build's libgsseg_hip.so>
selects the library, --label names the run in every line it prints, and --repeat N runs the whole table N times in one
process (the spread between repeats of one build is the yardstick for a difference between two).  Run on the GPU box."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_segmentation_amd import ops  # noqa: E402
from semantic_segmentation_amd._lib import ACT_RELU  # noqa: E402

SHAPES = ((128, 128), (64, 256), (32, 512), (16, 1024))
ITERS = 15


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("batch", nargs="?", type=int, default=32)
    ap.add_argument("--corunner", choices=("cc", "2cc", "both"), default="both", help="which weight gradient runs beside")
    ap.add_argument("--forms", default="normal,slim", help="comma-separated: normal, slim")
    ap.add_argument("--label", default="", help="name of this build in the printed lines")
    ap.add_argument("--repeat", type=int, default=1, help="run the whole table this many times")
    args = ap.parse_args()
    forms = [(dict(normal=ops.BN_BWD_NORMAL, slim=ops.BN_BWD_SLIM)[f], f) for f in args.forms.split(",")]
    tag = f"[{args.label}] " if args.label else ""
    dev = torch.device("cuda:0")
    N = args.batch
    dt = torch.float16
    main_s = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(device=dev)
    fill = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    print(f"{tag}batch {N}, f16, median of {ITERS}; times in us; wgrad family 0 = register-staged, 2 = 128-cout LDS-DMA")
    cases = []                                               # (BatchNorm side, C, co-runner name, its side, cin, cout)
    for H, C in SHAPES:
        if args.corunner in ("cc", "both"):
            cases.append((H, C, "C->C", H, C, C))
        if args.corunner in ("2cc", "both") and C >= 256:
            cases.append((H, C, "2C->C", 2 * H, C, C // 2))
    for rep in range(args.repeat):
        print(f"{tag}{'shape':>14s} {'beside':>6s} {'fam':>3s} {'form':>6s} {'t_w':>7s} {'t_bn':>7s} {'t_both':>7s} {'hidden':>7s}")
        tot = {}
        for H, C, kind, Hw, cin, cout in cases:
            x = torch.randn(N, Hw, Hw, cin, device=dev).to(dt)      # the conv's input
            dyw = torch.randn(N, Hw, Hw, cout, device=dev).to(dt)   # d(conv output) of the weight gradient's stage
            y = torch.randn(N, H, H, C, device=dev).to(dt)          # the next stage's conv output (BatchNorm input)
            dz = torch.randn(N, H, H, C, device=dev).to(dt)
            dy = torch.empty_like(y)
            coef = torch.rand(4, C, device=dev) + 0.5
            c12 = torch.empty(2, C, device=dev)
            dgb = torch.empty(2, C, device=dev)
            part = torch.empty(ops.bn_partials_numel(ops.bn_bwd_tiles(N, H, H), C), device=dev)
            ntiles = ops.bn_bwd_tiles_used(N, H, H, False)
            ws = torch.empty(ops.conv3x3_wgrad_ws_floats(N, Hw, Hw, cin, cout), device=dev)
            dw = torch.empty(cout, cin, 3, 3, device=dev)
            fam = ops.conv3x3_wgrad_family(Hw, cout)

            def wgrad():
                ops.conv3x3_wgrad_det(x, dyw, ws, dw, N, Hw, Hw, cin, cout, 1.0)

            def bn():
                ops.bn_act_bwd_reduce(y, dz, C, 0, None, coef[0], coef[1], coef[2], coef[3], ACT_RELU, part)
                ops.bn_bwd_coeffs(part, ntiles, C, N * H * H, 1.0, dgb[0], dgb[1], c12[0], c12[1])
                ops.bn_act_bwd_apply(y, dz, C, 0, None, coef[0], coef[1], coef[2], coef[3], c12[0], c12[1], ACT_RELU, True, dy)

            def timed(do_w, do_bn):
                ts = []
                for _ in range(ITERS + 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    done = torch.cuda.Event()
                    fill.zero_()
                    e0.record(main_s)
                    if do_w:
                        with torch.cuda.stream(side):
                            side.wait_event(e0)
                            wgrad()
                            done.record(side)
                    if do_bn:
                        bn()
                    if do_w:
                        main_s.wait_event(done)
                    e1.record(main_s)
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
                return statistics.median(ts[2:])

            for form, name in forms:
                with ops.bn_bwd_form(form):
                    t_w, t_bn, t_both = timed(True, False), timed(False, True), timed(True, True)
                short = min(t_w, t_bn)
                hid = t_w + t_bn - t_both
                a = tot.setdefault((kind, name), [0.0, 0.0, 0.0])
                a[0] += hid; a[1] += short; a[2] += t_bn
                print(f"{tag}{H:4d}^2 x {C:4d} {kind:>6s} {fam:3d} {name:>6s} {t_w:7.1f} {t_bn:7.1f} {t_both:7.1f} {hid / short:7.2f}")
        for (kind, name), (hid, short, tbn) in tot.items():
            print(f"{tag}run {rep}: sum over the {kind:>5s} shapes, {name:>6s}: hidden {hid:7.1f} us of min(t_w, t_bn) {short:7.1f} us"
                  f" = {hid / short:.2f}   (t_bn alone {tbn:7.1f} us)")
        if ("C->C", "slim") in tot:
            hid, short, _ = tot[("C->C", "slim")]
            print(f"{tag}run {rep}: gate (slim hides >= 0.25 of the shorter parts, C->C): " + ("PASS" if hid >= 0.25 * short else "FAIL"))


if __name__ == "__main__":
    main()
