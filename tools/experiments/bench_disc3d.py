"""The 3-D Pix2Pix discriminators (models_pix2pix/discriminator_engine.py, csrc/ends_img.hip, csrc/ends3d.hip) timed at the reference's
--crop_size, 64^3: forward + backward with dx of NLayerDiscriminator(2, 64, 3) and PixelDiscriminator(2, 64) on volumes, batch 1
and 4, under BatchNorm3d and InstanceNorm3d, the two norms interleaved in one process; then every launch of each plan on its own
(event pairs around each call, in the plan's order): time, algorithmic TFLOP/s for the convs, GB/s for the passes.  The algorithmic
work is computed here from the shapes: a conv's 2 * outputs * Cin * taps (pad taps included), and the bytes each launch has to
move once (inputs read, outputs written, fp32 weights / 16-bit packs).

    python tools/experiments/bench_disc3d.py [--out profiles/disc3d_time.txt]
Device events, warm-up, medians; figures of one process on one GPU.  First numbers for this path: no threshold is set on them."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from semantic_segmentation_amd import ops                                            # noqa: E402

dev = "cuda"
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps=3, inner=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner * 1e3)
    return out                                                                       # us per call


def interleaved(forms, rounds=4, **kw):
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            t[k] += timed(f, **kw)
    return t


def row(name, v):
    med = statistics.median(v)
    say(f"  {name:<34} median {med:9.1f} us   min {min(v):9.1f}   max {max(v):9.1f}   spread {(max(v) - min(v)) / med * 100:5.1f} %")
    return med


def _b(*ts):
    return float(sum(t.numel() * t.element_size() for t in ts if t is not None))


def _conv_flops(t16, w):
    """2 * voxels * Cout * Cin * k^3 of a conv between a 16-bit tensor [voxels, C16] and the other side of weight w"""
    c16 = t16.shape[-1]
    return 2.0 * (t16.numel() // c16) * w.numel()


# launch name -> (flops, bytes) from the call's arguments
WORK = {
    "conv3d_img_fwd": lambda a: (_conv_flops(a[3], a[1]), _b(a[0], a[1], a[3])),
    "conv3d_img_wgrad": lambda a: (_conv_flops(a[1], a[2]), _b(a[0], a[1], a[2])),
    "conv3d_img_dgrad": lambda a: (_conv_flops(a[0], a[1]), _b(a[0], a[1], a[2])),
    "conv3d_head_fwd": lambda a: (2.0 * a[3].numel() * a[1].numel(), _b(a[0], a[1], a[3])),
    "conv3d_head_bwd": lambda a: (4.0 * a[2].numel() * a[1].numel(), _b(a[0], a[1], a[2], a[3], a[4])),
    "conv_igemm": lambda a: (ops._geom_flops(a[0]), ops._geom_bytes(a[0])),
    "conv_igemm_batch": lambda a: (sum(ops._geom_flops(g) for g in a[0]), 2.0 * a[1].numel() + 2.0 * a[3].numel() + 2.0 * a[2][0].numel()),
    "conv_wgrad_det": lambda a: (ops._geom_flops(a[0]), ops._geom_bytes(a[0], True)),
    "pack_weight": lambda a: (0.0, _b(a[0], a[1], a[2])),
    "bn_act_apply": lambda a: (0.0, _b(a[0], a[4])),
    "bn_act_bwd_reduce": lambda a: (0.0, _b(a[0], a[1])),
    "bn_act_bwd_apply": lambda a: (0.0, _b(a[0], a[1], a[13])),
    "in_stats": lambda a: (0.0, _b(a[0])),
    "in_act_apply": lambda a: (0.0, _b(a[0], a[4])),
    "in_act_bwd": lambda a: (0.0, _b(a[0], a[3], a[7])),
    "colsum": lambda a: (0.0, float(a[3] * a[4] * a[5] * a[10] * 2)),
    "bn_finalize": lambda a: (0.0, 0.0),
    "bn_bwd_coeffs": lambda a: (0.0, 0.0),
}


def fwd_bwd(net, x, dl):
    eng = net.engine

    def run():
        with torch.no_grad():
            logits, ctx = eng.forward(x, True, True)
            eng.backward(ctx, dl, True)
    return run


def per_launch(run, total_us):
    calls = []
    saved = {n: getattr(ops, n) for n in WORK}

    def wrap(n, f):
        def g(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = f(*a, **k)
            e1.record()
            calls.append((n, e0, e1, WORK[n](a)))
            return r
        return g
    for n in WORK:
        setattr(ops, n, wrap(n, saved[n]))
    try:
        acc, work = {}, {}
        for it in range(6):
            calls.clear()
            run()
            torch.cuda.synchronize()
            if it == 0:
                continue
            for i, (n, e0, e1, wk) in enumerate(calls):
                acc.setdefault((i, n), []).append(e0.elapsed_time(e1) * 1e3)
                work[(i, n)] = wk
    finally:
        for n in WORK:
            setattr(ops, n, saved[n])
    say("  per launch (in the plan's order; event pairs around each call, medians of 5; algorithmic work from the shapes):")
    total = 0.0
    for (i, n), v in sorted(acc.items()):
        m = statistics.median(v)
        total += m
        fl, nb = work[(i, n)]
        rate = f"{fl / m / 1e6:8.2f} TFLOP/s" if fl else (f"{nb / m / 1e3:8.1f} GB/s   " if nb else " " * 16)
        say(f"    {i:2d} {n:<20} {m:9.1f} us   {rate}   {fl / 1e9:9.3f} GFLOP {nb / 1e6:9.2f} MB")
    say(f"    sum of the timed launches {total:9.1f} us (the plan end to end: {total_us:.1f} us)")


def bench(netD, N, side=64):
    from semantic_segmentation_amd.models_pix2pix import networks
    name = "NLayerDiscriminator(2, 64, 3)" if netD == "basic" else "PixelDiscriminator(2, 64)"
    say(f"3-D {name}, forward + backward with dx, batch {N}, {side}^3, fp16")
    x = torch.rand(N, 2, side, side, side, device=dev) * 2 - 1
    forms, nets = {}, {}
    for norm in ("batch", "instance"):
        torch.manual_seed(1)
        nets[norm] = networks.define_D(2, 64, netD, norm=norm, threed=True).cuda().train()
        with torch.no_grad():
            shape = nets[norm](x).shape
        dl = torch.randn(shape, device=dev) / shape.numel()
        forms[norm] = fwd_bwd(nets[norm], x, dl)
    med = {k: row(f"{netD} {k}", v) for k, v in interleaved(forms).items()}
    for norm in ("batch", "instance"):
        say(f"  -- {norm} norm")
        per_launch(forms[norm], med[norm])
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    say(f"device {torch.cuda.get_device_name(0)}")
    for netD in ("basic", "pixel"):
        for N in (1, 4):
            bench(netD, N)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
