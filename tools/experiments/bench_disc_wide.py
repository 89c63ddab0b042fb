"""The image-side conv of 5..16 channels (csrc/ends_img.hip) and the discriminators that use it, timed:

  kernels   at 256^2, batch 2 and batch 32, ndf 64: gs_conv_imgwide_fwd / _wgrad / _dgrad at 6 channels beside the direct kernels
            gs_conv_smallcin_fwd / _wgrad / _dgrad at 4 channels on the same shape, interleaved rounds in one process; per kernel
            the median, the spread over the rounds, the algorithmic bytes and the bytes/s achieved
  patchgan  NLayerDiscriminator(6 | 4, 64, 3) under InstanceNorm, forward + backward (need_dx), same interleaving
  pixel     PixelDiscriminator(6, 64) under BatchNorm and InstanceNorm, forward + backward, and a per-launch breakdown of the
            BatchNorm plan (each launch of the plan timed on its own, in the plan's order)

    python tools/experiments/bench_disc_wide.py [--out profiles/disc_wide_time.txt]
Device events, warm-up, medians; figures of one process on one GPU."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from semantic_segmentation_amd import ops                                            # noqa: E402
from semantic_segmentation_amd._lib import ACT_LEAKY02                               # noqa: E402

dev = "cuda"
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps=3, inner=10, warm=2):
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


def interleaved(forms, rounds=5, **kw):
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            t[k] += timed(f, **kw)
    return t


def row(name, v, nbytes=None):
    med = statistics.median(v)
    s = f"  {name:<34} median {med:9.1f} us   min {min(v):9.1f}   max {max(v):9.1f}   spread {(max(v) - min(v)) / med * 100:5.1f} %"
    if nbytes is not None:
        s += f"   {nbytes / 1e6:8.1f} MB   {nbytes / med / 1e6:6.2f} TB/s"
    say(s)
    return med


def bench_kernels(N):
    H = W = 256
    Cout, k, s, p = 64, 4, 2, 1
    OH = OW = 128
    say(f"kernels, batch {N}, {H} x {W}, Cout {Cout}, k4/s2/p1, fp16 (algorithmic bytes: image fp32 + 16-bit tensor + weights)")
    forms, nbytes = {}, {}
    for cin in (6, 4):
        x = torch.rand(N, cin, H, W, device=dev)
        w = (torch.rand(Cout, cin, k, k, device=dev) * 2 - 1) / (16 * cin) ** 0.5
        b = torch.zeros(Cout, device=dev)
        y = torch.empty(N, OH, OW, Cout, dtype=torch.float16, device=dev)
        dy = torch.randn(N, OH, OW, Cout, device=dev).half()
        dwt = torch.zeros_like(w)
        dx = torch.empty_like(x)
        io = N * cin * H * W * 4 + N * OH * OW * Cout * 2 + w.numel() * 4
        tag = f"cin{cin} " + ("imgwide" if cin > 4 else "smallcin")
        if cin > 4:
            ws = ops.conv_imgwide_wgrad_ws(N, OH, OW, cin, Cout, k, dev)
            forms[tag + " fwd"] = lambda x=x, w=w, b=b, y=y: ops.conv_imgwide_fwd(x, w, b, y, k, s, p, ACT_LEAKY02)
            forms[tag + " wgrad"] = lambda x=x, dy=dy, dwt=dwt, ws=ws: ops.conv_imgwide_wgrad(x, dy, dwt, k, s, p, 1.0, ws)
            forms[tag + " dgrad"] = lambda dy=dy, w=w, dx=dx: ops.conv_imgwide_dgrad(dy, w, dx, k, s, p, 1.0)
        else:
            forms[tag + " fwd"] = lambda x=x, w=w, b=b, y=y: ops.conv_smallcin_fwd(x, w, b, y, None, k, s, p, ACT_LEAKY02)
            forms[tag + " wgrad"] = lambda x=x, dy=dy, dwt=dwt: ops.conv_smallcin_wgrad(x, dy, dwt, k, s, p, 1.0)
            forms[tag + " dgrad"] = lambda dy=dy, w=w, dx=dx: ops.conv_smallcin_dgrad(dy, w, dx, k, s, p, 1.0)
        for op in ("fwd", "wgrad", "dgrad"):
            nbytes[f"{tag} {op}"] = io
    t = interleaved(forms)
    med = {name: row(name, v, nbytes[name]) for name, v in t.items()}
    for op in ("fwd", "wgrad", "dgrad"):
        a, b4 = f"cin6 imgwide {op}", f"cin4 smallcin {op}"
        say(f"  {op}: ns per byte  6 ch {med[a] * 1e3 / nbytes[a]:.5f}   4 ch {med[b4] * 1e3 / nbytes[b4]:.5f}   "
            f"ratio {med[a] / nbytes[a] / (med[b4] / nbytes[b4]):.2f}")
    say()


def fwd_bwd(net, x, dl):
    eng = net.engine

    def run():
        with torch.no_grad():
            logits, ctx = eng.forward(x, True, True)
            eng.backward(ctx, dl, True)
    return run


def bench_patchgan(N):
    from semantic_segmentation_amd.models_pix2pix import networks
    say(f"PatchGAN (ndf 64, 3 layers, InstanceNorm), forward + backward with dx, batch {N}, 256 x 256, fp16")
    forms = {}
    for cin in (6, 4):
        torch.manual_seed(1)
        net = networks.define_D(cin, 64, "basic", norm="instance").cuda().train()
        x = torch.rand(N, cin, 256, 256, device=dev)
        with torch.no_grad():
            shape = net(x).shape
        dl = torch.randn(shape, device=dev) / shape.numel()
        forms[f"patchgan cin{cin}"] = fwd_bwd(net, x, dl)
    for name, v in interleaved(forms, inner=5).items():
        row(name, v)
    say()


def bench_pixel(N):
    from semantic_segmentation_amd.models_pix2pix import networks
    H = W = 256
    say(f"PixelDiscriminator (6 channels, ndf 64), forward + backward with dx, batch {N}, {H} x {W}, fp16")
    forms, nets = {}, {}
    x = torch.rand(N, 6, H, W, device=dev)
    dl = torch.randn(N, 1, H, W, device=dev) / (N * H * W)
    for norm in ("batch", "instance"):
        torch.manual_seed(1)
        nets[norm] = networks.define_D(6, 64, "pixel", norm=norm).cuda().train()
        forms[f"pixel {norm}"] = fwd_bwd(nets[norm], x, dl)
    med = {name: row(name, v) for name, v in interleaved(forms, inner=5).items()}
    # per launch: wrap every op the plan calls, run the plan under a recorder that times each call with events
    calls = []
    names = [n for n in dir(ops) if callable(getattr(ops, n)) and not n.startswith("_")]
    saved = {n: getattr(ops, n) for n in names}
    launch = {"conv_imgwide_fwd", "conv_igemm", "bn_act_apply", "conv_smallcout_fwd", "conv_smallcout_bwd", "bn_act_bwd_reduce",
              "bn_bwd_coeffs", "bn_act_bwd_apply", "conv_wgrad_det", "conv_imgwide_wgrad", "colsum", "conv_imgwide_dgrad", "bn_finalize",
              "pack_weight", "bn_coeffs_from_partials", "bn_finalize_coeffs"}

    def wrap(n, f):
        def g(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = f(*a, **k)
            e1.record()
            calls.append((n, e0, e1))
            return r
        return g
    run = forms["pixel batch"]
    for n in names:
        if n in launch:
            setattr(ops, n, wrap(n, saved[n]))
    try:
        acc = {}
        for it in range(6):
            calls.clear()
            run()
            torch.cuda.synchronize()
            if it == 0:
                continue
            for i, (n, e0, e1) in enumerate(calls):
                acc.setdefault((i, n), []).append(e0.elapsed_time(e1) * 1e3)
    finally:
        for n in names:
            setattr(ops, n, saved[n])
    say("  per launch (BatchNorm plan, in order; event pairs around each call, medians of 5):")
    total = 0.0
    for (i, n), v in sorted(acc.items()):
        m = statistics.median(v)
        total += m
        say(f"    {i:2d} {n:<22} {m:9.1f} us")
    say(f"    sum of the timed launches {total:9.1f} us (the plan end to end: {med['pixel batch']:.1f} us)")
    # traffic of the intermediate tensors (16-bit elements per pixel, every write and read of the composed plan):
    #   forward   z0 [64] w + r; y1 [128] w + r; z1 [128] w + r                                                   = 640
    #   backward  head: z1 r, dz1 w; BN reduce: y1, dz1 r; BN apply: y1, dz1 r, dy1 w; wgrad: z0, dy1 r; dgrad: dy1 r, dz0 w;
    #             first layer: z0, dz0 r, dy0 w; wgrad, bias sum, dgrad: dy0 r x 3                                 = 1664
    px_ = N * H * W
    inter = px_ * 2 * (640 + 1664)
    ends = px_ * (6 * 4 * 3 + 4 * 2)                            # the image read by fwd and wgrad, dx written; logits and dlogits
    say(f"  algorithmic bytes of the plan: intermediates {inter / 1e6:.0f} MB, image / logits side {ends / 1e6:.0f} MB: "
        f"{100.0 * inter / (inter + ends):.0f} % of the plan's traffic is the two intermediate tensors and their gradients")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    say(f"device {torch.cuda.get_device_name(0)}")
    for N in (2, 32):
        bench_kernels(N)
    for N in (2, 32):
        bench_patchgan(N)
    for N in (2, 32):
        bench_pixel(N)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
