"""Times the 3-D Pix2Pix generator, define_G(1, 1, 64, 'unet_128', threed=True, upsampling='linear'), at 64^3, batch 1 and 2, both
norms: the training forward and forward + backward (medians of 5 windows of `reps` calls, the four configurations interleaved window
by window), the share of each launch family in one forward + backward (device events around every call the plan makes: cells,
up-convs, upsample, norm passes, tail), and the tail kernels beside the route they replace (the generic engine with C_out
zero-padded to 8, then the tanh pass, then NHWC -> NCDHW; backward: the reverse), alternating.  profiles/gen3d_time.txt is this
script's output.  First measurements: nothing asserts a time.

Usage:  python tools/bench_gen3d.py [--dtype f16|bf16] [--reps 20] [--ngf 64]"""
import argparse
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_segmentation_amd import ops  # noqa: E402
from semantic_segmentation_amd._lib import ACT_TANH  # noqa: E402
from semantic_segmentation_amd.models_pix2pix import generator3d_engine as g3e  # noqa: E402
from semantic_segmentation_amd.models_pix2pix import networks, networks3d  # noqa: E402
from semantic_segmentation_amd.models_pix2pix.pix2pix_engine import conv_wgrad, pack_conv  # noqa: E402

SIDE = 64


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(fns, reps, rounds=5):
    """{name: (median, min, max) ms per call}: every round times each function once, in turn"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(window(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def fmt(t):
    med, lo, hi = t
    return f"{med:8.3f} ms  (min {lo:8.3f} max {hi:8.3f}, spread {100 * (hi - lo) / med:4.1f} %)"


# ---------------------------------------------------------------------------------------------------- launch families
class Families:
    """device events around every call the plan makes, by family"""
    OPS = {"bn_act_apply": "norm passes", "in_act_apply": "norm passes", "colsum": "norm passes", "conv3d_tail_fwd": "tail",
           "conv3d_tail_bwd": "tail"}
    CE = {"gather": "cells", "merge_packs": "cells", "wgrad_split": "cells", "dgrad": "cells", "upsample_forward": "upsample",
          "upsample_backward": "upsample"}
    HERE = {"conv_wgrad": "up-convs", "pack_conv": "up-convs", "norm_act_bwd": "norm passes", "instance_stats": "norm passes",
            "bn_coeffs": "norm passes"}

    def __init__(self):
        self.records = []
        self.saved = {}

    def wrap(self, fn, fam):
        def timed(*a, **kw):
            f = fam(*a) if callable(fam) else fam
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            self.records.append((f, e0, e1))
            return r
        return timed

    def proxy(self, mod, table, extra=None):
        p = types.SimpleNamespace(**{k: getattr(mod, k) for k in dir(mod) if not k.startswith("__")})
        for k, fam in table.items():
            setattr(p, k, self.wrap(getattr(mod, k), fam))
        for k, fam in (extra or {}).items():
            setattr(p, k, self.wrap(getattr(mod, k), fam))
        return p

    def __enter__(self):
        self.saved = {k: getattr(g3e, k) for k in ("ops", "ce", *self.HERE)}
        # conv_igemm serves the cells' forward (64 gathered taps at most, never 27) and the up-convs' forward / data gradient (27)
        g3e.ops = self.proxy(ops, self.OPS, {"conv_igemm": lambda g, *a: "up-convs" if g.ntaps == 27 else "cells"})
        g3e.ce = self.proxy(g3e.ce, self.CE)
        for k, fam in self.HERE.items():
            setattr(g3e, k, self.wrap(self.saved[k], fam))
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(g3e, k, v)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for fam, e0, e1 in self.records:
            d = out.setdefault(fam, [0, 0.0])
            d[0] += 1
            d[1] += e0.elapsed_time(e1)
        return out


# ---------------------------------------------------------------------------------------------------- the tail and its route
def tail_beside_route(N, cin, tdt, reps):
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    D = H = W = SIDE
    v = torch.randn((N * D, H, W, cin), device=dev, generator=g).to(tdt)
    w = torch.randn((1, cin, 3, 3, 3), device=dev, generator=g) * (27 * cin) ** -0.5
    b = torch.zeros(1, device=dev)
    out = torch.empty((N, 1, D, H, W), device=dev)
    dout = torch.randn(out.shape, device=dev, generator=g) / out.numel()
    S = float(2 ** round(torch.log2(torch.tensor(float(out.numel()))).item()))
    dv, dw, db = torch.empty_like(v), torch.empty_like(w), torch.empty(1, device=dev)
    ws = torch.empty(int(ops._lib.load().gs_conv3d_tail_bwd_ws_floats(N, D, H, W, cin, 1)), device=dev)
    # the route: C_out padded to 8 on the generic engine
    w8 = torch.zeros((8, cin, 3, 3, 3), device=dev)
    w8[:1] = w
    b8 = torch.zeros(8, device=dev)
    wf, wd = pack_conv(w8, tdt, view=ops.conv3d_weight_view)
    gf = ops.geom_conv3d(N, D, H, W, cin, 8, 3, 1, 1)
    gd = ops.geom_conv3d_dgrad_s1(N, D, H, W, cin, 8, 3, 1)
    u8, t8, dt8, du8 = (torch.zeros((N * D, H, W, 8), device=dev, dtype=tdt) for _ in range(4))
    colws, db8 = torch.empty(1024 * 8, device=dev), torch.empty(8, device=dev)

    def tail_fwd():
        ops.conv3d_tail_fwd(v, w, b, out, ACT_TANH)

    def route_fwd():
        ops.conv_igemm(gf, v, wf, u8, b8)
        ops.bn_act_apply(u8, None, None, ACT_TANH, t8, 8, 0)
        ops.nhwc_to_nchw(t8, out.view(N, 1, D * H, W), 8, 0)

    def tail_bwd():
        ops.conv3d_tail_bwd(v, w, out, dout, dv, dw, db, ACT_TANH, S, ws)

    def route_bwd():
        ops.nchw_to_nhwc((dout * S).view(N, 1, D * H, W), dt8, 8, 0)
        ops.bn_act_bwd_apply(u8, dt8, 8, 0, None, None, None, None, None, None, None, ACT_TANH, False, du8)
        conv_wgrad(gf, v, du8, w8, 8, cin, 27, 1.0 / S)
        ops.colsum(du8, 8, 0, N * D, H, W, 0, 0, H, W, 8, 1.0 / S, colws, db8)
        ops.conv_igemm(gd, du8, wd, dv)

    tail_fwd()
    t = interleaved({"tail forward": tail_fwd, "route forward": route_fwd, "tail backward": tail_bwd, "route backward": route_bwd}, reps)
    nb_f = v.numel() * 2.0 + out.numel() * 4.0
    nb_b = v.numel() * 4.0 + out.numel() * 8.0
    print(f"  tail {cin} -> 1 @ {SIDE}^3, batch {N}: algorithmic bytes forward {nb_f / 1e6:.1f} MB, backward {nb_b / 1e6:.1f} MB")
    for k in t:
        nb = nb_f if "forward" in k else nb_b
        note = f"  {nb / t[k][0] / 1e9:6.2f} TB/s of the tail's algorithmic bytes" if k.startswith("tail") else ""
        print(f"    {k:<16}{fmt(t[k])}{note}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16", choices=("f16", "bf16"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ngf", type=int, default=64)
    a = ap.parse_args()
    os.environ["GSSEG_DTYPE"] = a.dtype
    tdt = ops.DTYPES[a.dtype][1]
    print("device", torch.cuda.get_device_name(0))
    print(f"3-D Pix2Pix generator unet_128 (6 downs) on {SIDE}^3, ngf {a.ngf}, {a.dtype}, train mode; medians of 5 windows of {a.reps} calls, "
          "the configurations interleaved")
    torch.manual_seed(1)
    networks3d.conv_arch = torch.randn(6, 3, device="cuda").requires_grad_(True)
    fns, nets = {}, {}
    for N in (1, 2):
        for norm in ("batch", "instance"):
            net = networks.define_G(1, 1, a.ngf, "unet_128", norm=norm, threed=True, upsampling="linear").cuda().train()
            x = torch.randn((N, 1, SIDE, SIDE, SIDE), device="cuda")
            dense = torch.randn((N, 1, SIDE, SIDE, SIDE), device="cuda") / x.numel()
            nets[(N, norm)] = (net, x, dense)

            def fwd(net=net, x=x):
                return net(x)

            def fwdbwd(net=net, x=x, dense=dense):
                net(x).backward(dense)
            fns[f"batch {N} {norm:<8} forward"] = fwd
            fns[f"batch {N} {norm:<8} forward + backward"] = fwdbwd
    for k, t in interleaved(fns, a.reps).items():
        print(f"  {k:<38}{fmt(t)}")
    print("launch families of one forward + backward (device events around each call; host gaps between calls are not in the shares)")
    for (N, norm), (net, x, dense) in nets.items():
        with Families() as fam:
            net(x).backward(dense)
            s = fam.summary()
        total = sum(v[1] for v in s.values())
        print(f"  batch {N} {norm:<8} " + ", ".join(f"{k} {100 * v[1] / total:4.1f} % ({v[1]:.2f} ms, {v[0]} calls)"
                                                   for k, v in sorted(s.items(), key=lambda kv: -kv[1][1])) + f"; sum {total:.2f} ms")
    print("the tail kernels beside the route they replace (generic engine with C_out zero-padded to 8 + tanh pass + layout pass), alternating")
    for N in (1, 2):
        tail_beside_route(N, a.ngf // 2, tdt, a.reps)


if __name__ == "__main__":
    main()
