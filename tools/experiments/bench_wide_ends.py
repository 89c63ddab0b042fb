"""The wide end kernels of the pair forward, timed: gs_conv_widecin_fwd_split against
its HBM floor, gs_conv_smallcin_fwd_split at Cin = 3 beside it for scale, the one-launch head, and the whole training step
of UNet(8, 9) in the default mode (pair forward) and with precise=False (the 16-bit engine, what "auto" ran before the wide end
kernels existed).  Device events, warm-up, medians of repeats, one process, kernels alternated.

    python tools/experiments/bench_wide_ends.py [--kernels] [--step] [--head-bwd] [--step3d] [--once] [--once3d] [--stem-once]
    (--once: three untimed default-mode steps, --stem-once: three launches of the stem per shape -- for a profiler)
--head-bwd: the head's backward for 9 and 64 classes at fp16, batch 8, 256^2 -- the one-launch wide kernels against the
groups-of-four loop they replaced (restated here with ops.conv_smallcout_bwd and the fp32 adds), and the 16-bit forward loop
against the single-plane launch; --step3d / --once3d: the training step of UNet3D(1, 6) on one 64^3 volume."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from semantic_segmentation_amd import ops                                            # noqa: E402

dev = "cuda"
STEM_SHAPES = {"unet_8ch_256": (32, 8, 256, 256, 64), "unet3d_2ch_128": (128, 6, 128, 128, 32)}      # (N, Cin, H, W, Cout)
HBM_TBS = (4.8, 5.9)          # what the project's BatchNorm passes sustain ("What's weak 5")


def timed(fn, reps=9, inner=10, warm=3):
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


def bench_kernels(res):
    for name, (N, Cin, H, W, Cout) in STEM_SHAPES.items():
        x = torch.rand(N, Cin, H, W, device=dev)
        w = (torch.rand(Cout, Cin, 3, 3, device=dev) * 2 - 1) / (9 * Cin) ** 0.5
        y_hi = torch.empty(N, H, W, Cout, dtype=torch.float16, device=dev)
        y_lo = torch.empty_like(y_hi)
        part = torch.empty(ops.bn_partials_numel(ops.conv_widecin_mtiles(N, H, W), Cout), dtype=torch.float32, device=dev)
        x3, w3 = x[:, :3].contiguous(), w[:, :3].contiguous()
        part3 = torch.empty(ops.bn_partials_numel(ops.conv_smallcin_mtiles(N, H, W), Cout), dtype=torch.float32, device=dev)
        forms = {"mfma": lambda: ops.conv_widecin_fwd_split(x, w, y_hi, y_lo, part),
                 "smallcin_cin3": lambda: ops.conv_smallcin_fwd_split(x3, w3, y_hi, y_lo, part3, 3, 1)}
        t = {k: [] for k in forms}
        for rnd in range(3):                                                          # alternate the forms
            for k, f in forms.items():
                t[k] += timed(f, reps=3)
        gbytes = N * H * W * (Cin * 4 + Cout * 4) / 1e9
        floor = [gbytes / r * 1e3 for r in HBM_TBS]                                   # us at 4.8 / 5.9 TB/s
        r = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in t.items()}
        r["bytes_GB"] = gbytes
        r["hbm_floor_us"] = floor
        r["mfma_over_floor"] = [r["mfma"]["median_us"] / f for f in floor]
        r["mfma_tflops"] = 2.0 * N * H * W * 9 * Cin * Cout / r["mfma"]["median_us"] / 1e6
        res["stem_" + name] = r
        print("stem", name, json.dumps(r), flush=True)
    N, H, W = 8, 256, 256
    v = torch.randn(N, H, W, 64, device=dev)
    x_hi = v.half()
    x_lo = (v - x_hi.float()).half()
    for ncls in (4, 9, 64):
        wgt = torch.randn(ncls, 64, device=dev) / 8
        b = torch.zeros(ncls, device=dev)
        logits = torch.empty(N, ncls, H, W, device=dev)
        t = timed(lambda: ops.head1x1_fwd_split(x_hi, x_lo, wgt, b, logits))
        res[f"head_{ncls}"] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                               "bytes_GB": N * H * W * (256 + 4 * ncls) / 1e9}
        print("head", ncls, json.dumps(res[f"head_{ncls}"]), flush=True)


def head_bwd_forms(ncls, N=8, H=256, W=256):
    """(new, old) closures over one set of tensors: the whole head backward (dz, dw, db) both ways"""
    z = torch.randn(N, H, W, 64, device=dev).half()
    wgt = torch.randn(ncls, 64, device=dev) / 8
    w4 = wgt.view(ncls, 64, 1, 1)
    dl = torch.randn(N, ncls, H, W, device=dev)
    dz = torch.empty(N, H, W, 64, dtype=torch.float16, device=dev)
    dw, db = torch.zeros(ncls, 64, device=dev), torch.zeros(ncls, device=dev)
    dw4 = dw.view(ncls, 64, 1, 1)
    b = torch.zeros(ncls, device=dev)
    logits = torch.empty(N, ncls, H, W, device=dev)

    def new_bwd():
        ops.head1x1_wide_bwd(z, wgt, dl, dz, dw, db, gscale=1.0)

    def old_bwd():
        dzs = torch.zeros((N, H, W, 64), dtype=torch.float32, device=dev)
        for g0 in range(0, ncls, 4):
            g1 = min(g0 + 4, ncls)
            dzg = torch.empty(N, H, W, 64, dtype=torch.float16, device=dev)
            ops.conv_smallcout_bwd(z, w4[g0:g1].contiguous(), dl[:, g0:g1].contiguous(), dzg, dw4[g0:g1], db[g0:g1], gscale=1.0)
            dzs += dzg
        return dzs.half()

    def new_fwd():
        ops.head1x1_wide_fwd(z, wgt, b, logits)

    def old_fwd():
        for g0 in range(0, ncls, 4):
            g1 = min(g0 + 4, ncls)
            tmp = torch.empty(N, g1 - g0, H, W, dtype=torch.float32, device=dev)
            ops.conv_smallcout_fwd(z, w4[g0:g1].contiguous(), b[g0:g1].contiguous(), tmp)
            logits[:, g0:g1] = tmp

    return {"bwd_wide": new_bwd, "bwd_groups_of_4": old_bwd, "fwd16_wide": new_fwd, "fwd16_groups_of_4": old_fwd,
            "bwd_wide_dz_only": lambda: ops.head1x1_wide_bwd(None, wgt, dl, dz, None, None),
            "bwd_wide_dw_db_only": lambda: ops.head1x1_wide_bwd(z, wgt, dl, None, dw, db, gscale=1.0)}


def bench_head_bwd(res):
    N, H, W = 8, 256, 256
    M = N * H * W
    for ncls in (9, 64):
        forms = head_bwd_forms(ncls, N, H, W)
        t = {k: [] for k in forms}
        for rnd in range(3):                                                          # alternate the forms
            for k, f in forms.items():
                t[k] += timed(f, reps=3, inner=5, warm=2)
        r = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in t.items()}
        groups = -(-ncls // 4)
        # bytes each form moves: dl fp32 read by both gradients, z read by the weight gradient, dz written once (wide); per group the
        # loop reads z again, writes a 16-bit dz, and the fp32 sum tensor is read and written (+ zero fill, + the final cast)
        wide = M * (2 * ncls * 4 + 128 + 128)
        loop = M * (2 * ncls * 4 + 2 * ncls * 4 + groups * (128 + 128 + 128 + 256 + 256) + 256 + 256 + 128)
        r["bytes_GB"] = {"bwd_wide": wide / 1e9, "bwd_groups_of_4": loop / 1e9,
                         "fwd16_wide": M * (128 + 4 * ncls) / 1e9, "fwd16_groups_of_4": M * (groups * 128 + 3 * 4 * ncls) / 1e9}
        r["hbm_floor_us"] = {k: [v / tb * 1e3 for tb in HBM_TBS] for k, v in r["bytes_GB"].items()}
        res[f"head_bwd_{ncls}"] = r
        print("head_bwd", ncls, json.dumps(r), flush=True)


def make_step3d():
    from semantic_segmentation_amd.losses import seg_loss
    from semantic_segmentation_amd.unet3d import UNet3D
    torch.manual_seed(0)
    net = UNet3D(1, 6).cuda().train()
    x = torch.randn(1, 1, 64, 64, 64, device=dev)
    mask = torch.randint(0, 6, (1, 64 * 64, 64), device=dev)

    def step():
        for p in net.parameters():
            p.grad = None
        seg_loss(net(x).reshape(1, 6, 64 * 64, 64), mask).backward()
    return step


def bench_step3d(res):
    t = timed(make_step3d(), reps=9, inner=5, warm=3)
    res["step_unet3d_1_6_64cubed_default"] = {"median_ms": statistics.median(t) / 1e3, "min_ms": min(t) / 1e3, "max_ms": max(t) / 1e3}
    print("step3d", json.dumps(res["step_unet3d_1_6_64cubed_default"]), flush=True)


def make_step(precise):
    from semantic_segmentation_amd.losses import seg_loss
    from semantic_segmentation_amd.unet import UNet
    torch.manual_seed(0)
    net = (UNet(8, 9) if precise is None else UNet(8, 9, precise=precise)).cuda().train()
    x = torch.randn(8, 8, 256, 256, device=dev)
    mask = torch.randint(0, 9, (8, 1, 256, 256), device=dev)

    def step():
        for p in net.parameters():
            p.grad = None
        seg_loss(net(x), mask).backward()
    return step


def bench_step(res):
    steps = {"default": make_step(None), "precise_false": make_step(False)}
    t = {k: [] for k in steps}
    for rnd in range(3):
        for k, f in steps.items():
            t[k] += timed(f, reps=3, inner=5, warm=3 if rnd == 0 else 1)
    for k, v in t.items():
        res["step_unet_8_9_b8_256_" + k] = {"median_ms": statistics.median(v) / 1e3, "min_ms": min(v) / 1e3, "max_ms": max(v) / 1e3}
        print("step", k, json.dumps(res["step_unet_8_9_b8_256_" + k]), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--once", action="store_true", help="three untimed default-mode steps (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--stem-once", action="store_true", help="three untimed launches of the stem at each benchmark shape (for counters)")
    ap.add_argument("--head-bwd", action="store_true", help="the wide head backward / 16-bit forward against the groups-of-four loops")
    ap.add_argument("--step3d", action="store_true", help="the training step of UNet3D(1, 6) at 64^3, default mode")
    ap.add_argument("--once3d", action="store_true", help="three untimed UNet3D(1, 6) 64^3 steps (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured on the CPU")
    res = {}
    if a.once:
        f = make_step(None)
        for _ in range(3):
            f()
        torch.cuda.synchronize()
    if a.stem_once:
        for N, Cin, H, W, Cout in STEM_SHAPES.values():
            x = torch.rand(N, Cin, H, W, device=dev)
            w = (torch.rand(Cout, Cin, 3, 3, device=dev) * 2 - 1) / (9 * Cin) ** 0.5
            y_hi = torch.empty(N, H, W, Cout, dtype=torch.float16, device=dev)
            y_lo = torch.empty_like(y_hi)
            part = torch.empty(ops.bn_partials_numel(ops.conv_widecin_mtiles(N, H, W), Cout), dtype=torch.float32, device=dev)
            for _ in range(3):
                ops.conv_widecin_fwd_split(x, w, y_hi, y_lo, part)
        torch.cuda.synchronize()
    if a.once3d:
        f = make_step3d()
        for _ in range(3):
            f()
        torch.cuda.synchronize()
    if a.kernels:
        bench_kernels(res)
    if a.head_bwd:
        bench_head_bwd(res)
    if a.step3d:
        bench_step3d(res)
    if a.step:
        bench_step(res)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
