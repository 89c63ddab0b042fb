"""UNet3D inference, default mode, batch 1: UNet3D(1,2) and UNet3D(1,9) at 64^3 and 128^3 -- the eval forward with BatchNorm folded
into the segment packs, the two-pass eval forward (FOLD_BN_INFERENCE = False), predict (labels from the head), and forward followed by
torch.argmax.  3 warm-up calls per figure, then 20 timed calls each between device events, the variants alternating within the one
process.  On a tree without UNet3D.predict only the forward figures are printed."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from semantic_segmentation_amd.unet import unet_engine
from semantic_segmentation_amd.unet3d import UNet3D

WARM, TIMED = 3, 20


def forward(net, x, fold):
    unet_engine.FOLD_BN_INFERENCE = fold
    try:
        return net(x)
    finally:
        unet_engine.FOLD_BN_INFERENCE = True


for ncls in (2, 9):
    for size in (64, 128):
        torch.manual_seed(0)
        net = UNet3D(1, ncls).cuda().eval()
        x = torch.randn(1, 1, size, size, size, device="cuda")
        variants = [("eval forward folded", lambda: forward(net, x, True)), ("eval forward two-pass", lambda: forward(net, x, False))]
        if hasattr(net, "predict"):
            variants += [("predict", lambda: net.predict(x)), ("forward + argmax", lambda: torch.argmax(forward(net, x, True), 1))]
        total = {n: 0.0 for n, _ in variants}
        best = {n: float("inf") for n, _ in variants}
        with torch.no_grad():
            for _, fn in variants:
                for _ in range(WARM):
                    fn()
            torch.cuda.synchronize()
            for _ in range(TIMED):
                for n, fn in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ms = e0.elapsed_time(e1)
                    total[n] += ms
                    best[n] = min(best[n], ms)
        for n, _ in variants:
            print(f"UNet3D(1,{ncls}) {size}^3  {n:22s} mean {total[n] / TIMED:7.3f} ms  min {best[n]:7.3f} ms", flush=True)
        del net, x
        torch.cuda.empty_cache()
