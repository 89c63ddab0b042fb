"""gs_wce_fwd (with and without the label map) and gs_wce_bwd against gs_seg_loss_fwd / gs_seg_loss_bwd on the same logits
(reshaped to [N,C,H,W]; unweighted CE + soft Dice: more arithmetic, three passes over the class planes), at 128^3 with C = 2 and at
64^3 with C = 9, batch 1.  Device events around CALLS back-to-back launches of one entry point (a single launch is shorter than
the launch overhead), WARM warm-up groups per variant, then ROUNDS rounds with the variants alternating inside the one process.
Per variant: mean and min over the rounds of the time per call, the spread (max - min over the rounds) relative to the mean, the
algorithmic bytes (logits read once per pass, target read, dlogits written, labels written where asked for) and those bytes over
the mean time.  Both tensors of either size fit the 256 MiB Infinity Cache: the rates are cache-resident rates, not HBM rates.
Usage: python tools/experiments/wce_time.py [output file]"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from semantic_segmentation_amd import ops

WARM, ROUNDS, CALLS = 3, 12, 200
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def group(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS            # microseconds per call


torch.manual_seed(0)
dev = torch.device("cuda")
for side, C in ((128, 2), (64, 9)):
    S = side ** 3
    x = 2.0 * torch.randn(1, C, S, device=dev)
    t = torch.randint(0, C, (1, S), device=dev).to(torch.uint8)
    w = torch.tensor([(0.004, 0.996)[c % 2] for c in range(C)], dtype=torch.float32, device=dev)
    x4, t3 = x.view(1, C, S // side, side), t.view(1, S // side, side)
    ws_w = torch.empty(ops.wce_ws_floats(), dtype=torch.float32, device=dev)
    ws_s = torch.empty(ops.LOSS_WS, dtype=torch.float32, device=dev)
    out_w, out_s = torch.empty(8, device=dev), torch.empty(8, device=dev)
    lab = torch.empty(1, S, dtype=torch.uint8, device=dev)
    dx = torch.empty_like(x)
    one = torch.ones(1, device=dev)
    ops.wce_fwd(x, t, w, ws_w, out_w)
    ops.seg_loss_fwd(x4, t3, ws_s, out_s)
    fwd_bytes, bwd_bytes = 4 * C * S + S, 8 * C * S + S
    variants = [("gs_wce_fwd", lambda: ops.wce_fwd(x, t, w, ws_w, out_w), fwd_bytes),
                ("gs_wce_fwd + labels", lambda: ops.wce_fwd(x, t, w, ws_w, out_w, lab), fwd_bytes + S),
                ("gs_seg_loss_fwd", lambda: ops.seg_loss_fwd(x4, t3, ws_s, out_s), fwd_bytes),
                ("gs_wce_bwd", lambda: ops.wce_bwd(x, t, w, out_w, one, 1.0, dx), bwd_bytes),
                ("gs_seg_loss_bwd", lambda: ops.seg_loss_bwd(x4, t3, out_s, one, 1.0, dx.view_as(x4)), bwd_bytes)]
    for _, fn, _ in variants:
        for _ in range(WARM):
            group(fn)
    times = {n: [] for n, _, _ in variants}
    for _ in range(ROUNDS):
        for n, fn, _ in variants:
            times[n].append(group(fn))
    for n, _, nbytes in variants:
        v = times[n]
        mean = sum(v) / len(v)
        say(f"{side}^3 C={C}  {n:20s} mean {mean:8.2f} us  min {min(v):8.2f} us  spread {(max(v) - min(v)) / mean * 100:5.1f} %  "
            f"bytes {nbytes / 1e6:8.2f} MB  {nbytes / mean / 1e6:7.3f} TB/s")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
