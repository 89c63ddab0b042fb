"""Pair-forward conv + its BatchNorm apply pass, dense lo plane against fragment-order lo plane, per layer.

Each side is timed twice, sides alternated; the difference between two runs of one side is the spread.  The fragment-order side is
kept only where it beats the dense side by more than that spread, conv and apply TOGETHER."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from semantic_segmentation_amd import ops

# (name, H, channels of the input pair, K, wrap, Cout): the "xw" stages of the bs-32 step at 256^2 and the deep "1" stage
LAYERS = [("64->64 @256 xw", 256, 64, 192, 128, 64), ("128->64 @256 xw (K 320)", 256, 128, 320, 192, 64),
          ("128->128 @128 xw", 128, 128, 384, 256, 128), ("512->512 @32 1", 32, 512, 512, 512, 512)]
N = int(os.environ.get("NB", "32"))
dev, dt = torch.device("cuda:0"), torch.float16


def timeit(fn, iters=20):
    fn(); fn(); torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    for _ in range(iters):
        fn()
    e[1].record(); torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]) / iters * 1e3


for name, H, cin, K, wrap, cout in LAYERS:
    x = (torch.randn(N, H, H, 2 * cin, device=dev) * 0.7).to(dt)
    pack = (0.05 * torch.randn(9, cout, K, device=dev)).to(dt)
    y_hi, y_lo = torch.empty(N, H, H, cout, device=dev, dtype=dt), torch.empty(N, H, H, cout, device=dev, dtype=dt)
    z = torch.empty(N, H, H, 2 * cout, device=dev, dtype=dt)
    part = torch.empty(ops.bn_partials_numel(ops.conv3x3_mtiles(N, H, H, cout), cout), device=dev)
    sc, sh = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev)
    res = {0: [], 1: []}
    for rnd in range(2):
        for side in (0, 1):
            ops.pair_lo_set_layout(0 if side == 0 else -1)
            lay = ops.conv3x3_pair_lo_layout(N, H, H, K, cout)
            assert lay == side, (name, side, lay)
            conv = lambda: ops.conv3x3_segs(x, pack, y_hi, y_lo, N, H, H, K, wrap, cin, cout, in_stride=2 * cin, bn_partials=part, lo_layout=lay)
            app = lambda: ops.bn_act_apply_split(y_hi, y_lo, sc, sh, 1, z, z[..., cout:], 2 * cout, 0, lo_layout=lay)
            res[side].append((timeit(conv), timeit(app), timeit(lambda: (conv(), app()))))
    ops.pair_lo_set_layout(-1)
    for side, tag in ((0, "dense   "), (1, "fragment")):
        print(f"{name:26s} {tag} " + "  ".join(f"conv {c:7.1f} apply {a:6.1f} both {b:7.1f} us" for c, a, b in res[side]), flush=True)
    d, f = [b for _, _, b in res[0]], [b for _, _, b in res[1]]
    spread = max(abs(d[0] - d[1]), abs(f[0] - f[1]))
    print(f"{name:26s} gain {min(d) - max(f):+7.1f} us (slowest fragment against fastest dense), spread {spread:.1f} us", flush=True)
