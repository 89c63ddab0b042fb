"""gs_conv_ends_to_c16 / gs_conv_ends_to_img / gs_conv_ends_wgrad (csrc/ends.hip), the 7x7 ends of the ResNet generator with the
weights tiled through LDS, at ZERO tolerance on integer operands against torch's fp64 convolution on the CPU.

Operands are integers in {-1, 0, 1}: a forward sum has at most 4 * 49 = 196 terms, so it is an integer below 2^8 -- exact in fp32
and after the one rounding to fp16 or bf16; a weight-gradient sum runs over fewer than 2^12 pixels, exact in fp32 in any order.  Each
kernel is run in both of its roles: pad 0 (the convolution the reference states on the reflection-padded tensor) and pad k-1 with
flipped taps (its data gradient, back onto the padded grid), which autograd's own gradient of F.conv2d states.
Shapes are the smallest that take every path: image channels 1 / 3 / 4; wide channels 8 (one 8-channel group), 24 (not 8 * 2^j),
64 (two weight tiles of 32; one weight-gradient chunk), 72 (a ragged third tile; a second weight-gradient chunk of one group);
planes 3 x 5 (smaller than the kernel once padded back) and 30 x 37 (more than one 1024-pixel tile, ragged); N 1 / 2; fp16 and bf16."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
SHAPES = [(1, 1, 8, 3, 5), (2, 3, 24, 3, 5), (2, 3, 64, 9, 11), (1, 4, 72, 30, 37), (1, 2, 64, 30, 37)]       # N, Cimg, C16, H, W
GS_EINVAL = -1
K = 7


def ints(shape, seed):
    return torch.randint(-1, 2, shape, generator=torch.Generator().manual_seed(seed)).double()


def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).cuda()


def nchw64(t):
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def stem_case(N, Cimg, C16, H, W, seed):
    """y = conv(xp, w) with autograd's gradients for an integer dy: xp is the image already padded by 3"""
    xp = ints((N, Cimg, H + 6, W + 6), seed).requires_grad_(True)
    w = ints((C16, Cimg, K, K), seed + 1).requires_grad_(True)
    y = F.conv2d(xp, w)
    dy = ints(tuple(y.shape), seed + 2)
    dxp, dw = torch.autograd.grad(y, (xp, w), dy)
    return xp.detach(), w.detach(), y.detach(), dy, dxp, dw


def head_case(N, Cimg, C16, H, W, seed):
    tp = ints((N, C16, H + 6, W + 6), seed).requires_grad_(True)
    w = ints((Cimg, C16, K, K), seed + 1).requires_grad_(True)
    b = ints((Cimg,), seed + 3).requires_grad_(True)
    out = F.conv2d(tp, w, b)
    d = ints(tuple(out.shape), seed + 2)
    dtp, dw, db = torch.autograd.grad(out, (tp, w, b), d)
    return tp.detach(), w.detach(), b.detach(), out.detach(), d, dtp, dw, db


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("N,Cimg,C16,H,W", SHAPES)
def test_stem_forward_partials_and_gradients_are_exact(N, Cimg, C16, H, W, dtype):
    from semantic_segmentation_amd import ops
    dt = DTYPES[dtype]
    xp, w, y, dy, dxp, dw = stem_case(N, Cimg, C16, H, W, 11)
    xd, wd = xp.float().cuda(), w.float().cuda()
    mt = ops.conv_ends_mtiles(N, H, W)
    assert mt == -(-N * H * W // 1024)
    outs = []
    for _ in range(2):
        yg = torch.full((N, H, W, C16), float("nan"), dtype=dt, device="cuda")
        part = torch.full((mt, 2, C16), float("nan"), dtype=torch.float32, device="cuda")
        ops.conv_ends_to_c16(xd, wd, yg, part)
        dwg = torch.full((C16, Cimg, K, K), float("nan"), dtype=torch.float32, device="cuda")
        ops.conv_ends_wgrad(nhwc(dy, dt), xd, dwg, None, gscale=0.5)
        dxg = torch.full((N, Cimg, H + 6, W + 6), float("nan"), dtype=torch.float32, device="cuda")
        ops.conv_ends_to_img(nhwc(dy, dt), wd, None, dxg, pad=6, flip=True, w_img_major=False, gscale=0.25)
        outs.append((yg, part, dwg, dxg))
    torch.cuda.synchronize()
    yg, part, dwg, dxg = outs[0]
    assert torch.equal(nchw64(yg), y)
    flat = y.permute(0, 2, 3, 1).reshape(-1, C16)
    for t in range(mt):                                              # the BatchNorm partials of each 1024-pixel tile
        rows = flat[t * 1024:(t + 1) * 1024]
        assert torch.equal(part[t, 0].cpu().double(), rows.sum(0)) and torch.equal(part[t, 1].cpu().double(), (rows * rows).sum(0))
    assert torch.equal(dwg.cpu().double(), 0.5 * dw)
    assert torch.equal(dxg.cpu().double(), 0.25 * dxp)
    assert all(torch.equal(a.view(torch.int16 if a.dtype == dt else torch.int32), b.view(torch.int16 if b.dtype == dt else torch.int32))
               for a, b in zip(outs[0], outs[1]))                    # two runs give equal bits


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("N,Cimg,C16,H,W", SHAPES)
def test_head_forward_and_gradients_are_exact(N, Cimg, C16, H, W, dtype):
    from semantic_segmentation_amd import ops
    dt = DTYPES[dtype]
    tp, w, b, out, d, dtp, dw, db = head_case(N, Cimg, C16, H, W, 21)
    td, wd, dd = nhwc(tp, dt), w.float().cuda(), d.float().cuda()
    outs = []
    for _ in range(2):
        og = torch.full((N, Cimg, H, W), float("nan"), dtype=torch.float32, device="cuda")
        ops.conv_ends_to_img(td, wd, b.float().cuda(), og)
        dtg = torch.full((N, H + 6, W + 6, C16), float("nan"), dtype=dt, device="cuda")
        ops.conv_ends_to_c16(dd, wd, dtg, None, pad=6, flip=True, w_img_major=True)
        dwg = torch.full((Cimg, C16, K, K), float("nan"), dtype=torch.float32, device="cuda")
        dbg = torch.full((Cimg,), float("nan"), dtype=torch.float32, device="cuda")
        ops.conv_ends_wgrad(td, dd, dwg, dbg, pad=6, flip=True, w_img_major=True, gscale=0.5)
        outs.append((og, dtg, dwg, dbg))
    torch.cuda.synchronize()
    og, dtg, dwg, dbg = outs[0]
    assert torch.equal(og.cpu().double(), out)
    assert torch.equal(nchw64(dtg), dtp)
    assert torch.equal(dwg.cpu().double(), 0.5 * dw)
    assert torch.equal(dbg.cpu().double(), 0.5 * db)
    assert all(torch.equal(a.view(torch.int16 if a.dtype == dt else torch.int32), b.view(torch.int16 if b.dtype == dt else torch.int32))
               for a, b in zip(outs[0], outs[1]))


def test_refusals_launch_nothing():
    from semantic_segmentation_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    N, Cimg, C16, H, W = 1, 2, 16, 4, 5
    img = torch.ones((N * Cimg * (H + 6) * (W + 6) + 4,), dtype=torch.float32, device="cuda")
    w = torch.ones((C16 * Cimg * K * K + 4,), dtype=torch.float32, device="cuda")
    t16 = torch.full((N * (H + 6) * (W + 6) * C16 + 16,), 7.0, dtype=torch.float16, device="cuda")
    out = torch.full((max(N * Cimg * (H + 6) * (W + 6), C16 * Cimg * K * K) + 4,), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.full((int(lib.gs_conv_ends_wgrad_ws_floats(N, H + 6, W + 6, Cimg, C16, K)),), 7.0, dtype=torch.float32, device="cuda")

    def c16(imgp=img.data_ptr(), outp=t16.data_ptr(), cimg=Cimg, c=C16, oh=H, ow=W, k=K, pad=0, flip=0, major=0, dtype=0):
        return lib.gs_conv_ends_to_c16(P(imgp), P(w.data_ptr()), P(outp), None, N, cimg, H + 6, W + 6, c, oh, ow, k, pad, flip, major,
                                       dtype, None)

    def toimg(tp=t16.data_ptr(), outp=out.data_ptr(), cimg=Cimg, c=C16, oh=H, ow=W, k=K, pad=0, dtype=0, bias=None):
        return lib.gs_conv_ends_to_img(P(tp), P(w.data_ptr()), bias, P(outp), N, H + 6, W + 6, c, cimg, oh, ow, k, pad, 0, 1, 1.0,
                                       dtype, None)

    def wgrad(tp=t16.data_ptr(), imgp=img.data_ptr(), dwp=out.data_ptr(), wsp=ws.data_ptr(), cimg=Cimg, c=C16, bh=H + 6, k=K, pad=0,
              dtype=0):
        return lib.gs_conv_ends_wgrad(P(tp), P(imgp), P(dwp), None, P(wsp), N, H, W, c, cimg, bh, W + 6, k, pad, 0, 0, 1.0, dtype, None)

    bad = [c16(c=12), c16(c=0), c16(cimg=5), c16(cimg=0), c16(dtype=2), c16(outp=t16.data_ptr() + 8), c16(imgp=img.data_ptr() + 2),
           c16(imgp=0), c16(oh=H + 1), c16(k=8), c16(k=0), c16(pad=7), c16(pad=-1), c16(flip=2), c16(major=2),
           toimg(c=12), toimg(cimg=5), toimg(dtype=3), toimg(tp=t16.data_ptr() + 2), toimg(outp=out.data_ptr() + 1), toimg(ow=W - 1),
           toimg(pad=7), toimg(bias=P(w.data_ptr() + 2)), toimg(outp=0),
           wgrad(c=20), wgrad(cimg=5), wgrad(dtype=2), wgrad(tp=t16.data_ptr() + 4), wgrad(wsp=0), wgrad(bh=H + 5), wgrad(k=9),
           wgrad(dwp=out.data_ptr() + 3)]
    torch.cuda.synchronize()
    assert all(rc == GS_EINVAL for rc in bad), bad
    assert bool((t16 == 7.0).all()) and bool((out == 7.0).all()) and bool((ws == 7.0).all())
    assert c16() == 0 and toimg() == 0 and wgrad() == 0             # and the same calls with sound arguments run
    torch.cuda.synchronize()
