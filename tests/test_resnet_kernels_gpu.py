"""gs_reflect_norm_apply, gs_reflect_fold_add, gs_reflect_pad_image / gs_reflect_fold_image and the tanh pair (csrc/reflect.hip) at
ZERO tolerance on integer / dyadic operands.

  pad-apply  identity coefficients, no activation: a pure gather -- every 16-bit word of the padded tensor equals the reflected
             source (ReflectionPad2d excludes the edge, so replicate / symmetric / zero padding all differ).  With small-integer
             BatchNorm scale / shift (or InstanceNorm integer means and power-of-two invstd), an integer residual read from the
             interior of a padded tensor whose border holds other numbers, and a keep mask with factor 2, every intermediate is an
             integer below 2^8: exact in fp32 and in both 16-bit types, so the result is the fp64 formula exactly.
  fold+add   integers |d| <= 4: at most nine images and the addend, |sum| <= 40: exact in any order; compared element by element
             with resnet_reference.fold64 (proven the adjoint of F.pad(mode='reflect') by the CPU tests).
  refusals   H <= pad, W <= pad, C % 8, a misaligned pointer, a bad dtype: GS_EINVAL, and the output buffer is untouched.
Shapes: pad 0 / 1 / 3; planes 2 x 2 (the minimum under pad 1), 4 x 4 (the minimum under pad 3), 5 x 7 (odd, not square), 33 x 70 (more
than one block per plane at 64 channels, ragged); C 8 / 64 / 256; N 1 / 3; fp16 and bf16.  Each case runs in well under a second."""
import pytest
import torch
import torch.nn.functional as F

from tests import resnet_reference as rr

pytestmark = pytest.mark.gpu

PLANES = [(0, 2, 2), (1, 2, 2), (0, 4, 4), (1, 4, 4), (3, 4, 4), (0, 5, 7), (1, 5, 7), (3, 5, 7), (0, 33, 70), (1, 33, 70),
          (3, 33, 70)]
NC = [(1, 8), (3, 64), (1, 256)]
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
GS_EINVAL = -1


def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).cuda()


def nchw64(t):
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("N,C", NC)
@pytest.mark.parametrize("p,H,W", PLANES)
def test_pad_apply_is_a_pure_gather(p, H, W, N, C, dtype):
    from semantic_segmentation_amd import ops
    dt = DTYPES[dtype]
    # every representable pattern class: integers, fractions, a subnormal, -0
    y = ints((N, C, H, W), -2000, 2000, 1) / 16.0
    y[0, 0, 0, 0], y[0, 1 % C, H - 1, W - 1] = -0.0, 2.0 ** -20
    y16 = nhwc(y, dt)
    z = torch.full((N, H + 2 * p, W + 2 * p, C), float("nan"), dtype=dt, device="cuda")
    ops.reflect_norm_apply(y16, None, None, ops.NORM_NONE, 0, z, p)
    z2 = torch.full_like(z, float("nan"))
    ops.reflect_norm_apply(y16, None, None, ops.NORM_NONE, 0, z2, p)
    torch.cuda.synchronize()
    src = y16.cpu().permute(0, 3, 1, 2)
    want = src if p == 0 else F.pad(src.float(), [p] * 4, mode="reflect").to(dt)     # (a gather: float and back is the identity)
    assert torch.equal(bits(z.permute(0, 3, 1, 2)), bits(want))
    assert torch.equal(bits(z), bits(z2))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("norm", ["batch", "instance"])
@pytest.mark.parametrize("N,C", NC)
@pytest.mark.parametrize("p,H,W", PLANES)
def test_pad_apply_with_norm_residual_and_keep_is_exact(p, H, W, N, C, norm, dtype):
    from semantic_segmentation_amd import ops
    dt = DTYPES[dtype]
    y = ints((N, C, H, W), -8, 8, 2)
    if norm == "batch":
        a, b = ints((C,), -2, 2, 3), ints((C,), -4, 4, 4)
        v = y * a.view(1, C, 1, 1) + b.view(1, C, 1, 1)
        kind = ops.NORM_BATCH
    else:
        a = ints((N, C), -3, 3, 3)
        b = torch.pow(2.0, ints((N, C), -1, 1, 4))
        v = (y - a.view(N, C, 1, 1)) * b.view(N, C, 1, 1)
        kind = ops.NORM_INSTANCE
    keep = ints((N, C, H, W), 0, 1, 5)
    res = ints((N, C, H + 2, W + 2), -8, 8, 6)                      # padded by 1: its border must NOT be read
    y16, res16 = nhwc(y, dt), nhwc(res, dt)
    keep8 = keep.permute(0, 2, 3, 1).contiguous().to(torch.uint8).cuda()
    ca, cb = a.float().contiguous().cuda(), b.float().contiguous().cuda()
    for act, use_res, use_keep in ((1, False, True), (0, True, False), (1, True, True), (0, False, False)):
        want = v.clamp_min(0) if act else v
        if use_keep:
            want = want * keep * 2.0
        if use_res:
            want = want + res[:, :, 1:-1, 1:-1]
        want = rr.pad64(want, p)
        z = torch.full((N, H + 2 * p, W + 2 * p, C), float("nan"), dtype=dt, device="cuda")
        ops.reflect_norm_apply(y16, ca, cb, kind, act, z, p, res16 if use_res else None, 1, keep8 if use_keep else None, 2.0)
        torch.cuda.synchronize()
        assert torch.equal(nchw64(z), want), (act, use_res, use_keep)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("N,C", NC)
@pytest.mark.parametrize("p,H,W", [s for s in PLANES if s[0] > 0])
def test_fold_add_is_exact(p, H, W, N, C, dtype):
    from semantic_segmentation_amd import ops
    dt = DTYPES[dtype]
    d = ints((N, C, H + 2 * p, W + 2 * p), -4, 4, 7)
    add = ints((N, C, H, W), -4, 4, 8)
    d16, add16 = nhwc(d, dt), nhwc(add, dt)
    for with_add in (False, True):
        out = torch.full((N, H, W, C), float("nan"), dtype=dt, device="cuda")
        out2 = torch.full_like(out, float("nan"))
        ops.reflect_fold_add(d16, out, p, add16 if with_add else None)
        ops.reflect_fold_add(d16, out2, p, add16 if with_add else None)
        torch.cuda.synchronize()
        want = rr.fold64(d, p) + (add if with_add else 0)
        assert torch.equal(nchw64(out), want), with_add
        assert torch.equal(bits(out), bits(out2))


def test_fold_of_ones_counts_the_images():
    """d = 1 everywhere: the fold counts how many padded elements land on each pixel -- 4 next to a corner (the pixel, its row image,
    its column image and the diagonal one), 2 along an edge, 1 inside and on the edge itself; 9 at most where a plane is so small that
    both mirrors reach a pixel."""
    from semantic_segmentation_amd import ops
    for p, H, W in ((1, 5, 7), (3, 8, 9), (3, 4, 4), (1, 2, 2)):
        d16 = torch.ones((1, H + 2 * p, W + 2 * p, 8), dtype=torch.float16, device="cuda")
        out = torch.empty((1, H, W, 8), dtype=torch.float16, device="cuda")
        ops.reflect_fold_add(d16, out, p)
        cnt = nchw64(out)[0, 0]
        assert float(cnt.sum()) == (H + 2 * p) * (W + 2 * p)
        rows = torch.tensor([1 + (1 <= i <= p) + (H - 1 - p <= i <= H - 2) for i in range(H)], dtype=torch.float64)
        cols = torch.tensor([1 + (1 <= j <= p) + (W - 1 - p <= j <= W - 2) for j in range(W)], dtype=torch.float64)
        assert torch.equal(cnt, rows.view(-1, 1) * cols.view(1, -1))


@pytest.mark.parametrize("p,H,W", [(3, 4, 4), (3, 5, 7), (3, 33, 70), (1, 2, 2)])
def test_image_pad_and_fold_are_exact(p, H, W):
    from semantic_segmentation_amd import ops
    x = (ints((3, 2, H, W), -1000, 1000, 9) / 8.0).float().cuda()
    xp = torch.full((3, 2, H + 2 * p, W + 2 * p), float("nan"), device="cuda")
    ops.reflect_pad_image(x, xp, p)
    assert torch.equal(xp.cpu(), F.pad(x.cpu(), [p] * 4, mode="reflect"))
    d = ints((3, 2, H + 2 * p, W + 2 * p), -64, 64, 10)
    dx = torch.full((3, 2, H, W), float("nan"), device="cuda")
    ops.reflect_fold_image(d.float().cuda(), dx, p)
    assert torch.equal(dx.cpu().double(), rr.fold64(d, p))


def test_tanh_pair():
    """t = tanhf(x) against torch's fp64 tanh: the device's tanhf is good to a few fp32 units in the last place of a value below
    one (2^-24 each); 16 of them is 2^-20.  d = S * dout * (1 - t) * (1 + t) on the kernel's own t: 1 - |t| is exact from 0.5 up and
    one rounding below, 1 + |t| and the three products one relative rounding each -- five at most, no cancellation where tanh
    saturates; held to 6 * 2^-24 |d|."""
    from semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.cat((torch.randn(70001, generator=g) * 2, torch.tensor([0.0, -0.0, 20.0, -20.0, 1e-8]))).cuda()
    t = torch.empty_like(x)
    ops.tanh_fwd(x, t)
    assert float((t.cpu().double() - torch.tanh(x.cpu().double())).abs().max()) <= 2.0 ** -20
    dout = torch.randn(x.shape, generator=g).cuda()
    d = torch.empty_like(x)
    ops.tanh_bwd(t, dout, 1024.0, d)
    t64, do64 = t.cpu().double(), dout.cpu().double()
    want = 1024.0 * do64 * (1 - t64 * t64)
    bound = 6 * 2.0 ** -24 * want.abs() + 2.0 ** -126
    assert bool(((d.cpu().double() - want).abs() <= bound).all())
    ops.tanh_fwd(x, x)                                             # in place
    assert torch.equal(x, t)


def test_refusals_launch_nothing():
    import ctypes
    from semantic_segmentation_amd import _lib
    lib = _lib.load()
    N, H, W, C = 1, 3, 5, 16
    y = torch.ones((N, H, W, C + 8), dtype=torch.float16, device="cuda")
    z = torch.full((N, H + 6, W + 6, C + 8), 7.0, dtype=torch.float16, device="cuda")
    coef = torch.ones(64, dtype=torch.float32, device="cuda")
    keep = torch.ones(N * H * W * C + 8, dtype=torch.uint8, device="cuda")
    P = ctypes.c_void_p

    def apply(yp=y.data_ptr(), zp=z.data_ptr(), a=None, b=None, norm=0, act=0, res=None, keepp=None, pad=1, h=H, w=W, c=C, dtype=0):
        return lib.gs_reflect_norm_apply(P(yp), a, b, norm, act, res, 1, keepp, 2.0, P(zp), pad, N, h, w, c, dtype, None)

    def fold(dp=z.data_ptr(), addp=None, outp=y.data_ptr(), pad=1, h=H, w=W, c=C, dtype=0):
        return lib.gs_reflect_fold_add(P(dp), addp, P(outp), pad, N, h, w, c, dtype, None)

    bad = [apply(pad=3), apply(pad=5, h=8, w=5), apply(pad=1, h=1), apply(pad=1, w=1), apply(c=12), apply(c=0), apply(dtype=2),
           apply(yp=y.data_ptr() + 2), apply(zp=z.data_ptr() + 8), apply(res=P(y.data_ptr() + 4)), apply(keepp=P(keep.data_ptr() + 1)),
           apply(norm=1), apply(norm=1, a=P(coef.data_ptr()), b=P(coef.data_ptr() + 4)), apply(norm=0, a=P(coef.data_ptr())),
           apply(norm=3), apply(act=2), apply(pad=-1), apply(pad=9, h=16, w=16),
           fold(pad=3), fold(pad=1, h=1), fold(c=12), fold(dtype=5), fold(dp=z.data_ptr() + 2), fold(outp=y.data_ptr() + 6),
           fold(addp=P(y.data_ptr() + 2)),
           lib.gs_reflect_pad_image(P(coef.data_ptr()), P(z.data_ptr()), 3, 1, 1, 3, 8, None),
           lib.gs_reflect_pad_image(P(coef.data_ptr() + 2), P(z.data_ptr()), 1, 1, 1, 3, 8, None),
           lib.gs_reflect_fold_image(P(z.data_ptr()), P(coef.data_ptr()), 3, 1, 1, 8, 3, None),
           lib.gs_tanh_fwd(None, P(coef.data_ptr()), 4, None), lib.gs_tanh_bwd(P(coef.data_ptr()), None, 1.0, P(coef.data_ptr()), 4, None)]
    torch.cuda.synchronize()
    assert all(rc == GS_EINVAL for rc in bad), bad
    assert b"Padding size should be less than the corresponding input dimension" in (apply(pad=3), lib.gs_last_error())[1]
    assert bool((z == 7.0).all()) and bool((y == 1.0).all()) and bool((coef == 1.0).all())
    assert apply() == 0 and fold() == 0                            # and the same calls with sound arguments run
    torch.cuda.synchronize()
