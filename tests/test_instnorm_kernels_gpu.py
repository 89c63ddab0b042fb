"""gs_in_stats, gs_in_act_apply and gs_in_act_bwd (csrc/instnorm.hip) against the fp64 statement of tests/instnorm_reference.py.

Operands are integer-valued and exactly representable in the dtype (|y| <= 8, |dz| <= 4; one case: a plane of mean 96 with values
in {95, 96, 97}), so every plane sum is exact in any order and what is left are the roundings of the kernels' own formulas:

  mean      the double mean converted once: exact where H*W is a power of two (the mean is then an fp32 number), else float32(ref) or
            its neighbour.
  invstd    ONE fp32 rounding, the conversion of 1 / sqrt(M2 / HW + eps) formed in double from exact fp32 sums about each thread's
            first pixel joined by Chan's update; the double arithmetic in front of it gets 2^-44:  |d| <= 2^-24 (1 + 2^-20) ref.
  apply     on the kernel's own mean / invstd: xh = (y - mean) * invstd is 2 roundings, the LeakyReLU product 1 (and 0.2f is not
            1 / 5: 1 more), keep * 2 is exact; then the 16-bit store:  |d| <= ulp_dt(ref) / 2 + 4 * 2^-24 |ref|.
  g means   each term in fp32, summed in double, converted once.  g = dz_a * relu' * keep * 2 + dz_b * leaky' is 3 roundings (product
            with 0.2f, 0.2f itself, the sum); g * xh adds the 2 of xh and the product; + 1 for the conversion:
            |d m1| <= 4 * 2^-24 mean|g|,  |d m2| <= 7 * 2^-24 mean|g * xh|   (means over the plane).
  dy        on the kernel's own mean / invstd / g means: invstd * (g - m1 - xh * m2) is at most 8 roundings of its terms, then the
            store:  |d| <= ulp_dt(ref) / 2 + 8 * 2^-24 invstd (|g| + |m1| + |xh * m2|).
Shapes: the smallest plane; an odd plane where a 64-pixel run straddles samples; the PatchGAN's 31 x 31 (two unequal slices); planes
over several blocks (64 x 64, 128 x 128); 8 x 8 (the last plane of one slice at 16 channels); 5 x 13 x 520 (five chunk groups, the
last one channel chunk wide).  Each case runs in well under a second."""
import ctypes

import pytest
import torch

from tests import instnorm_reference as ir

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 2, 136), (3, 3, 3, 8), (2, 31, 31, 24), (2, 64, 64, 16), (1, 128, 128, 8), (2, 8, 8, 16), (2, 5, 13, 520)]
DTYPES = [("f16", torch.float16, 10, -14), ("bf16", torch.bfloat16, 7, -126)]
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))
U = 2.0 ** -24
ACTS = {"none": 0, "relu": 1, "leaky": 2}


def ulp(ref, mant, emin):
    """spacing of the dtype at |ref| (the subnormal spacing below 2^emin)"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.full_like(ref, 2.0), e - mant)


def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).cuda()


def nchw64(t):
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def make_y(shape, seed, offset=False):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    if offset:
        return torch.randint(95, 98, (N, C, H, W), generator=g).double()
    return torch.randint(-8, 9, (N, C, H, W), generator=g).double()


def run_stats(ops, y16):
    N, H, W, C = y16.shape
    mi = torch.full((2, N, C), float("nan"), dtype=torch.float32, device="cuda")
    ops.in_stats(y16, 1e-5, mi[0], mi[1], ops.in_workspace(N, H, W, C, y16.device))
    return mi


def check_stats(shape, dt, y):
    from semantic_segmentation_amd import ops
    N, H, W, C = shape
    mi = run_stats(ops, nhwc(y, dt))
    mi2 = run_stats(ops, nhwc(y, dt))
    torch.cuda.synchronize()
    assert torch.equal(mi, mi2), "two runs give equal bits"
    mean, invstd = mi[0].cpu().double(), mi[1].cpu().double()
    rmean, rvar = y.mean((2, 3)), y.var((2, 3), unbiased=False)
    rinv = 1.0 / torch.sqrt(rvar + EPS32)
    if (H * W) & (H * W - 1) == 0:
        assert torch.equal(mean, rmean), float((mean - rmean).abs().max())
    else:
        assert bool(((mean - rmean).abs() <= 2.0 ** -23 * rmean.abs()).all()), float((mean - rmean).abs().max())
    d = ((invstd - rinv).abs() / rinv).max()
    print(f"stats {shape}: invstd worst {float(d) / U:.3f} roundings")
    assert float(d) <= U * (1 + 2.0 ** -20)
    return mi


@pytest.mark.parametrize("dtn,dt,mant,emin", DTYPES, ids=[d[0] for d in DTYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_in_stats(shape, dtn, dt, mant, emin):
    check_stats(shape, dt, make_y(shape, 1))


@pytest.mark.parametrize("shape", [(2, 16, 16, 8), (2, 3, 3, 8), (1, 128, 128, 8)], ids=lambda s: "x".join(map(str, s)))
def test_in_stats_mean_far_above_spread(shape):
    """values in {95, 96, 97}, exact in bf16: E[y^2] - mean^2 in fp32 would lose the variance (9216 against 2/3)"""
    check_stats(shape, torch.bfloat16, make_y(shape, 2, offset=True))


@pytest.mark.parametrize("dtn,dt,mant,emin", DTYPES, ids=[d[0] for d in DTYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_in_act_apply(shape, dtn, dt, mant, emin):
    """LeakyReLU into the second half of a NaN-filled buffer of twice the width with a keep mask times 2, and ReLU as the second
    output into the first half of another: the other halves stay NaN"""
    from semantic_segmentation_amd import ops
    N, H, W, C = shape
    y = make_y(shape, 3)
    y16 = nhwc(y, dt)
    mi = run_stats(ops, y16)
    keep = (torch.rand((N, H, W, C), generator=torch.Generator().manual_seed(4)) >= 0.5).to(torch.uint8).cuda()

    def run():
        z = torch.full((N, H, W, 2 * C), float("nan"), dtype=dt, device="cuda")
        z2 = torch.full((N, H, W, 2 * C), float("nan"), dtype=dt, device="cuda")
        ops.in_act_apply(y16, mi[0], mi[1], ACTS["leaky"], z, 2 * C, C, keep, 2.0, z2=z2, act2=ACTS["relu"], z2_stride=2 * C, z2_coff=0)
        return z, z2
    (z, z2), (zb, z2b) = run(), run()
    torch.cuda.synchronize()
    assert torch.equal(z.view(torch.int16), zb.view(torch.int16)) and torch.equal(z2.view(torch.int16), z2b.view(torch.int16))
    assert bool(z[..., :C].isnan().all()) and bool(z2[..., C:].isnan().all()), "channels outside the written range were touched"
    mean, invstd = mi[0].cpu().double(), mi[1].cpu().double()
    for got, ref in ((nchw64(z[..., C:]), ir.in_act_apply64(y, mean, invstd, "leaky", nchw64(keep), 2.0)),
                     (nchw64(z2[..., :C]), ir.in_act_apply64(y, mean, invstd, "relu"))):
        bound = ulp(ref, mant, emin) / 2 + 4 * U * ref.abs()
        bad = ~((got - ref).abs() <= bound)
        assert not bool(bad.any()), (int(bad.sum()), float(((got - ref).abs() / bound.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("dtn,dt,mant,emin", DTYPES, ids=[d[0] for d in DTYPES])
@pytest.mark.parametrize("both", [True, False], ids=["two_consumers_keep", "one_consumer"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_in_act_bwd(shape, both, dtn, dt, mant, emin):
    """dz_a strided (second half of a buffer of twice the width) through ReLU with a keep mask times 2, dz_b dense through LeakyReLU;
    or dz_a alone through LeakyReLU, dense"""
    from semantic_segmentation_amd import ops
    N, H, W, C = shape
    g = torch.Generator().manual_seed(5)
    y = make_y(shape, 6)
    y16 = nhwc(y, dt)
    mi = run_stats(ops, y16)
    dza = torch.randint(-4, 5, (N, C, H, W), generator=g).double()
    dzb = torch.randint(-4, 5, (N, C, H, W), generator=g).double() if both else None
    keep = (torch.rand((N, H, W, C), generator=g) >= 0.5).to(torch.uint8).cuda() if both else None
    if both:
        buf = torch.full((N, H, W, 2 * C), float("nan"), dtype=dt, device="cuda")
        buf[..., C:] = nhwc(dza, dt)
        sa, ca, act = 2 * C, C, "relu"
    else:
        buf, sa, ca, act = nhwc(dza, dt), C, 0, "leaky"
    dzb16 = nhwc(dzb, dt) if both else None

    def run():
        dy = torch.full((N, H, W, C), float("nan"), dtype=dt, device="cuda")
        gm = torch.full((2, N, C), float("nan"), dtype=torch.float32, device="cuda")
        ops.in_act_bwd(y16, mi[0], mi[1], buf, sa, ca, ACTS[act], dy, gm, ops.in_workspace(N, H, W, C, "cuda"), dz_b=dzb16,
                       act_b=ACTS["leaky"], keep_mask=keep, keep_scale=2.0 if both else 1.0)
        return dy, gm
    (dy, gm), (dyb, gmb) = run(), run()
    torch.cuda.synchronize()
    assert torch.equal(dy.view(torch.int16), dyb.view(torch.int16)) and torch.equal(gm, gmb), "two runs give equal bits"
    mean, invstd = mi[0].cpu().double(), mi[1].cpu().double()
    k64 = nchw64(keep) if both else None
    _, m1, m2 = ir.in_act_bwd64(y, mean, invstd, dza, act, dz_b=dzb, act_b="leaky", keep=k64, kscale=2.0 if both else 1.0)
    xh = (y - ir._pl(mean)) * ir._pl(invstd)
    ga = ir.act_bwd64(dza, xh, act)
    gg = (ga * k64 * 2.0 + ir.act_bwd64(dzb, xh, "leaky")) if both else ga
    got1, got2 = gm[0].cpu().double(), gm[1].cpu().double()
    b1, b2 = 4 * U * gg.abs().mean((2, 3)), 7 * U * (gg * xh).abs().mean((2, 3))
    assert bool(((got1 - m1).abs() <= b1).all()), float(((got1 - m1).abs() / b1.clamp_min(1e-300)).max())
    assert bool(((got2 - m2).abs() <= b2).all()), float(((got2 - m2).abs() / b2.clamp_min(1e-300)).max())
    ref = ir._pl(invstd) * (gg - ir._pl(got1) - xh * ir._pl(got2))
    bound = ulp(ref, mant, emin) / 2 + 8 * U * ir._pl(invstd) * (gg.abs() + ir._pl(got1).abs() + (xh * ir._pl(got2)).abs())
    got = nchw64(dy)
    bad = ~((got - ref).abs() <= bound)
    assert not bool(bad.any()), (int(bad.sum()), float(((got - ref).abs() / bound.clamp_min(1e-300)).max()))


def test_bad_arguments_are_refused_before_any_launch():
    """H*W = 1, C = 12, a pointer off by 8 bytes, a bad dtype: GS_EINVAL (-1) from all three entry points, outputs untouched"""
    from semantic_segmentation_amd import _lib
    lib = _lib.load()
    dev = "cuda"
    big = torch.zeros(4 * 4 * 4 * 16 + 8, dtype=torch.float16, device=dev)
    mi = torch.full((2, 4, 16), 7.0, dtype=torch.float32, device=dev)
    out = torch.full((4 * 4 * 4 * 16 + 8,), 3.0, dtype=torch.float16, device=dev)
    gm = torch.full((2, 4, 16), 5.0, dtype=torch.float32, device=dev)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    cases = {"plane_of_one": (0, 4, 1, 1, 16, 0), "c12": (0, 4, 2, 2, 12, 0), "off_by_8_bytes": (8, 4, 4, 4, 16, 0),
             "bad_dtype": (0, 4, 4, 4, 16, 7)}
    for what, (off, N, H, W, C, dtype) in cases.items():
        rcs = (lib.gs_in_stats(P(big, off), 1e-5, P(mi), P(mi[1]), None, N, H, W, C, dtype, None),
               lib.gs_in_act_apply(P(big, off), P(mi), P(mi[1]), 1, P(out), C, 0, None, 1.0, None, 0, 0, 0, N, H, W, C, dtype, None),
               lib.gs_in_act_bwd(P(big, off), P(mi), P(mi[1]), P(big), C, 0, 1, None, 1.0, None, 0, P(out), P(gm), None, N, H, W, C,
                                 dtype, None))
        assert rcs == (-1, -1, -1), (what, rcs, lib.gs_last_error())
    # a misaligned OUTPUT is refused too
    assert lib.gs_in_act_apply(P(big), P(mi), P(mi[1]), 1, P(out, 8), 16, 0, None, 1.0, None, 0, 0, 0, 4, 4, 4, 16, 0, None) == -1
    torch.cuda.synchronize()
    assert bool((mi == 7.0).all()) and bool((out == 3.0).all()) and bool((gm == 5.0).all())
