"""gs_upsample2x_bilinear_fwd / _fwd_pair / _bwd and gs_affine_warp (csrc/resample.hip) against the fp64 statements of
tests/resample_reference.py, per element, within the bounds counted there from each kernel's own formula (6 fp32 roundings for the
nested interpolation, 6 + T - 1 for an accumulator of T backward terms, 4 on a warp coordinate; then the 16-bit store or the pair's
lo rounding).  The reference holds the same fp32-coordinate weights as the kernels, so nothing is allowed for them.

Every case runs through the C ABI itself with its buffer layout: the low-resolution tensor dense or at channel 8 of a stride C + 24,
the high-resolution one at channel C of 2C or at 16 of C + 40, inside a padded PH x PW buffer.  Everything a kernel must not write
holds a sentinel bit pattern and is compared as integers; the backward's dy carries large finite values around the patch, and dx is
bit-equal between two such fills.  Planted cases put a single 1 at the corners, the last row / column and the middle (per channel
group), so that a wrong clamp, a shifted pad or a short candidate window is a per-element miss.  tests/test_resample_reference_cpu.py
proves the cases: a right implementation passes, the stated wrong ones fail.  Each test takes well under a second, the grid-stride
ones (more than 8192 x 256 work items, reference in fp64 on the device) a few."""
import time

import pytest
import torch

from tests import resample_reference as rr

pytestmark = pytest.mark.gpu

CASES = {c[0]: c for c in rr.UP_CASES}
PAIRS = {c[0]: c for c in rr.PAIR_CASES}
DTS = rr.DTYPES


def _call(name, *args):
    from semantic_segmentation_amd import _lib, ops
    _lib.call(name, *args, ops._stream())


def P(t):
    return None if t is None else t.data_ptr()


def code(dt):
    return 0 if dt == torch.float16 else 1


def run_fwd(xbuf, ybuf, geo, dt):
    _call("gs_upsample2x_bilinear_fwd", P(xbuf), P(ybuf), geo["N"], geo["h"], geo["w"], geo["C"], geo["xs"], geo["xc"], geo["PH"],
          geo["PW"], geo["ys"], geo["yc"], geo["ooy"], geo["oox"], code(dt))


def run_pair(xhi, xlo, yhi, ylo, geo, dt):
    _call("gs_upsample2x_bilinear_fwd_pair", P(xhi), P(xlo), P(yhi), P(ylo), geo["N"], geo["h"], geo["w"], geo["C"], geo["xs"],
          geo["xc"], geo["PH"], geo["PW"], geo["ys"], geo["yc"], geo["ooy"], geo["oox"], code(dt))


def run_bwd(dybuf, dxbuf, geo, dt):
    _call("gs_upsample2x_bilinear_bwd", P(dybuf), P(dxbuf), geo["N"], geo["h"], geo["w"], geo["C"], geo["ys"], geo["yc"], geo["PH"],
          geo["PW"], geo["xs"], geo["xc"], geo["ooy"], geo["oox"], code(dt))


# ------------------------------------------------------------------------------------------------ bilinear forward / backward
@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("name", rr.UP_IDS)
def test_bilinear_forward_and_backward(name, dtn, dt):
    case = CASES[name]
    geo = rr.case_geometry(case)
    x, g = rr.up_case_data(case, dt)
    xbuf = rr.lo_buffer(x, dt, geo).cuda()
    ybuf = rr.hi_buffer(None, dt, geo).cuda()
    run_fwd(xbuf, ybuf, geo, dt)
    torch.cuda.synchronize()
    assert torch.equal(rr.bits(xbuf.cpu()), rr.bits(rr.lo_buffer(x, dt, geo))), "the input is only read"
    y = ybuf.cpu()
    n, r, kept = rr.hold_up_fwd(y, x, geo, dt)
    print(f"fwd {name} {dtn}: worst {r:.3f} of the bound")
    assert n == 0 and kept, (n, r, kept)
    if geo["h"] == 1 and geo["w"] == 1:                                    # r = 0 on both axes: an exact copy
        assert torch.equal(rr.bits(rr.patch(y, geo)), rr.bits(x.to(dt).expand(-1, 2, 2, -1).contiguous()))

    dxs = []
    for fill in rr.BWD_FILLS:
        dybuf = rr.hi_buffer(g, dt, geo, fill=fill).cuda()
        dxbuf = rr.sentinel((geo["N"], geo["h"], geo["w"], geo["xs"]), dt, "cuda")
        run_bwd(dybuf, dxbuf, geo, dt)
        torch.cuda.synchronize()
        dxs.append(dxbuf.cpu())
    assert torch.equal(rr.bits(dxs[0]), rr.bits(dxs[1])), "dx depends on the pad border or on the other channels of dy"
    n, r, kept = rr.hold_up_bwd(dxs[0], g, geo, dt)
    print(f"bwd {name} {dtn}: worst {r:.3f} of the bound")
    assert n == 0 and kept, (n, r, kept)

    if name in rr.RANDOM_UP_IDS:                                           # adjointness from the kernels' own outputs
        Wy, Wx = rr.case_weights(geo["h"], geo["w"])
        d, b = rr.adjointness(x, rr.patch(y, geo), g, rr.lo_slice(dxs[0], geo), Wy, Wx)
        print(f"adjoint {name} {dtn}: |<fwd x, g> - <x, bwd g>| = {d:.3e}, bound {b:.3e}")
        assert d <= b, (d, b)


def _device_hold(got, ref_fn, bound_fn, data, Wy, Wx, dt):
    """per sample, in fp64 on the device: (misses, worst ratio) of the whole tensor"""
    n, r = 0, 0.0
    for i in range(data.shape[0]):
        v = data[i:i + 1].double()
        ref = ref_fn(v, Wy, Wx)
        ni, ri = rr.worst(got[i:i + 1], ref, rr.store16_bound(ref, bound_fn(v, Wy, Wx), dt))
        n, r = n + ni, max(r, ri)
    return n, r


@pytest.mark.parametrize("dtn,dt", DTS)
def test_bilinear_forward_grid_stride(dtn, dt):
    N, h, w, C = rr.GRID_FWD
    geo = rr.geometry(N, h, w, C, (0, 0), "dense", "dense")
    x = torch.randint(-8, 9, (N, h, w, C), generator=torch.Generator().manual_seed(21)).to(dt).cuda()
    y = rr.sentinel((N, 2 * h, 2 * w, C), dt, "cuda")
    run_fwd(x, y, geo, dt)
    torch.cuda.synchronize()
    Wy, Wx = (t.cuda() for t in rr.case_weights(h, w))
    n, r = _device_hold(y, rr.up_fwd64, rr.up_fwd_bound32, x, Wy, Wx, dt)
    print(f"fwd grid-stride {dtn}: worst {r:.3f} of the bound")
    assert n == 0, (n, r)


@pytest.mark.parametrize("dtn,dt", DTS)
def test_bilinear_backward_grid_stride(dtn, dt):
    N, h, w, C = rr.GRID_BWD
    geo = rr.geometry(N, h, w, C, (0, 0), "dense", "dense")
    t0 = time.perf_counter()
    g = torch.randint(-8, 9, (N, 2 * h, 2 * w, C), device="cuda", generator=torch.Generator("cuda").manual_seed(22)).to(dt)
    dx = rr.sentinel((N, h, w, C), dt, "cuda")
    run_bwd(g, dx, geo, dt)
    torch.cuda.synchronize()
    Wy, Wx = (t.cuda() for t in rr.case_weights(h, w))
    n, r = _device_hold(dx, rr.up_bwd64, rr.up_bwd_bound32, g, Wy, Wx, dt)
    print(f"bwd grid-stride {dtn}: worst {r:.3f} of the bound, {time.perf_counter() - t0:.2f} s")
    assert n == 0, (n, r)


# ------------------------------------------------------------------------------------------------ the pair form
@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_bilinear_pair_forward(name, dtn, dt):
    case = PAIRS[name]
    geo = rr.geometry(*case[1:8])
    hi, lo = rr.pair_case_data(case, dt)
    val = hi.double() + lo.double()
    xhi, xlo = rr.lo_buffer(hi, dt, geo).cuda(), rr.lo_buffer(lo, dt, geo).cuda()
    yhi, ylo = rr.hi_buffer(None, dt, geo).cuda(), rr.hi_buffer(None, dt, geo).cuda()
    run_pair(xhi, xlo, yhi, ylo, geo, dt)
    yhi2, ylo2 = rr.hi_buffer(None, dt, geo).cuda(), rr.hi_buffer(None, dt, geo).cuda()
    run_pair(xhi, xlo, yhi2, None, geo, dt)                                # no consumer of the lo plane
    torch.cuda.synchronize()
    n, r, nh, rh, kept = rr.hold_up_pair(yhi.cpu(), ylo.cpu(), val, geo, dt)
    print(f"pair {name} {dtn}: hi + lo worst {r:.3f} of the bound, hi alone {rh:.3f}")
    assert n == 0 and nh == 0 and kept, (n, r, nh, rh, kept)
    assert float(rr.patch(ylo.cpu(), geo).float().abs().max()) > 0
    assert torch.equal(rr.bits(yhi2), rr.bits(yhi)), "the hi plane depends on whether the lo plane is stored"
    assert bool((rr.bits(ylo2) == rr.SENTINEL).all())


@pytest.mark.parametrize("dtn,dt", DTS)
def test_bilinear_pair_forward_grid_stride(dtn, dt):
    N, h, w, C = rr.GRID_FWD
    geo = rr.geometry(N, h, w, C, (0, 0), "dense", "dense")
    v = torch.randn(N, h, w, C, device="cuda", generator=torch.Generator("cuda").manual_seed(23)) * 1.5
    hi, lo = rr.split(v, dt)
    yhi, ylo = rr.sentinel((N, 2 * h, 2 * w, C), dt, "cuda"), rr.sentinel((N, 2 * h, 2 * w, C), dt, "cuda")
    run_pair(hi, lo, yhi, ylo, geo, dt)
    torch.cuda.synchronize()
    Wy, Wx = (t.cuda() for t in rr.case_weights(h, w))
    n = nh = 0
    r = rh = 0.0
    for i in range(N):
        val = hi[i:i + 1].double() + lo[i:i + 1].double()
        ref, b32 = rr.up_fwd64(val, Wy, Wx), rr.up_fwd_bound32(val, Wy, Wx)
        ni, ri = rr.worst(yhi[i:i + 1].double() + ylo[i:i + 1].double(), ref, rr.pair_bound(ylo[i:i + 1], b32, dt))
        nhi, rhi = rr.worst(yhi[i:i + 1], ref, rr.store16_bound(ref, b32, dt))
        n, r, nh, rh = n + ni, max(r, ri), nh + nhi, max(rh, rhi)
    print(f"pair grid-stride {dtn}: hi + lo worst {r:.3f} of the bound, hi alone {rh:.3f}")
    assert n == 0 and nh == 0, (n, r, nh, rh)


# ------------------------------------------------------------------------------------------------ the warp
def warp(src, mats, thresh=-1.0):
    from semantic_segmentation_amd.augment import affine_warp
    out = affine_warp(src.cuda(), mats.cuda(), thresh)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("name", sorted(rr.exact_warp_cases()))
def test_warp_exact(name):
    N, C, H, W, mats = rr.exact_warp_cases()[name]
    src, m = rr.warp_case_data(name, N, C, H, W), torch.tensor(mats, dtype=torch.float32)
    got = warp(src, m)
    assert torch.equal(got, rr.warp64(src.double(), m).float()), int((got.double() != rr.warp64(src.double(), m)).sum())


def test_warp_exact_grid_stride():
    N, C, H, W, mats = rr.GRID_WARP
    src, m = rr.warp_case_data("grid", N, C, H, W), torch.tensor(mats, dtype=torch.float32)
    got = warp(src, m)
    assert torch.equal(got, rr.warp64(src.double(), m).float())


@pytest.mark.parametrize("name,thresh", rr.THRESH_CASES, ids=[f"{n}_{t}" for n, t in rr.THRESH_CASES])
def test_warp_threshold_is_strict_and_border_taps_are_zero(name, thresh):
    N, C, H, W, mats = rr.exact_warp_cases()[name]
    src, m = rr.warp_case_data(name, N, C, H, W, hi=1), torch.tensor(mats, dtype=torch.float32)
    got = warp(src, m, thresh)
    ref = rr.warp64(src.double(), m, thresh)
    assert set(got.unique().tolist()) <= {0.0, 1.0}, "thresh >= 0 binarises, 0.0 included"
    assert torch.equal(got.double(), ref), int((got.double() != ref).sum())


@pytest.fixture(scope="module")
def general():
    return rr.general_warp_cases()


@pytest.mark.parametrize("name", [f"{k}_{d}" for k in [f"seed{s}" for s in rr.GENERAL_SEEDS] + ["hand"] for d in ("random", "mask")])
def test_warp_general(general, name):
    src, mats = general[name]
    s64 = src.double()
    n, r = rr.hold_warp_raw(warp(src, mats), s64, mats)
    print(f"warp {name}: raw worst {r:.3f} of the bound")
    assert n == 0, (n, r)
    bad, share = rr.hold_warp_binary(warp(src, mats, 0.1), s64, mats, 0.1)
    print(f"warp {name}: {share:.5f} of the pixels within their bound of the threshold")
    assert bad == 0 and share <= rr.ADJACENT_CAP, (bad, share)


def test_mask_augmenter_is_its_matrices_through_the_kernel(general):
    from semantic_segmentation_amd.augment import MaskAugmenter
    mask = general["hand_mask"][0]
    for seed in rr.GENERAL_SEEDS:
        mats = torch.from_numpy(MaskAugmenter(seed=seed).matrices(*mask.shape[:1], *mask.shape[2:]))
        got = MaskAugmenter(seed=seed)(mask.cuda()).cpu()
        assert torch.equal(got, warp(mask, mats, 0.1))
