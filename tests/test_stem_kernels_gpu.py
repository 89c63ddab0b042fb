"""The one-channel stem's fused forward and backward (csrc/direct.hip) on the GPU (`-m gpu`) against the fp64 statements of
tests/stem_reference.py, element by element at ZERO tolerance, in fp16 and bf16: gs_stem_fwd_bn, gs_stem_fwd_bn_pair (the rows256
staging, the lane-by-lane stores and write_lo=False), gs_stem_bwd_onepass (dense and strided), gs_stem_bwd_finalize (train and
eval statistics, accumulation into dw, both gradient scales), the stored-y fallback gs_stem_bn_bwd_wgrad, and the refusal of both
backward kernels one pixel past the widest image strip that fits 64 KiB of LDS.

The shapes (stem_reference.STEM_SHAPES) are the smallest that reach 1 x 1 to 3 x 3 images, one / a ragged / eight / seven forward
tiles, blocks that straddle rows and image seams, 141 and 196 pixels per backward block (a second loop iteration, all four
unroll slots, a clamped tail) and the 64 KiB strip.  tests/test_stem_reference_cpu.py proves that every case is exact in fp32 in
any order and that each of eight stated mutants is told from the reference.  The finalize's two 8-deep reduction loops need more
than 112 forward tiles, more than an image of this list has: they run on synthetic integer partials (FINALIZE_SYNTHETIC).

The ONE allowance: gs_stem_bwd_finalize with train statistics on a pixel count that is no power of two.  There c1 = s1 / count and
c2 = s2 / count are no binary numbers, and dW is bounded by one fp32 rounding of the result plus the kernel's fp64 roundings,
counted from its formula (stem_reference.STEM_FINALIZE_ROUNDINGS); the expected value itself is exact (rational arithmetic).
On counts that are a power of two, with eval statistics, and for dgamma / dbeta, the tolerance is zero.

Outputs and workspaces are NaN-filled and sit between guard words that are checked when each test ends."""
import collections
from fractions import Fraction

import pytest
import torch

from tests import exact_reference as E
from tests import stem_reference as S
from tests.exact_reference import DTS, assert_exact, channels_last

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 3.0
GUARD = 4096
GUARD_VALUE = -512.0
_GUARDED = []
_CACHE = collections.OrderedDict()


def dev():
    return torch.device("cuda:0")


def guarded(shape, dtype, fill) -> torch.Tensor:
    n = 1
    for v in shape:
        n *= int(v)
    flat = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=dtype, device=dev())
    body = flat[GUARD:GUARD + n]
    body.fill_(fill)
    _GUARDED.append((flat, n))
    return body.view(*[int(v) for v in shape])


def nan32(*shape):
    return guarded(shape, torch.float32, NAN)


@pytest.fixture(autouse=True)
def check_guards():
    _GUARDED.clear()
    yield
    torch.cuda.synchronize()
    for flat, n in _GUARDED:
        ok = bool((flat[:GUARD] == GUARD_VALUE).all()) and bool((flat[GUARD + n:] == GUARD_VALUE).all())
        assert ok, f"a launch wrote outside a buffer of {n} {flat.dtype} elements (guard words overwritten)"
    _GUARDED.clear()


@pytest.fixture(scope="module", autouse=True)
def leave_the_process_as_found():
    yield
    _CACHE.clear()
    _GUARDED.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def cached(case):
    """operands and fp64 references of a case, built once per session for every test and both dtypes (the two large shapes take a
    second each on the CPU)"""
    if case not in _CACHE:
        c = S.stem_build(case)
        refs = {dtn: S.stem_reference(c, dt) for dtn, dt in DTS}
        common = {k: refs["f16"][k] for k in ("z", "g", "X", "s1", "A")}
        _CACHE[case] = {"c": c, "common": common, "refs": {dtn: {"hi": r["hi"], "lo": r["lo"]} for dtn, r in refs.items()}}
    return _CACHE[case]


def vec(t):
    return t.float().contiguous().to(dev())


def operands(c):
    return c["x"].to(dev()), c["w"].to(dev()), vec(c["scale"]), vec(c["shift"])


def dz_buffer(c, dt):
    """the gradient, channels-last, in the layout of the case: dense, or channels [64, 128) of a 128-wide buffer with NaN outside"""
    stride, coff = S.dz_layout(c["case"])
    cl = channels_last(c["dz"])
    buf = torch.full(tuple(cl.shape[:-1]) + (stride,), NAN, dtype=dt, device=dev())
    buf[..., coff:coff + 64] = cl.to(dt).to(dev())
    return buf, stride, coff


def forward_pair(ops, c, dt):
    N, _, H, W = c["x"].shape
    zpair = guarded((N, H, W, 128), dt, NAN)
    x, w, sc, sh = operands(c)
    ops.stem_fwd_bn_pair(x, w, sc, sh, S.ACTS[c["act"]], zpair)
    return zpair


CASES = pytest.mark.parametrize("case", S.STEM_CASES, ids=S.case_id)
BOTH = pytest.mark.parametrize("dtn,dt", DTS)


@BOTH
@CASES
def test_stem_fwd_bn_exact(case, dtn, dt):
    """z == round16(act(conv(x, w) * scale + shift)), every element of a NaN-filled output"""
    from semantic_segmentation_amd import ops
    r = cached(case)
    c = r["c"]
    N, _, H, W = c["x"].shape
    z = guarded((N, H, W, 64), dt, NAN)
    x, w, sc, sh = operands(c)
    ops.stem_fwd_bn(x, w, sc, sh, S.ACTS[c["act"]], z)
    torch.cuda.synchronize()
    assert_exact(z, r["refs"][dtn]["hi"], f"stem_fwd_bn {S.case_id(case)} {dtn} z [n][y][x][c]")


@BOTH
@CASES
def test_stem_fwd_bn_pair_exact_on_its_three_store_paths(case, dtn, dt, monkeypatch):
    """hi is the single-output form bit for bit, lo == round16(z - hi), hi + lo == z in fp64; the same bits through the rows256
    staging and through the lane-by-lane stores; write_lo=False writes hi and leaves the lo plane alone"""
    from semantic_segmentation_amd import ops
    r = cached(case)
    c, ref = r["c"], r["refs"][dtn]
    N, _, H, W = c["x"].shape
    what = f"stem_fwd_bn_pair {S.case_id(case)} {dtn}"
    x, w, sc, sh = operands(c)
    act = S.ACTS[c["act"]]
    monkeypatch.delenv("GSSEG_STEM_ROWS256_OFF", raising=False)
    zpair = forward_pair(ops, c, dt)
    z = guarded((N, H, W, 64), dt, NAN)
    ops.stem_fwd_bn(x, w, sc, sh, act, z)
    torch.cuda.synchronize()
    assert_exact(zpair[..., :64], ref["hi"], what + " hi (rows256)")
    assert_exact(zpair[..., 64:], ref["lo"], what + " lo (rows256)")
    assert torch.equal(zpair[..., :64], z), what + ": hi is not what gs_stem_fwd_bn stores"
    total = zpair[..., :64].double().cpu() + zpair[..., 64:].double().cpu()
    assert_exact(total, r["common"]["z"], what + " hi + lo in fp64")
    monkeypatch.setenv("GSSEG_STEM_ROWS256_OFF", "1")
    zlanes = forward_pair(ops, c, dt)
    torch.cuda.synchronize()
    monkeypatch.delenv("GSSEG_STEM_ROWS256_OFF")
    assert_exact(zlanes, zpair, what + " lane-by-lane stores against rows256")
    assert torch.equal(zlanes, zpair)
    zhi = guarded((N, H, W, 128), dt, SENTINEL)
    zhi[..., :64] = NAN
    ops.stem_fwd_bn_pair(x, w, sc, sh, act, zhi, write_lo=False)
    torch.cuda.synchronize()
    assert_exact(zhi[..., :64], ref["hi"], what + " hi (write_lo=False)")
    assert bool((zhi[..., 64:] == SENTINEL).all()), what + ": write_lo=False wrote into the lo plane"


def run_onepass(ops, c, dt, zpair, x=None):
    """gs_stem_bwd_onepass on the dense z and gs_stem_bwd_onepass_strided on the hi plane of zpair: (nt, s1 partials, slabs) of
    the strided launch, after asserting that both wrote the same bits"""
    from semantic_segmentation_amd import _lib
    N, _, H, W = c["x"].shape
    x = c["x"].to(dev()) if x is None else x
    dz, stride, coff = dz_buffer(c, dt)
    nt = ops.stem_bwd_tiles(N, H, W)
    assert nt == S.stem_bwd_blocks(N * H * W), "gs_stem_bwd_tiles is not the host formula the case list was derived from"
    act = S.ACTS[c["act"]]
    s1p, ws = nan32(nt * 64), nan32(nt * 576)
    assert ops.stem_bwd_onepass(x, zpair, dz, stride, coff, act, s1p, ws, z_stride=128)
    zd = zpair[..., :64].contiguous()
    s1d, wsd = nan32(nt * 64), nan32(nt * 576)
    _lib.call("gs_stem_bwd_onepass", x.data_ptr(), zd.data_ptr(), dz.data_ptr(), stride, coff, act, s1d.data_ptr(), wsd.data_ptr(),
              N, H, W, ops.dt_code(zd), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(s1d, s1p) and torch.equal(wsd, ws), "the dense and the strided launch differ"
    return nt, s1p, ws


def pair_of(r, dtn, dt):
    """the [hi | lo] buffer of the reference (test_stem_fwd_bn_pair_exact_on_its_three_store_paths holds the kernel to it)"""
    return torch.cat([r["refs"][dtn]["hi"], r["refs"][dtn]["lo"]], -1).to(dev())


@BOTH
@CASES
def test_stem_bwd_onepass_exact(case, dtn, dt):
    """summed over the blocks in fp64, s1 == sum g and A[c][t] == sum_p g x_t(p) with g = dz * act'(sign of the stored z); z is the hi
    plane of the pair buffer the forward kernel wrote"""
    from semantic_segmentation_amd import ops
    r = cached(case)
    c = r["c"]
    what = f"stem_bwd_onepass {S.case_id(case)} {dtn}"
    zpair = forward_pair(ops, c, dt)
    torch.cuda.synchronize()
    assert_exact(zpair[..., :64], r["refs"][dtn]["hi"], what + " z")
    nt, s1p, ws = run_onepass(ops, c, dt, zpair)
    assert_exact(s1p.view(nt, 64).double().sum(0).cpu(), r["common"]["s1"], what + f" s1 [c] over {nt} blocks")
    assert_exact(ws.view(nt, 64, 9).double().sum(0).cpu(), r["common"]["A"], what + f" A [c][t] over {nt} blocks")


@BOTH
def test_comparer_sees_an_image_rolled_by_one_pixel_on_the_gpu(dtn, dt):
    """negative control: the same launch on the image rolled by one pixel gives exactly the A of the rolled image, and the comparer
    finds it different from the A of the case"""
    from semantic_segmentation_amd import ops
    case = ((3, 45, 53), "relu", "T")
    r = cached(case)
    c = r["c"]
    rolled = c["x"].reshape(-1).roll(1).view_as(c["x"]).contiguous()
    nt, s1p, ws = run_onepass(ops, c, dt, pair_of(r, dtn, dt), x=rolled.to(dev()))
    got = ws.view(nt, 64, 9).double().sum(0).cpu()
    assert_exact(got, r["common"]["g"].t() @ S.stem_taps(rolled), f"one-pass A of the rolled image {dtn}")
    assert_exact(s1p.view(nt, 64).double().sum(0).cpu(), r["common"]["s1"], "s1 does not read the image")
    n = E.mismatches(got, r["common"]["A"]).shape[0]
    assert n > 0, "the comparer missed an image rolled by one pixel"
    with pytest.raises(AssertionError, match="elements differ"):
        assert_exact(got, r["common"]["A"], "rolled")
    print(f"rolled image {dtn}: {n} of {got.numel()} entries of A differ")


def f32_of(fractions, shape):
    """float32(exact): float(Fraction) is the correctly rounded fp64 value -- the exact one wherever the CPU test proved fewer than
    53 bits -- and .float() rounds once"""
    return torch.tensor([float(v) for v in fractions], dtype=torch.float64).float().view(*shape)


@BOTH
@CASES
def test_stem_bwd_finalize_against_the_definition(case, dtn, dt):
    """dW, dgamma, dbeta of gs_stem_bwd_finalize, fed by gs_stem_stats and gs_stem_bwd_onepass, against the pixel-by-pixel
    definition in exact rational arithmetic.  Train statistics with the case's gradient scale: zero tolerance where the pixel count is a
    power of two, stem_reference.finalize_bound elsewhere (derived, see the module docstring).  dgamma / dbeta start from NaN and are
    overwritten; dw is accumulated: from an integer start, two calls give (start + dW) + dW in fp32.  Eval statistics with the other
    gradient scale and no tap sums: dW == float32(gscale * scale * A)."""
    from semantic_segmentation_amd import ops
    r = cached(case)
    c = r["c"]
    N, _, H, W = c["x"].shape
    what = f"stem_bwd_finalize {S.case_id(case)} {dtn}"
    x, w, sc, _ = operands(c)
    mean, invstd = vec(c["mean"]), vec(c["invstd"])
    mt = ops.conv_smallcin_mtiles(N, H, W)
    assert mt == S.stem_fwd_tiles(N * H * W)
    part, taps = nan32(ops.bn_partials_numel(mt, 64)), nan32(mt * 54)
    ops.stem_stats(x, w, part, taps)
    nt, s1p, ws = run_onepass(ops, c, dt, pair_of(r, dtn, dt))
    ref = {"g": r["common"]["g"], "X": r["common"]["X"], "s1": r["common"]["s1"], "A": r["common"]["A"]}
    sums = S.stem_pixel_sums(c, ref)
    gs = c["gscale"]
    want = S.stem_finalize_definition(c, sums, True, gs)
    dw, dgamma, dbeta = guarded((64, 1, 3, 3), torch.float32, 0.0), nan32(64), nan32(64)
    ops.stem_bwd_finalize(ws, s1p, taps, w, sc, mean, invstd, True, gs, dw, dgamma, dbeta, N, H, W)
    torch.cuda.synchronize()
    assert_exact(dgamma, f32_of(want["dgamma"], (64,)), what + " dgamma")
    assert_exact(dbeta, f32_of(want["dbeta"], (64,)), what + " dbeta")
    assert_dw(dw, want, S.pow2_count(case[0]), what)
    start = ((torch.arange(576) % 7) - 3).float()
    start[start == 0] = 5.0
    acc = guarded((64, 1, 3, 3), torch.float32, 0.0)
    acc.copy_(start.view(64, 1, 3, 3))
    for _ in range(2):
        g2, b2 = nan32(64), nan32(64)
        ops.stem_bwd_finalize(ws, s1p, taps, w, sc, mean, invstd, True, gs, acc, g2, b2, N, H, W)
    torch.cuda.synchronize()
    assert_exact(acc, (start.view(64, 1, 3, 3).to(dev()) + dw) + dw, what + " dw is accumulated: (start + dW) + dW")
    assert torch.equal(g2, dgamma) and torch.equal(b2, dbeta)
    # eval statistics: c1 = c2 = 0, the tap sums are not read
    gs2 = 1.5 - gs
    want = S.stem_finalize_definition(c, sums, False, gs2)
    dwe, dge, dbe = guarded((64, 1, 3, 3), torch.float32, 0.0), nan32(64), nan32(64)
    ops.stem_bwd_finalize(ws, s1p, None, w, sc, mean, invstd, False, gs2, dwe, dge, dbe, N, H, W)
    torch.cuda.synchronize()
    assert_exact(dwe, f32_of(want["dW"], (64, 1, 3, 3)), what + " eval dW")
    assert_exact(dge, f32_of(want["dgamma"], (64,)), what + " eval dgamma")
    assert_exact(dbe, f32_of(want["dbeta"], (64,)), what + " eval dbeta")


def assert_dw(dw, want, exact: bool, what):
    """dW against its exact rational value: float32(exact) where `exact`, else within stem_reference.finalize_bound"""
    if exact:
        return assert_exact(dw, f32_of(want["dW"], (64, 1, 3, 3)), what + " dW [c][0][ky][kx] (count a power of two)")
    bad = []
    for i, (gv, ev, mg) in enumerate(zip(dw.double().cpu().view(-1).tolist(), want["dW"], want["mag"])):
        if not (gv == gv and abs(Fraction(gv) - ev) <= S.finalize_bound(ev, mg)):
            bad.append(f"    (c {i // 9}, tap {i % 9}): got {gv!r} exact {float(ev)!r} bound {float(S.finalize_bound(ev, mg)):.3e}")
    assert not bad, f"{what}: {len(bad)} of 576 dW entries outside their bound\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("shape", S.FINALIZE_SYNTHETIC, ids=lambda s: "x".join(map(str, s)))
def test_stem_bwd_finalize_unrolled_reduction_loops(shape):
    """gs_stem_bwd_finalize alone on synthetic integer partials of more than 112 forward tiles and 512 backward blocks: both 8-deep
    unrolled loops run, with a tail on some lanes at 140 tiles; zero tolerance at 2^17 pixels, the derived bound at 140 * 1024"""
    from semantic_segmentation_amd import ops
    r = S.finalize_synthetic_build(shape)
    N, H, W = shape
    assert (ops.stem_bwd_tiles(N, H, W), ops.conv_smallcin_mtiles(N, H, W)) == (r["nb"], r["nsg"])
    what = "stem_bwd_finalize synthetic " + "x".join(map(str, shape))
    want = S.finalize_closed_from_sums(r, r["S"], r["packed"], r["s1"], r["A"], r["count"], True, 0.5)
    ws, s1p, taps = nan32(r["nb"] * 576), nan32(r["nb"] * 64), nan32(r["nsg"] * 54)
    ws.copy_(r["ws"].view(-1)), s1p.copy_(r["s1p"].view(-1)), taps.copy_(r["taps"].view(-1))
    dw, dgamma, dbeta = guarded((64, 1, 3, 3), torch.float32, 0.0), nan32(64), nan32(64)
    ops.stem_bwd_finalize(ws, s1p, taps, r["w"].to(dev()), vec(r["scale"]), vec(r["mean"]), vec(r["invstd"]), True, 0.5, dw, dgamma, dbeta, N, H, W)
    torch.cuda.synchronize()
    assert_exact(dgamma, f32_of(want["dgamma"], (64,)), what + " dgamma")
    assert_exact(dbeta, f32_of(want["dbeta"], (64,)), what + " dbeta")
    assert_dw(dw, want, S.pow2_count(shape), what)


@BOTH
@CASES
def test_stem_bn_bwd_wgrad_exact(case, dtn, dt):
    """the stored-y fallback: dw == float32(gscale * sum_p dy x_t) with dy as exact_reference.bn_reference states it, on a stored y
    of its own, dz in the layout of the case; dw is accumulated"""
    from semantic_segmentation_amd import ops
    c = S.wgrad_build(case)
    want = S.wgrad_reference(c)["dw"].to(dev())
    what = f"stem_bn_bwd_wgrad {S.case_id(case)} {dtn}"
    y = channels_last(c["y"]).to(dt).to(dev())
    assert torch.equal(y.float().cpu(), channels_last(c["y"])), "the stored y is not exact in the dtype"
    dz, stride, coff = dz_buffer(c, dt)
    co = [vec(c[k]) for k in ("scale", "shift", "mean", "invstd", "c1", "c2")]
    x = c["x"].to(dev())
    dw = guarded((64, 1, 3, 3), torch.float32, 0.0)
    assert ops.stem_bn_bwd_wgrad(y, dz, stride, coff, x, *co, S.ACTS[c["act"]], dw, c["gscale"])
    torch.cuda.synchronize()
    assert_exact(dw, want, what + " dw [c][0][ky][kx]")
    start = (((torch.arange(576) % 5) - 2).float() * 2 + 1).view(64, 1, 3, 3).to(dev())
    acc = guarded((64, 1, 3, 3), torch.float32, 0.0)
    acc.copy_(start)
    for _ in range(2):
        assert ops.stem_bn_bwd_wgrad(y, dz, stride, coff, x, *co, S.ACTS[c["act"]], acc, c["gscale"])
    torch.cuda.synchronize()
    assert_exact(acc, (start + want) + want, what + " dw is accumulated")


@BOTH
def test_both_backward_kernels_refuse_one_pixel_past_the_widest_strip(dtn, dt):
    """N = 1, H = 2: the widest image whose strip fits 64 KiB of LDS is in the case list and runs (exactly 64 KiB); its neighbour is
    refused by gs_stem_bwd_onepass and by gs_stem_bn_bwd_wgrad, which leave their poisoned outputs untouched"""
    from semantic_segmentation_amd import ops
    N, H, W = S.STEM_REFUSED
    widest = S.widest_accepted(N, H)
    assert W == widest + 1 and (N, H, widest) in S.STEM_SHAPES and S.stem_lds_bytes(N, H, widest) == S.LDS_LIMIT
    g = E.generator(("stem_refused", dtn))
    x = S.stem_image(g, (N, H, W), "P").to(dev())
    z = torch.ones((N, H, W, 128), dtype=dt, device=dev())
    dz = torch.ones((N, H, W, 64), dtype=dt, device=dev())
    nt = ops.stem_bwd_tiles(N, H, W)
    s1p, ws = nan32(nt * 64), nan32(nt * 576)
    assert ops.stem_bwd_onepass(x, z, dz, 64, 0, S.ACTS["relu"], s1p, ws, z_stride=128) is False
    ones = torch.ones(64, device=dev())
    dw = guarded((64, 1, 3, 3), torch.float32, SENTINEL)
    assert ops.stem_bn_bwd_wgrad(z[..., :64].contiguous(), dz, 64, 0, x, ones, ones, ones, ones, ones, ones, S.ACTS["relu"], dw, 1.0) is False
    torch.cuda.synchronize()
    assert bool(torch.isnan(s1p).all()) and bool(torch.isnan(ws).all()), "a refused gs_stem_bwd_onepass wrote its outputs"
    assert bool((dw == SENTINEL).all()), "a refused gs_stem_bn_bwd_wgrad wrote dw"
