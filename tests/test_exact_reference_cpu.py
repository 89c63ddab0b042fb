"""CPU tests of tests/exact_reference.py: (a) every entry of every case list meets its exactness conditions in both dtypes, so
a GPU run can never fail for a reason of the test's own making (this is also where every T(d) density is proven); (b) the
reference is order independent -- an fp32 evaluation accumulated in permuted K chunks equals fp64 bit for bit; (c) the gap the
exact tests close is demonstrated: local mutations that the norm-wise rel_err of tests/test_gpu_kernels.py lets pass are
each reported by assert_exact."""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_reference as E
from tests.exact_reference import DTS, channels_last, expect16, expect32
from tests.test_gpu_kernels import rel_err, tol


def _id(v):
    return "x".join(_id(i) for i in v) if isinstance(v, tuple) else str(v)


def _representable(t, dt):
    assert torch.equal(t.to(dt).float(), t.float()), f"operand not representable in {dt}"


# ------------------------------------------------------------------------------------------------ (a) conditions
@pytest.mark.parametrize("shape,wgrad", E.CONV3X3_CASES + [(E.GRID_SHAPE, False)], ids=[_id(s) for s, _ in E.CONV3X3_CASES] + ["grid"])
def test_conv3x3_cases_meet_the_conditions(shape, wgrad):
    """S and P: the conditions follow from the value ranges (operands drawn, bounds asserted, nothing evaluated); T(d): the
    per-channel sums of |y| and y^2 of the reference stay below 2^24 at the density the case list chose."""
    N, H, W, Cin, Cout = shape
    for vset, d in E.conv3x3_sets(shape, wgrad):
        g = E.generator((("conv3x3",) + tuple(shape), vset))
        x = E.draw(g, vset, "a", (N, Cin, H, W), d)
        w = E.draw(g, vset, "w", (Cout, Cin, 3, 3), d)
        E.require_integers(x, w)
        for _, dt in DTS:
            _representable(x, dt), _representable(w, dt)
        E.require_products(9 * Cin, x, w)                      # y (+ |bias| <= 8: far below the limit)
        E.require_products(9 * Cout, torch.tensor([8.0 if vset != "T" else 1.0]), w)     # dx
        if E.conv3x3_wgrad_runs(wgrad, vset):                  # dw: dense where the case list says so, under T(d) on every shape
            E.require_products(N * H * W, x, torch.tensor([8.0 if vset != "T" else 1.0]))
        if vset == "T":
            y = F.conv2d(x, w, None, padding=1)                # fp32 == fp64 here: require_products above
            s1, s2 = E.require_channel_sums(y, _id(shape))
            assert float(s2.max()) > 0


def test_densities_are_the_largest_the_rule_allows():
    """density(): doubling d quadruples the expected sum of y^2 -- the chosen d is the largest power of 1/2 under the rule"""
    for shape, _ in E.CONV3X3_CASES:
        N, H, W, Cin, Cout = shape
        d = E.density(N * H * W, 9 * Cin)
        assert N * H * W * 9 * Cin * d * d < E.LIMIT / 2
        assert d == 0.5 or N * H * W * 9 * Cin * (2 * d) ** 2 >= E.LIMIT / 2
    assert E.density(24 * 96 * 128, 9 * 64) == 0.125


def test_value_sets_have_the_stated_ranges_and_exercise_rounding():
    g = E.generator("ranges")
    x, w = E.draw(g, "S", "a", (4, 64, 20, 20)), E.draw(g, "S", "w", (64, 64, 3, 3))
    assert x.min() == -8 and x.max() == 8 and w.min() == -4 and w.max() == 4
    xp, wp = E.draw(g, "P", "a", (4, 64, 20, 20)), E.draw(g, "P", "w", (64, 64, 3, 3))
    assert xp.min() == 0 and xp.max() == 8 and wp.min() == 0 and wp.max() == 4
    t = E.draw(g, "T", "a", (4, 64, 20, 20), 0.125)
    assert set(t.unique().tolist()) == {-1.0, 0.0, 1.0} and 0.10 < float((t != 0).float().mean()) < 0.15
    yp = F.conv2d(xp.double(), wp.double(), None, padding=1)
    inner = yp[:, :, 1:-1, 1:-1]
    # set P rounds in BOTH dtypes (the fp32-ness of the accumulator and the round-to-nearest-even of the store are exercised)
    assert float((inner.half().double() != inner).double().mean()) > 0.5
    assert float((inner.bfloat16().double() != inner).double().mean()) > 0.9
    ys = F.conv2d(x.double(), w.double(), None, padding=1)
    assert float((ys.half().double() != ys).double().mean()) < 0.01 and float((ys.bfloat16().double() != ys).double().mean()) > 0.2


# ------------------------------------------------------------------------------------------------ (b) order independence
@pytest.mark.parametrize("chunk", [16, 32])
def test_reference_is_order_independent(chunk):
    """conv, dgrad and wgrad: fp32 accumulation over permuted K chunks == fp64, bit for bit"""
    N, H, W, Cin, Cout = 2, 37, 41, 64, 72
    c = E.conv_case("order", "S", (N, Cin, H, W), (Cout, Cin, 3, 3), lambda x, w: F.conv2d(x, w, None, padding=1), 9 * Cin, 9 * Cout,
                    N * H * W)
    x, w, dy = c["x"], c["w"], c["dy"]
    assert torch.equal(E.chunked_conv2d_fp32(x, w, 1, chunk, 1).double(), c["y"])
    # dgrad = the convolution of dy with the flipped, transposed weight: K = Cout
    wd = w.flip(2, 3).transpose(0, 1).contiguous()
    assert torch.equal(E.chunked_conv2d_fp32(dy, wd, 1, chunk, 2).double(), c["dx"])
    # wgrad: K = pixels, accumulated image by image and in permuted row chunks
    acc = torch.zeros(Cout, Cin, 3, 3)
    rows = torch.randperm(H, generator=torch.Generator().manual_seed(3))
    xp = F.pad(x, (1, 1, 1, 1))
    for n in (1, 0):
        for r0 in range(0, H, chunk):
            for r in rows[r0:r0 + chunk].tolist():
                for ky in range(3):
                    for kx in range(3):
                        acc[:, :, ky, kx] += dy[n, :, r, :] @ xp[n, :, r + ky, kx:kx + W].t()
    assert torch.equal(acc.double(), c["dw"])
    # and the fp32 evaluation the large cases use equals the fp64 one
    y32, (dx32, dw32) = E.autograd(lambda a, b: F.conv2d(a, b, None, padding=1), (x, w), dy, torch.float32)
    assert torch.equal(y32.double(), c["y"]) and torch.equal(dx32.double(), c["dx"]) and torch.equal(dw32.double(), c["dw"])


# ------------------------------------------------------------------------------------------------ (c) the gap
def _mutations(y):
    """(name, mutated copy of a correct NCHW output): one element zero, one whole pixel zero; the caller adds the lost taps"""
    one_zero = y.clone(); one_zero[0, 5, 3, 4] = 0
    pixel_zero = y.clone(); pixel_zero[0, :, 3, 4] = 0
    return [("one element zero", one_zero), ("one pixel zero", pixel_zero)]


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("shape", [(2, 13, 9, 64, 64), (2, 37, 41, 64, 64), (1, 32, 64, 192, 64)], ids=_id)
def test_comparer_reports_what_the_norm_lets_pass(shape, dtn, dt):
    N, H, W, Cin, Cout = shape
    c = E.conv_case(("gap",) + shape, "S", (N, Cin, H, W), (Cout, Cin, 3, 3), lambda x, w: F.conv2d(x, w, None, padding=1), 9 * Cin)
    x, w, y = c["x"].double(), c["w"].double(), c["y"]
    muts = _mutations(y)
    # one edge pixel (0, H-1, 0) loses its tap (ky, kx) = (0, 1) -- the products x[0, :, H-2, 0] . w[co, :, 0, 1] -- in one output
    # channel (one wave's fragment), and in all of them
    lost = y.clone()
    lost[0, 5, H - 1, 0] -= w[5, :, 0, 1] @ x[0, :, H - 2, 0]
    muts.append(("one edge pixel loses one tap in one channel", lost))
    lost_all = y.clone()
    lost_all[0, :, H - 1, 0] -= w[:, :, 0, 1] @ x[0, :, H - 2, 0]
    muts.append(("one edge pixel loses one tap in every channel", lost_all))
    # every image's corner pixel (0, 0) loses the tap row ky = 1 (the taps (1, 1) and (1, 2) that are inside the image)
    row = y.clone()
    for n in range(N):
        row[n, :, 0, 0] -= w[:, :, 1, 1] @ x[n, :, 0, 0] + w[:, :, 1, 2] @ x[n, :, 0, 1]
    muts.append(("corner pixels lose a tap row", row))
    want = expect16(channels_last(y), dt)
    E.assert_exact(want.clone(), want, "identity")
    for name, m in muts:
        got = expect16(channels_last(m), dt)
        n = E.mismatches(got, want).shape[0]
        assert n > 0, f"{name}: not reported"
        with pytest.raises(AssertionError, match="elements differ"):
            E.assert_exact(got, want, name)
    if shape == (2, 37, 41, 64, 64):
        # the first mutation of the table stays under the norm-wise limit of tests/test_gpu_kernels.py in both dtypes
        got = expect16(channels_last(lost), dt)
        assert rel_err(got.float(), y.permute(0, 2, 3, 1)) < tol(dt)


def test_norm_metric_on_real_inputs_lets_the_lost_tap_pass():
    """The same mutation on real-valued inputs with the shape and seed of test_conv3x3_halo_fwd_dgrad, rounded to the dtype.
    Measured: rounding alone 2.1e-4 (fp16) / 1.7e-3 (bf16) of the norm; the tap lost in one channel 8.4e-4 / 1.8e-3 -- 3.6x and
    8x under the limits; lost in every channel of the pixel 7.5e-3 / 7.7e-3 -- under the bf16 limit, 2.5x over the fp16 one."""
    N, H, W, Cin, Cout = 2, 37, 41, 64, 64
    for _, dt in DTS:
        g = torch.Generator().manual_seed(12)
        x = (torch.randn(N, Cin, H, W, generator=g)).to(dt).float()
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(dt).float()
        ref = F.conv2d(x, w, None, padding=1)
        m = ref.clone()
        m[0, 5, H - 1, 0] -= w[5, :, 0, 1] @ x[0, :, H - 2, 0]
        assert not torch.equal(m.to(dt), ref.to(dt))
        assert rel_err(m.to(dt).float(), ref) < tol(dt) / 3


@pytest.mark.parametrize("shape", [(2, 13, 9, 64, 64), (4, 64, 64, 64, 128)], ids=_id)
def test_comparer_reports_one_dropped_wgrad_contribution(shape):
    """weight gradient: one pixel's contribution to one tap dropped -> a 64 x 64 block of one tap differs, and is reported"""
    N, H, W, Cin, Cout = shape
    c = E.conv_case(("gapw",) + shape, "S", (N, Cin, H, W), (Cout, Cin, 3, 3), lambda x, w: F.conv2d(x, w, None, padding=1), 9 * Cin,
                    None, N * H * W, fast=True)
    dw = c["dw"].double()
    m = dw.clone()
    m[:, :, 2, 0] -= torch.outer(c["dy"][0, :, 1, 2].double(), c["x"][0, :, 2, 1].double())       # pixel (1, 2), tap (2, 0) reads x(2, 1)
    n = E.mismatches(expect32(m), expect32(dw)).shape[0]
    assert n > 0
    print(f"dropped wgrad contribution {shape}: {n} elements differ, rel_err {rel_err(m, dw):.2e}")
    with pytest.raises(AssertionError, match="elements differ"):
        E.assert_exact(expect32(m), expect32(dw), "dropped contribution")


def test_leaky_rule_is_one_ulp_on_negatives_only():
    ref = torch.tensor([-1000.0, -7.0, -5.0, 0.0, 3.0, 1001.0, -3333.0], dtype=torch.float64)
    for _, dt in DTS:
        want = torch.where(ref >= 0, ref.float(), ref.float() * 0.2).to(dt)
        assert bool(E.leaky_ok(want, ref).all())
        up = (want.view(torch.int16) + 1).view(dt)            # one unit in the last place further from zero
        ok = E.leaky_ok(up, ref)
        assert ok.tolist() == [True, True, True, False, False, False, True]
        far = (want.view(torch.int16) + 2).view(dt)
        assert not bool(E.leaky_ok(far, ref).any())
        with pytest.raises(AssertionError, match="elements differ"):
            E.assert_leaky_exact(far, ref, "two ulp")


# ------------------------------------------------------------------------------------------------ (a) conditions, group B
@pytest.mark.parametrize("case", E.IGEMM_FWD_CASES, ids=E.fwd_id)
def test_igemm_forward_cases_meet_the_conditions(case):
    """the builders assert every condition (integers, products, per-channel sums under T(d)): building a case is the proof"""
    for vset, d in sorted(set(E.igemm_fwd_sets(case, "f16") + E.igemm_fwd_sets(case, "bf16")), key=str):
        r = E.igemm_fwd_build(tuple(case.items()), vset, d)
        for _, dt in DTS:
            _representable(r["x"], dt), _representable(r["w"], dt)
        expect32(r["y"])


@pytest.mark.parametrize("case", E.IGEMM_GRAD_CASES, ids=_id)
def test_igemm_gradient_cases_meet_the_conditions(case):
    N, h, w, Cin, Cout, k, s, p, single = case
    M = N * E.out_size(h, k, s, p) * E.out_size(w, k, s, p)
    for vset in ("S", "P"):
        g = E.generator((("igemm_grad",) + tuple(case), vset))
        x, wt = E.draw(g, vset, "a", (N, Cin, h, w)), E.draw(g, vset, "w", (Cout, Cin, k, k))
        E.require_integers(x, wt)
        E.require_products(k * k * Cout, torch.tensor([8.0]), wt)
        E.require_products(M, x, torch.tensor([8.0]))


@pytest.mark.parametrize("case", E.CONVT_CASES, ids=_id)
def test_convT_cases_meet_the_conditions(case):
    for vset, d in sorted(set(E.convt_sets(case, "f16") + E.convt_sets(case, "bf16")), key=str):
        r = E.convt_build(case, vset, d)
        expect32(r["y"]), expect32(r["dw"])


# ------------------------------------------------------------------------------------------------ (a) conditions, groups C and D
@pytest.mark.parametrize("case,grads", [(c, "") for c in E.UPCONV_FWD_CASES] + [(c, "x") for c in E.UPCONV_DGRAD_CASES]
                         + [(c, "w") for c in E.UPCONV_WGRAD_CASES], ids=lambda v: _id(v) if isinstance(v, tuple) else "grad_" + v)
def test_upconv_cases_meet_the_conditions(case, grads):
    """operands drawn and bounds asserted from the value ranges (nothing evaluated: set S and P only)"""
    N, h, w, Cin, Cout, pad = case[:6]
    for vset in ("S", "P"):
        g = E.generator((("upconv",) + tuple(case[:6]), vset))
        x, wt = E.draw(g, vset, "a", (N, Cin, h, w)), E.draw(g, vset, "w", (Cin, Cout, 2, 2))
        E.require_integers(x, wt)
        E.require_products(Cin, x, wt)
        E.require_products(4 * Cout, torch.tensor([8.0]), wt)
        E.require_products(N * h * w, x, torch.tensor([8.0]))


@pytest.mark.parametrize("case", E.CONV3D_CASES, ids=_id)
def test_conv3d_cases_meet_the_conditions(case):
    for vset, d in E.conv3d_sets(case):
        E.conv3d_build(case, vset, d)


@pytest.mark.parametrize("case", E.UPCONV3D_CASES, ids=_id)
def test_upconv3d_cases_meet_the_conditions(case):
    for vset in ("S", "P"):
        E.upconv3d_build(case, vset)


# ------------------------------------------------------------------------------------------------ (a) conditions, group E
@pytest.mark.parametrize("case", E.SMALLCIN_CASES, ids=_id)
def test_smallcin_cases_meet_the_conditions(case):
    for vset, d in E.smallcin_sets(case):
        E.smallcin_build(case, vset, d)


def test_end_of_net_and_reduction_cases_meet_the_conditions():
    """the builders of the remaining lists assert their own conditions; the tie cases really tie"""
    for case in E.SMALLCOUT_CASES:
        for vset in ("S", "P"):
            r = E.smallcout_build(case, vset)
            expect32(r["y"]), expect32(r["db"], 0.5)
    for case in E.STEM_CASES:
        E.stem_build(case)
    for case in E.HEAD_CASES:
        r = E.head_build(case)
        expect32(r["logits"]), expect32(r["dw"], 0.5), expect32(r["db"], 0.5)
    for case in E.BIAS_FROM_DGRAD_CASES:
        r = E.bias_from_dgrad_build(case)
        for _, dt in DTS:
            assert torch.equal(expect16(r["dx"], dt).double(), r["dx"].double())
    for case in E.COLSUM_CASES:
        assert case[0] * case[1] * case[2] * 8 < E.LIMIT
        E.require_pow2(case[-1])
    for case in E.PARTIALS_COLSUM_CASES:
        assert case[0] * 1000 < E.LIMIT
        E.require_pow2(case[-1])
    for case in E.MAXPOOL3D_CASES:
        assert E.maxpool3d_build(case)["ties"] > 0.5
    for case in E.POOL_ROUTE_CASES:
        r = E.pool_route_build(case)
        N, H, W, C = case
        zw = r["y"][:, :, :H // 2 * 2, :W // 2 * 2].unfold(2, 2, 2).unfold(3, 2, 2)
        tied = ((zw == zw.amax((-2, -1), keepdim=True)).sum((-2, -1)) > 1).double().mean()
        assert float(tied) > 0.3
        expect32(r["dy"])


# ------------------------------------------------------------------------------------------------ (a) conditions, group F
def test_pix2pix_pack_cases_meet_the_conditions():
    for ky in range(8):
        for kx in range(8):           # the class / tap rule of include/gsseg.h, as test_upconv8_image_wgrad_matches_autograd states it
            assert E.class_tap_of(ky, kx) == (2 * (1 - ky % 2) + (1 - kx % 2), 4 * (ky // 2) + kx // 2)
    for case in E.MERGE_CASES:
        r = E.merge_build(case)
        assert torch.equal(E.classes_to_merged(E.merged_to_classes(r["wm"])), r["wm"])
        assert torch.equal(r["wm"] * 4, (r["wm"] * 4).round())
        for _, dt in DTS:             # a multiple of 0.25 up to 4: no rounding in either 16-bit pack
            assert torch.equal(expect16(r["wm"], dt).double(), r["wm"])
    for case in E.SPLIT_CASES:
        r = E.split_build(case)
        expect32(r["dots"], 0.5)
    for case in E.IMAGE_FWD_CASES:
        expect32(E.image_fwd_build(case)["y"])
    for case in E.IMAGE_WGRAD_CASES:
        expect32(E.image_wgrad_build(case)["dwm"])


# ------------------------------------------------------------------------------------------------ group G: BatchNorm / activation
_BN_ALL = E.BN_CASES + E.BN_FWD_ONLY_CASES
_HEADS = E.BN_HEAD_CASES + [E.BN_HEAD_TWO_CHUNKS]
_BN_BUILT = {}


def _bn(case):
    """built once per process: the operands are the same for both dtypes, the order-independence test and the mutant test"""
    if case not in _BN_BUILT:
        _BN_BUILT[case] = E.bn_head_build(case) if len(case) == 5 else E.bn_build(*case)
    return _BN_BUILT[case]


def _bn_ident(case):
    return "head-" + _id(case) if len(case) == 5 else E.bn_id(case)


def test_bn_case_lists_hold_what_the_issue_lists():
    plain = {s for s, p, v in E.BN_CASES if not p}
    assert plain == set(E.BN_SHAPES) and len(E.BN_SHAPES) == 8
    for s in E.BN_FULL_SHAPES:
        assert {v for s2, p, v in E.BN_CASES if s2 == s and not p} == set(E.BN_VARIANTS) - {"pool_only"}
    legal = {v for v, d in E.BN_VARIANTS.items() if d["dzb"] is None and not d["keep"]}
    for s in E.BN_POOLED_SHAPES:
        assert {v for s2, p, v in E.BN_CASES if s2 == s and p} == legal
    acts = {(d["act"], d["dzb"]) for d in E.BN_VARIANTS.values()}
    assert {("none", None), ("relu", None), ("leaky", None), ("relu", "none"), ("relu", "leaky")} <= acts
    assert E.BN_POOLED_SHAPES == [(2, 9, 7, 64), (1, 65, 33, 128), (2, 64, 64, 64)] and E.BN_FWD_ONLY_CASES[0][0] == (2, 96, 96, 512)
    assert E.BN_HEAD_CASES == [(2, 18, 22, 64, 2), (3, 45, 53, 64, 1), (2, 40, 40, 32, 4)] and E.BN_HEAD_TWO_CHUNKS == (1, 1472, 1472, 8, 3)
    assert all(c in E.BN_CASES for c in E.BN_REV_CASES)


def test_leaky_slope_is_exact_on_multiples_of_five_only():
    """float32(x) * float32(0.2) == x / 5 for every multiple of 5 up to +-4000 (and of 5/4, the pre-activations under scales
    down to 1/4); general integers are not exact, and require_fifths refuses them"""
    x = torch.arange(-4000, 4001, 5, dtype=torch.float64)
    E.require_fifths(x, x / 4, x * 4)
    n = torch.arange(1, 4001, dtype=torch.float32)
    exact = (n * torch.tensor(0.2)).double() * 5 == n.double()
    assert bool(exact[4::5].all()) and 0.1 < float(exact.double().mean()) < 0.9
    with pytest.raises(AssertionError):
        E.require_fifths(torch.tensor([3.0]))


@pytest.mark.parametrize("case", _BN_ALL + _HEADS, ids=_bn_ident)
def test_bn_cases_are_exact_in_fp32_in_any_order(case):
    """building a case asserts its conditions; then the backward evaluated in fp32, its sums over a shuffled pixel order in
    runs of 64, equals the fp64 reference bit for bit, in both dtypes (the dtype enters through the rounded z of the pool).
    Zeros of v, tied windows and negative gamma are present in every case that can hold them."""
    c = _bn(case)
    assert c["zero_share"] > 0 and c["gamma_negative"] > 0
    if c["pooled"]:
        assert c["tie_share"] > 0
    for k in ("y", "dza", "dzb", "dzp"):
        if c[k] is not None and c["dza_kind"] != "head":
            for _, dt in DTS:
                _representable(c[k], dt)
    for i, (dtn, dt) in enumerate(DTS):
        if case == E.BN_HEAD_TWO_CHUNKS and dtn != "f16":
            continue                                            # runs in fp16 only
        ref = E.bn_reference(c, dt)
        got = E.bn_fp32_shuffled(c, dt, seed=i + 1)
        for k in ("gh", "s1", "s2", "dy"):
            assert torch.equal(got[k].double(), ref[k]), (k, dtn)
        expect32(ref["s1"], 0.5), expect32(ref["s2"], 0.5), expect16(ref["dy"], dt)
    if c["dza_kind"] == "head":                                 # the kernel's fp32 sum over the classes, in its order
        dl, wh = c["dl"], c["w_head"]
        t = dl[:, 0, None] * wh[0].view(1, -1, 1, 1)
        for k in range(1, c["ncls"]):
            t = t + dl[:, k, None] * wh[k].view(1, -1, 1, 1)
        assert t.dtype == torch.float32 and torch.equal(t.double(), c["dza"])


@pytest.mark.parametrize("case", E.BN_CASES + _HEADS, ids=_bn_ident)
def test_comparer_separates_every_bn_mutant(case):
    """each reference-level mutant that applies to a case changes dy (as the kernel stores it, rounded to the dtype) somewhere,
    and assert_exact reports it; the sums move too, except where a mutant only moves a gradient inside its window"""
    c = _bn(case)
    for dtn, dt in DTS:
        if case == E.BN_HEAD_TWO_CHUNKS and dtn != "f16":
            continue                                            # runs in fp16 only
        ref = E.bn_reference(c, dt)
        want = expect16(channels_last(ref["dy"]), dt)
        for m in E.BN_MUTANTS:
            if not E.bn_mutant_applies(c, m):
                continue
            mut = E.bn_reference(c, dt, m)
            got = expect16(channels_last(mut["dy"]), dt)
            n = E.mismatches(got, want).shape[0]
            assert n > 0, f"{_bn_ident(case)} {dtn}: mutant {m} is not told from the reference"
            with pytest.raises(AssertionError, match="elements differ"):
                E.assert_exact(got, want, m)
            if m not in ("last", "unrounded"):
                assert not (torch.equal(mut["s1"], ref["s1"]) and torch.equal(mut["s2"], ref["s2"])), (m, dtn)


@pytest.mark.parametrize("shape,pooled", E.TANH_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else ("pool" if v else "plain"))
def test_tanh_reference_in_fp32_rarely_lands_on_the_neighbour(shape, pooled):
    """tanh and dz * (1 - tanh^2) evaluated in fp32 on the CPU and rounded to 16 bits: every element is the correctly rounded
    fp64 value or its neighbour, and the neighbour's share stays under TANH_NEIGHBOUR_SHARE (the GPU test uses the same cap)"""
    r = E.tanh_build(shape, pooled)
    assert float(r["y"].abs().max()) == 1.5
    for _, dt in DTS:
        _representable(r["y"], dt)
        t = torch.tanh(r["y"])
        for got32, ref in ((t, r["z"]), (r["dz"] * (1 - t * t), r["dy"])):
            ok, share = E.neighbour16(got32.to(dt), ref)
            assert bool(ok.all()) and share <= E.TANH_NEIGHBOUR_SHARE, share
        two_off = (E.ordered16(r["z"].to(dt)) + 2).to(torch.int16).view(dt)
        assert not bool(E.neighbour16(two_off, r["z"])[0][r["z"] > 0].any())


@pytest.mark.parametrize("ntiles", E.BN_FINALIZE_TILES)
def test_bn_finalize_reference_and_its_bounds(ntiles):
    """the edge channels are what they claim (a negative raw variance that clamps, |mean| = 100 std), and gs_bn_finalize's
    arithmetic replayed in numpy fp32 meets the rounding-count bounds the GPU test asserts"""
    import numpy as np
    for C in E.BN_FINALIZE_C:
        for count_one in ((False, True) if ntiles == 1 else (False,)):
            r = E.bn_finalize_build(C, ntiles, count_one)
            ref = E.bn_finalize_reference(r)
            assert ref["raw_var"][0] < 0 and ref["invstd"][0] == 1.0 / np.sqrt(float(np.float32(E.BN_EPS)))
            assert r["count"] == (1.0 if count_one else 64.0 * ntiles)
            if not count_one:
                assert 50 < abs(ref["mean"][1]) * ref["invstd"][1] < 200
            f = np.float32
            invstd = f(ref["invstd"])
            sc = r["gamma"].numpy() * invstd
            sh = r["beta"].numpy() - f(ref["mean"]) * sc
            rm = (f(1) - f(E.BN_MOMENTUM)) * r["rm"].numpy() + f(E.BN_MOMENTUM) * f(ref["mean"])
            var = np.maximum(ref["raw_var"], 0.0)
            unb = var * (r["count"] / (r["count"] - 1.0)) if r["count"] > 1 else var
            rv = (f(1) - f(E.BN_MOMENTUM)) * r["rv"].numpy() + f(E.BN_MOMENTUM) * f(unb)
            assert sc.dtype == sh.dtype == rm.dtype == rv.dtype == np.float32
            for name, got in (("mean", f(ref["mean"])), ("invstd", invstd), ("scale", sc), ("shift", sh), ("rm", rm), ("rv", rv)):
                assert np.all(np.abs(got.astype(np.float64) - ref[name]) <= E.coeff_bound(ref, name, E.BN_FINALIZE_ROUNDINGS)), name
