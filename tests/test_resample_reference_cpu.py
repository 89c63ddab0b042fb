"""The fp64 statements of csrc/resample.hip (tests/resample_reference.py) proven on the CPU:
  * the exact-weight forward IS F.interpolate(scale_factor=2, bilinear, align_corners=True) + F.pad in double, the backward its
    torch.autograd, the warp F.grid_sample(bilinear, zeros, align_corners=False) on the grid equivalent to the matrix, all at 1e-12;
    the fp32-coordinate weights stay within in * 2^-23 of the exact ones for every `in` of the case lists;
  * on the very cases of the GPU tests a right implementation (the statement re-evaluated in fp32 in another order, stored to 16 bits)
    passes every bound, and every stated wrong implementation fails the case named in CAUGHT_BY -- or is stated invisible;
  * the two conditions of the threshold tests hold: pixels sit exactly on the threshold, and at most 1 % of the pixels of a general
    case lie within their own bound of it;
  * the host side of the augmentation: every stage on points, the composition in the drawn order, the inverse handed to the kernel."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resample_reference as rr

torch.set_num_threads(min(torch.get_num_threads(), 16))
DTS = rr.DTYPES
CASES = {c[0]: c for c in rr.UP_CASES}
PAIRS = {c[0]: c for c in rr.PAIR_CASES}
SIZES = sorted({n for c in rr.UP_CASES + rr.PAIR_CASES for n in c[2:4]} | set(rr.GRID_FWD[1:3]) | set(rr.GRID_BWD[1:3]))


# ------------------------------------------------------------------------------------------------ the statements are the independent ones
@pytest.mark.parametrize("name", rr.UP_IDS)
def test_exact_forward_is_interpolate_plus_pad_and_backward_its_autograd(name):
    case = CASES[name]
    _, N, h, w, C, pad = case[:6]
    C = min(C, 8)
    geo = rr.geometry(N, h, w, C, pad, "dense", "dense")
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, h, w, C, generator=g, dtype=torch.float64)
    dy = torch.randn(N, geo["PH"], geo["PW"], C, generator=g, dtype=torch.float64)
    Wy, Wx = rr.case_weights(h, w, coords="exact")
    mine = torch.zeros(N, geo["PH"], geo["PW"], C, dtype=torch.float64)
    rr.patch(mine, geo)[...] = rr.up_fwd64(x, Wy, Wx)
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    up = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=True)
    pt, pl = pad[0] // 2, pad[1] // 2
    ref = F.pad(up, [pl, pad[1] - pl, pt, pad[0] - pt])
    assert float((mine - ref.detach().permute(0, 2, 3, 1)).abs().max()) < 1e-12
    ref.backward(dy.permute(0, 3, 1, 2))
    back = rr.up_bwd64(rr.patch(dy, geo), Wy, Wx)
    assert float((back - xt.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-12


def test_fp32_coordinate_weights_stay_within_the_stated_distance_of_the_exact_ones():
    assert {1, 2, 3, 7, 13, 33, 40, 64, 128} <= set(SIZES)
    for n in SIZES:
        W32, Wex = rr.up_weights(n, "fp32"), rr.up_weights(n, "exact")
        d = float((W32 - Wex).abs().max())
        print(f"in = {n}: fp32 against exact weights {d:.3e}, stated {rr.coord_weight_distance(n):.3e}")
        assert d <= rr.coord_weight_distance(n)
        assert float((W32.sum(1) - 1).abs().max()) == 0.0 and float((Wex.sum(1) - 1).abs().max()) < 1e-15
        assert bool((W32 >= 0).all()) and int((W32 != 0).sum(1).max()) <= 2


def _grid_of(mats, H, W):
    sx, sy = rr._warp_coords(mats, H, W)
    return torch.stack([2 * (sx + 0.5) / W - 1, 2 * (sy + 0.5) / H - 1], -1)


def test_warp_is_grid_sample():
    for name, (src, mats) in rr.general_warp_cases().items():
        ref = F.grid_sample(src.double(), _grid_of(mats, *src.shape[2:]), mode="bilinear", padding_mode="zeros", align_corners=False)
        assert float((rr.warp64(src.double(), mats) - ref).abs().max()) < 1e-12, name
    for name, (N, C, H, W, mats) in rr.exact_warp_cases().items():
        src, m = rr.warp_case_data(name, N, C, H, W).double(), torch.tensor(mats, dtype=torch.float32)
        ref = F.grid_sample(src, _grid_of(m, H, W), mode="bilinear", padding_mode="zeros", align_corners=False)
        assert float((rr.warp64(src, m) - ref).abs().max()) < 1e-12, name


def test_grid_stride_cases_exceed_one_pass_of_the_capped_grid():
    cap = 8192 * 256
    N, h, w, C = rr.GRID_FWD
    assert N * 4 * h * w * (C // 8) > cap and N * 4 * h * w * (C // 8) < 2 ** 31
    N, h, w, C = rr.GRID_BWD
    assert N * h * w * (C // 8) > cap and N * 4 * h * w * (C // 8) < 2 ** 31
    N, C, H, W, _ = rr.GRID_WARP
    assert N * C * H * W > cap


# ------------------------------------------------------------------------------------------------ a right implementation passes
@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("name", rr.UP_IDS)
def test_right_bilinear_implementation_passes(name, dtn, dt):
    case = CASES[name]
    geo = rr.case_geometry(case)
    x, g = rr.up_case_data(case, dt)
    for swap in (False, True):
        yhi, _ = rr.model_up_fwd(x, geo, dt, swap)
        n, r, kept = rr.hold_up_fwd(yhi, x, geo, dt)
        assert n == 0 and kept, (swap, n, r)
        if name in ("one", "one_pad"):                                     # a 1 x 1 input: the forward is a copy
            assert torch.equal(rr.patch(yhi, geo).double(), x.expand(-1, 2, 2, -1))
    dx = rr.model_up_bwd(g, geo, dt, seed=5)
    n, r, kept = rr.hold_up_bwd(dx, g, geo, dt)
    assert n == 0 and kept, (n, r)
    if name in rr.RANDOM_UP_IDS:
        Wy, Wx = rr.case_weights(geo["h"], geo["w"])
        d, b = rr.adjointness(x, rr.patch(yhi, geo), g, rr.lo_slice(dx, geo), Wy, Wx)
        assert d <= b and d > 0, (d, b)


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_right_pair_implementation_passes(name, dtn, dt):
    case = PAIRS[name]
    geo = rr.geometry(*case[1:8])
    hi, lo = rr.pair_case_data(case, dt)
    assert float(lo.float().abs().max()) > 0
    val = hi.double() + lo.double()
    assert torch.equal((hi.float() + lo.float()).double(), val), "the join of a split pair is exact in fp32 (no rounding counted)"
    yhi, ylo = rr.model_up_fwd(val, geo, dt, True)
    n, r, nh, rh, kept = rr.hold_up_pair(yhi, ylo, val, geo, dt)
    assert n == 0 and nh == 0 and kept, (n, r, nh, rh)
    # pair_lo_dropped: caught by every pair case
    yhi, ylo = rr.model_up_fwd(val, geo, dt, True, mutant="pair_lo_dropped", lo_plane=lo)
    assert rr.hold_up_pair(yhi, ylo, val, geo, dt)[0] > 0


# ------------------------------------------------------------------------------------------------ the wrong ones fail
# mutant -> the case that catches it (None: invisible to the case lists, said below)
CAUGHT_BY = {
    "align_false": "wide", "clamp_early": "wide", "unclamped": None, "xy_swapped": "wide",
    "pad_top_left": "two", "pad_dropped": "row", "slice_from_0": "tall",
    "window_short_low": "tall", "window_short_high": "tall", "ignore_r0": "one",
}


def _fwd_fails(name, mutant, dt):
    case = CASES[name]
    geo = rr.case_geometry(case)
    x, _ = rr.up_case_data(case, dt)
    n, _, kept = rr.hold_up_fwd(rr.model_up_fwd(x, geo, dt, False, mutant=mutant)[0], x, geo, dt)
    return n > 0 or not kept


def _bwd_fails(name, mutant, dt):
    case = CASES[name]
    geo = rr.case_geometry(case)
    _, g = rr.up_case_data(case, dt)
    n, _, kept = rr.hold_up_bwd(rr.model_up_bwd(g, geo, dt, 0, mutant=mutant), g, geo, dt)
    return n > 0 or not kept


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("mutant", rr.WEIGHT_MUTANTS + rr.PLACE_MUTANTS)
def test_wrong_forward_fails(mutant, dtn, dt):
    caught = {name for name in rr.UP_IDS if _fwd_fails(name, mutant, dt)}
    print(mutant, dtn, "caught by", sorted(caught))
    if CAUGHT_BY[mutant] is None:
        # an unclamped i1 reads the pixel behind the row with the weight l of the last output, which is 0 or a rounding of the fp32
        # coordinate: invisible in value to any case (it shows only as a read outside the tensor)
        assert not caught and all(rr.unclamped_weight(n) <= 2.0 ** -20 for n in SIZES)
        return
    assert CAUGHT_BY[mutant] in caught
    if mutant == "xy_swapped":
        assert not caught & {"one", "one_pad", "two"}, "invisible on a square shape"
    if mutant == "slice_from_0":
        assert caught == {"one_pad", "tall"}, "visible only where the input is a slice"
    if mutant == "clamp_early":
        assert "mid_pl" in caught and "tall" in caught


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("mutant", rr.BWD_MUTANTS + ("pad_top_left", "pad_dropped", "align_false", "clamp_early", "xy_swapped"))
def test_wrong_backward_fails(mutant, dtn, dt):
    caught = {name for name in rr.UP_IDS if _bwd_fails(name, mutant, dt)}
    print(mutant, dtn, "caught by", sorted(caught))
    assert CAUGHT_BY[mutant] in caught
    if mutant == "ignore_r0":
        assert caught == {"one", "one_pad", "row", "col"}, "the cases with a 1-pixel axis"
    if mutant.startswith("window_short"):
        assert {"two", "wide", "tall", "mid_pl"} <= caught


def _exact_case(name, hi=8):
    N, C, H, W, mats = rr.exact_warp_cases()[name]
    return rr.warp_case_data(name, N, C, H, W, hi).double(), torch.tensor(mats, dtype=torch.float32)


def test_exact_warp_cases_are_exact_and_say_what_they_say():
    for name in rr.exact_warp_cases():
        src, m = _exact_case(name)
        ref = rr.warp64(src, m)
        assert torch.equal(rr.model_warp(src, m).double(), ref), name                 # every fp32 step is exact
        assert torch.equal(ref * 4, torch.round(ref * 4)), name                        # dyadic averages
    src, m = _exact_case("identity")
    assert torch.equal(rr.warp64(src, m), src)
    src, m = _exact_case("translate")
    out = rr.warp64(src, m)
    assert torch.equal(out[0, :, 3:, 1:], src[0, :, :-3, :-1]) and float(out[0, :, :3].abs().max()) == 0       # moved by (+1, +3)
    assert torch.equal(out[3, :, :-3, :-1], src[3, :, 3:, 1:])
    src, m = _exact_case("translate_out")
    assert float(rr.warp64(src, m).abs().max()) == 0
    src, m = _exact_case("flip")
    out = rr.warp64(src, m)
    assert torch.equal(out[0], src[0].flip(-1)) and torch.equal(out[1], src[1].flip(-2))
    src, m = _exact_case("turns")
    out = rr.warp64(src, m)
    assert torch.equal(out[0], src[0].transpose(-1, -2)) and torch.equal(out[1], src[1])
    assert torch.equal(out[2], torch.rot90(src[2], 3, (-2, -1))) and torch.equal(out[3], torch.rot90(src[3], 2, (-2, -1)))
    assert torch.equal(out[4], torch.rot90(src[4], 1, (-2, -1)))
    src, m = _exact_case("half")
    out = rr.warp64(src, m)
    assert torch.equal(out[0, :, :, :-1], (src[0, :, :, :-1] + src[0, :, :, 1:]) / 2)
    assert torch.equal(out[2, :, :-1, :-1], (src[2, :, :-1, :-1] + src[2, :, :-1, 1:] + src[2, :, 1:, :-1] + src[2, :, 1:, 1:]) / 4)
    src, m = _exact_case("shrink")
    out = rr.warp64(src, m)
    assert torch.equal(out[..., :8, :12], F.avg_pool2d(src, 2)) and float(out[..., 8:, :].abs().max()) == 0
    N, C, H, W, mats = rr.GRID_WARP
    src = torch.arange(N * C * 8 * 8, dtype=torch.float64).reshape(N, C, 8, 8)
    out = rr.warp64(src, torch.tensor([[-1, 0, 8, 0, 1, 0], [1, 0, 0, 0, -1, 8], [-1, 0, 8, 0, -1, 8.0]]))
    assert torch.equal(out[0], src[0].flip(-1)) and torch.equal(out[1], src[1].flip(-2)) and torch.equal(out[2], src[2].flip(-1, -2))


def test_threshold_cases_have_ties_and_tell_the_wrong_warps_apart():
    for name, t in rr.THRESH_CASES:
        src, m = _exact_case(name, hi=1)
        raw = rr.warp64(src, m)
        ties = int((raw == t).sum())
        print(f"{name} at {t}: {ties} of {raw.numel()} pixels exactly on the threshold")
        assert ties > 0
        ref = rr.warp64(src, m, t)
        assert set(ref.unique().tolist()) <= {0.0, 1.0} and float(ref[raw == t].max()) == 0.0       # strict: a tie gives 0
        assert int((rr.warp64(src, m, t, mutant="ge") != ref).sum()) == ties                          # >= turns exactly the ties
        assert torch.equal(rr.model_warp(src, m, t).double(), ref)
        if t == 0.0:
            assert not torch.equal(ref, raw), "thresh = 0 binarises: the raw values are not the answer"
    name, t = rr.BORDER_CASE
    src, m = _exact_case(name, hi=1)
    ref, clamped = rr.warp64(src, m, t), rr.warp64(src, m, t, mutant="clamp_border")
    flips = ref != clamped
    assert int(flips.sum()) > 0
    assert int(flips[0, :, 1:, 1:].sum()) == 0 and int(flips[1, :, :-1, :-1].sum()) == 0, "only the border row / column"


def test_wrong_warps_fail():
    # without the half-pixel convention: caught by the flips (moved by one pixel); identity and translations cannot see it
    src, m = _exact_case("flip")
    assert not torch.equal(rr.warp64(src, m, mutant="no_half_pixel"), rr.warp64(src, m))
    src, m = _exact_case("shrink")
    assert not torch.equal(rr.warp64(src, m, mutant="no_half_pixel"), rr.warp64(src, m))
    for name in ("identity", "translate"):
        src, m = _exact_case(name)
        assert torch.equal(rr.warp64(src, m, mutant="no_half_pixel"), rr.warp64(src, m)), "invisible here"
    # clamped border taps, raw: caught by the translations too
    src, m = _exact_case("translate")
    assert not torch.equal(rr.warp64(src, m, mutant="clamp_border"), rr.warp64(src, m))
    # matrix row n C + c: caught by the case with C = 2 and three different matrices; invisible with C = 1
    src, m = _exact_case("per_sample")
    assert not torch.equal(rr.warp64(src, m, mutant="mat_nc"), rr.warp64(src, m))
    src, m = _exact_case("flip")
    assert torch.equal(rr.warp64(src, m, mutant="mat_nc"), rr.warp64(src, m))


@pytest.fixture(scope="module")
def general():
    return rr.general_warp_cases()


def test_general_warp_right_passes_wrong_fails_and_the_adjacent_share_is_small(general):
    from semantic_segmentation_amd.augment import sample_forward_matrix
    S = rr.GENERAL_SIZE
    for name, (src, mats) in general.items():
        s64 = src.double()
        n, r = rr.hold_warp_raw(rr.model_warp(src, mats), s64, mats)
        assert n == 0, (name, n, r)
        bad, share = rr.hold_warp_binary(rr.model_warp(src, mats, 0.1), s64, mats, 0.1)
        print(f"{name}: right implementation at {r:.3f} of the bound; {share:.5f} of the pixels within their bound of the threshold")
        assert bad == 0 and share <= rr.ADJACENT_CAP, (name, bad, share)
        for mutant in ("no_half_pixel", "clamp_border"):
            if mutant == "clamp_border" and name.endswith("_mask"):
                continue                                                   # a mask that is 0 along its border: invisible
            assert rr.hold_warp_raw(rr.warp64(s64, mats, mutant=mutant), s64, mats)[0] > 0, (name, mutant)
        assert rr.hold_warp_binary(rr.warp64(s64, mats, 0.1, mutant="no_half_pixel"), s64, mats, 0.1)[0] > 0, name
    # the forward matrix handed over instead of its inverse: caught by every seed, raw and binarised
    for seed in rr.GENERAL_SEEDS:
        rng = np.random.default_rng(seed)
        fwd = torch.from_numpy(np.stack([sample_forward_matrix(rng, S, S)[:2].reshape(6) for _ in range(3)]).astype(np.float32))
        for kind in ("random", "mask"):
            src, mats = general[f"seed{seed}_{kind}"]
            assert rr.hold_warp_raw(rr.warp64(src.double(), fwd), src.double(), mats)[0] > 0
            assert rr.hold_warp_binary(rr.warp64(src.double(), fwd, 0.1), src.double(), mats, 0.1)[0] > 0


# ------------------------------------------------------------------------------------------------ the host side of the augmentation
class StubRng:
    """fixes the draws of sample_forward_matrix: random() -> flip, then the uniform draws in their order, then the permutation"""

    def __init__(self, flip, pads=(0, 0, 0, 0), scale=(1, 1), translate=(0, 0), rotate=0.0, shear=0.0, order=None):
        self.flip, self.order = flip, order
        self.queue = [np.array(pads, dtype=np.float64), np.array(scale, dtype=np.float64), np.array(translate, dtype=np.float64),
                      float(rotate), float(shear)]

    def random(self):
        return 0.25 if self.flip else 0.75

    def uniform(self, lo, hi, size=None):
        v = self.queue.pop(0)
        assert (np.ndim(v) == 0) == (size is None) and (size is None or len(v) == size)
        assert np.all(v >= lo) and np.all(v <= hi)
        return v

    def permutation(self, n):
        assert n == (6 if self.flip else 5)
        return np.arange(n) if self.order is None else np.array(self.order)


def _apply(m, x, y):
    p = m @ np.array([x, y, 1.0])
    assert p[2] == 1.0
    return p[0], p[1]


def test_augmentation_stages_do_what_their_comments_say():
    from semantic_segmentation_amd.augment import sample_forward_matrix
    h, w = 40, 56
    cx, cy = w / 2, h / 2
    near = lambda p, q: np.allclose(p, q, rtol=0, atol=1e-12)
    assert np.array_equal(sample_forward_matrix(StubRng(False), h, w), np.eye(3))
    flip = sample_forward_matrix(StubRng(True), h, w)                      # Fliplr: x -> w - x
    assert near(_apply(flip, 3.0, 7.0), (w - 3.0, 7.0)) and near(_apply(flip, 0.0, 0.0), (w, 0.0))
    top, right, bottom, left = 0.02, 0.1, 0.05, 0.07                       # CropAndPad: the padded frame's corners -> the image corners
    pad = sample_forward_matrix(StubRng(False, pads=(top, right, bottom, left)), h, w)
    assert near(_apply(pad, -left * w, -top * h), (0, 0)) and near(_apply(pad, w + right * w, h + bottom * h), (w, h))
    scale = sample_forward_matrix(StubRng(False, scale=(0.8, 1.2)), h, w)  # scale, rotate, shear fix the centre
    assert near(_apply(scale, cx, cy), (cx, cy)) and near(_apply(scale, cx + 10, cy + 10), (cx + 8, cy + 12))
    rot = sample_forward_matrix(StubRng(False, rotate=15.0), h, w)
    a = math.radians(15.0)
    assert near(_apply(rot, cx, cy), (cx, cy)) and near(_apply(rot, cx + 10, cy), (cx + 10 * math.cos(a), cy + 10 * math.sin(a)))
    shear = sample_forward_matrix(StubRng(False, shear=8.0), h, w)
    assert near(_apply(shear, cx, cy), (cx, cy)) and near(_apply(shear, cx, cy + 10), (cx - 10 * math.tan(math.radians(8.0)), cy + 10))
    tr = sample_forward_matrix(StubRng(False, translate=(0.1, -0.05)), h, w)           # translate: by t w, t h
    assert near(_apply(tr, 1.0, 2.0), (1.0 + 0.1 * w, 2.0 - 0.05 * h))


def test_sample_forward_matrix_is_the_product_of_its_stages_in_the_drawn_order():
    from semantic_segmentation_amd.augment import sample_forward_matrix
    h, w = 40, 56
    draws = dict(pads=(0.02, 0.1, 0.05, 0.07), scale=(0.8, 1.2), translate=(0.1, -0.05), rotate=15.0, shear=-8.0)
    singles = [sample_forward_matrix(StubRng(True), h, w)] + [sample_forward_matrix(StubRng(False, **{k: v}), h, w) for k, v in draws.items()]
    for flip, order in ((True, [3, 1, 5, 0, 2, 4]), (True, [0, 1, 2, 3, 4, 5]), (False, [4, 2, 0, 3, 1])):
        stages = singles if flip else singles[1:]
        want = np.eye(3)
        for i in order:
            want = stages[i] @ want
        got = sample_forward_matrix(StubRng(flip, order=order, **draws), h, w)
        assert np.allclose(got, want, rtol=0, atol=1e-12), (flip, order)
    a = sample_forward_matrix(StubRng(True, order=[3, 1, 5, 0, 2, 4], **draws), h, w)
    b = sample_forward_matrix(StubRng(True, order=[0, 1, 2, 3, 4, 5], **draws), h, w)
    assert not np.allclose(a, b, atol=1e-3), "the order matters"


def test_matrices_are_the_inverses_in_the_row_layout_the_kernel_reads():
    from semantic_segmentation_amd.augment import MaskAugmenter, sample_forward_matrix
    n, h, w = 5, 48, 64
    unit = np.diag([1.0 / w, 1.0 / h, 1.0])                                 # in units of the image: fp32 entries of size O(1)
    for seed in rr.GENERAL_SEEDS:
        mats = MaskAugmenter(seed=seed).matrices(n, h, w)
        assert mats.shape == (n, 6) and mats.dtype == np.float32
        assert np.array_equal(mats, MaskAugmenter(seed=seed).matrices(n, h, w)), "two augmenters with one seed agree"
        rng = np.random.default_rng(seed)
        for i in range(n):
            inv = np.vstack([mats[i].astype(np.float64).reshape(2, 3), [0, 0, 1]])      # [a b c; d e f]
            prod = unit @ inv @ sample_forward_matrix(rng, h, w) @ np.linalg.inv(unit)
            assert np.abs(prod - np.eye(3)).max() < 1e-6, (seed, i, prod)
    assert not np.array_equal(MaskAugmenter(seed=3).matrices(2, h, w), MaskAugmenter(seed=5).matrices(2, h, w))
