"""What entitles tests/test_stem_kernels_gpu.py to its zero tolerance, proved on the CPU (no GPU, no native library):

  - the case list reaches the edges it names: pixels per block, block and tile counts, the loop iterations and unroll slots of
    the backward kernels, the 64 KiB strip and its refusal are re-derived from the host formulas;
  - the reference's flat-strip taps ARE the convolution (against F.unfold / F.conv2d);
  - every case meets its exactness conditions: an fp32 evaluation in shuffled order equals the fp64 reference bit for bit, hi + lo
    is the unrounded activation exactly, the sign of the stored z is the sign of v;
  - gs_stem_bwd_finalize: the kernel's closed form equals the pixel-by-pixel definition in exact rational arithmetic, and on counts
    that are a power of two every fp64 intermediate of the kernel's formula has fewer than 53 significant bits;
  - the comparer separates the reference from each mutant of stem_reference.STEM_MUTANTS on every case where the mutant applies."""
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

from tests import exact_reference as E
from tests import stem_reference as S
from tests.exact_reference import DTS

_BUILT = {}


def built(case):
    if case not in _BUILT:
        if len(_BUILT) > 3:
            _BUILT.clear()
        _BUILT[case] = S.stem_build(case)
    return _BUILT[case]


def test_case_list_reaches_the_edges_it_names():
    for shape, (ppb, nb, tiles) in S.STEM_SHAPES.items():
        M = shape[0] * shape[1] * shape[2]
        assert (S.stem_bwd_ppb(M), S.stem_bwd_blocks(M), S.stem_fwd_tiles(M)) == (ppb, nb, tiles), shape
        assert S.stem_lds_bytes(*shape) <= S.LDS_LIMIT
        assert all((min(b * ppb + ppb, M) - b * ppb) % S.LOOP_STEP for b in range(nb)), "drop_tail would not apply to every block"
    for shape in [(1, 1, 1), (1, 1, 5), (1, 7, 1), (2, 3, 3)]:
        assert shape[0] * shape[1] * shape[2] < 64                      # one partial wave, ppb > M
    assert S.pow2_count((1, 32, 32)) and S.pow2_count((2, 64, 64)) and 32 * 32 == S.SC_TILE
    assert not any(S.pow2_count(s) for s in [(2, 18, 22), (3, 45, 53), (3, 160, 150), (2, 224, 224), (1, 2, 4959)])
    assert S.STEM_SHAPES[(2, 64, 64)][0] == 64                           # blocks coincide with rows
    assert S.STEM_SHAPES[(3, 45, 53)][2] % S.SC_GROUP != 0 and 64 % 53 != 0 and (45 * 53) % 64 != 0
    # ppb = 141: pixel lane pl runs a second iteration while pl + 128 < 141; the last block is ragged
    assert sum(1 for pl in range(32) if pl + S.LOOP_STEP < 141) == 13 and 72000 - 510 * 141 == 90
    # ppb = 196 = 128 + 68: the first iteration fills all four slots, the second runs on every lane (68 >= 32) with a clamped tail
    assert 196 == S.LOOP_STEP + 68 and all(pl + S.LOOP_STEP < 196 for pl in range(32)) and 196 % 32 != 0 and 141 % 32 != 0
    # the strip: W = 4959 needs exactly 64 KiB, its neighbour is refused
    assert S.stem_lds_bytes(1, 2, 4959) == S.LDS_LIMIT and S.stem_lds_bytes(*S.STEM_REFUSED) > S.LDS_LIMIT
    assert S.widest_accepted(1, 2) == 4959 and S.STEM_REFUSED == (1, 2, S.widest_accepted(1, 2) + 1)
    assert len(S.STEM_CASES) == 2 * (len(S.STEM_SHAPES) + 2 * len(S.STEM_ALL_ACTS))


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 5), (1, 7, 1), (2, 3, 3), (3, 45, 53)])
def test_the_flat_strip_taps_are_the_convolution(shape):
    c = built((shape, "relu", "P"))
    N, H, W = shape
    X = S.stem_taps(c["x"])
    unf = F.unfold(c["x"].double(), 3, padding=1).permute(0, 2, 1).reshape(N * H * W, 9)
    assert torch.equal(X, unf)
    y = F.conv2d(c["x"].double(), c["w"].double(), None, padding=1).permute(0, 2, 3, 1).reshape(N * H * W, 64)
    assert torch.equal(X @ c["w"].double().view(64, 9).t(), y)


@pytest.mark.parametrize("case", S.STEM_CASES, ids=S.case_id)
def test_every_case_is_exact_in_fp32_in_any_order(case):
    c = built(case)                                                        # asserts the operand conditions
    shape, act, iset = case
    M = shape[0] * shape[1] * shape[2]
    assert c["zero_share"] > 0, "no v == 0 planted"
    for dtn, dt in DTS:
        ref = S.stem_reference(c, dt)
        shuf = S.stem_fp32_shuffled(c, dt, seed=E.case_seed((case, dtn)))
        for k in ("hi", "lo"):
            assert torch.equal(shuf[k], ref[k]), (k, dtn)
        for k in ("z", "s1", "A"):
            assert torch.equal(shuf[k].double(), ref[k]), (k, dtn)
        assert torch.equal(ref["hi"].double() + ref["lo"].double(), ref["z"]), f"{dtn}: z - hi is not a {dtn} number somewhere"
        assert float(ref["lo"].abs().max()) > 0, f"{dtn}: the lo plane is zero"
        if act != "none":
            assert torch.equal(ref["hi"].view(M, 64) > 0, ref["v"] > 0), "the stored z lost the sign of v"
        if act == "relu":                                                  # a gradient sits on a planted zero of every channel c % 4 == 0
            dz = c["dz"].permute(0, 2, 3, 1).reshape(M, 64)
            assert all(ref["v"][S.planted_pixel(ch, M), ch] == 0 and dz[S.planted_pixel(ch, M), ch] != 0 for ch in range(0, 64, 4))
    x = c["x"]
    rows = sorted({r for r in (0, 1, shape[1] - 2, shape[1] - 1) if 0 <= r < shape[1]})
    assert bool((x[:, 0, rows][:, :, [0, shape[2] - 1]] != 0).all()), "a planted image pixel is zero"
    assert float(x.min()) == (-1 if iset == "T" else 0) or M < 8


def _as_fractions(t):
    return [Fraction(v) for v in t.reshape(-1).tolist()]


@pytest.mark.parametrize("case", S.STEM_CASES, ids=S.case_id)
def test_finalize_closed_form_is_the_definition_and_fits_fp64(case):
    c = built(case)
    ref = S.stem_reference(c, torch.float16)                               # s1, A, g do not depend on the dtype
    sums = S.stem_pixel_sums(c, ref)
    assert torch.equal(sums["P1"], ref["A"]) and torch.equal(sums["s1"], ref["s1"])
    for train in (True, False):
        for gscale in (0.5, 1.0):
            want = S.stem_finalize_definition(c, sums, train, gscale)
            closed = S.stem_finalize_closed(c, ref, train, gscale)
            assert closed["dW"] == want["dW"], "the closed form is not the definition"
            if S.pow2_count(case[0]) or not train:
                assert closed["bits"] < 53, f"an fp64 intermediate of the kernel's formula needs {closed['bits']} bits"
                assert all(Fraction(float(v)) == v for v in want["dW"] + want["dgamma"] + want["dbeta"])
            else:
                assert closed["bits"] == float("inf")                      # s1 / count is no binary number: the bound applies
                assert all(S.finalize_bound(v, m) >= abs(v) * Fraction(1, 2 ** 24) for v, m in zip(want["dW"], want["mag"]))
    eval_ = S.stem_finalize_definition(c, sums, False, 1.0)                # eval statistics: dW = gscale * scale * A
    scale = _as_fractions(c["scale"])
    assert eval_["dW"] == [scale[i // 9] * v for i, v in enumerate(_as_fractions(ref["A"]))]
    assert closed["dgamma"] == want["dgamma"] and closed["dbeta"] == want["dbeta"]


@pytest.mark.parametrize("shape", S.FINALIZE_SYNTHETIC, ids=lambda s: "x".join(map(str, s)))
def test_synthetic_finalize_cases_reach_the_unrolled_tile_loop(shape):
    """16 lanes, 8 loads in flight: a lane runs an unrolled round while b + 7 * 16 < tiles; no image of STEM_SHAPES has more than 98"""
    assert max(v[2] for v in S.STEM_SHAPES.values()) <= 7 * 16
    r = S.finalize_synthetic_build(shape)
    assert r["nsg"] > 7 * 16 and r["nb"] > 7 * 24
    tails = sum(1 for lane in range(16) if lane + 8 * 16 < r["nsg"])
    assert tails == (0 if S.pow2_count(shape) else 12)
    E.require_integers(r["w"], r["mean"], r["taps"], r["s1p"], r["ws"])
    ref = S.finalize_closed_from_sums(r, r["S"], r["packed"], r["s1"], r["A"], r["count"], True, 0.5)
    if S.pow2_count(shape):
        assert ref["bits"] < 53 and all(Fraction(float(v)) == v for v in ref["dW"])
    for m in ("gram_row_major_full", "no_mean_term"):
        mut = S.finalize_closed_from_sums(r, r["S"], r["packed"], r["s1"], r["A"], r["count"], True, 0.5, m)
        assert any(abs(a - b) > S.finalize_bound(b, g) for a, b, g in zip(mut["dW"], ref["dW"], ref["mag"])), m


def _differs(a, b) -> bool:
    return E.mismatches(a, b).shape[0] > 0


@pytest.mark.parametrize("case", S.STEM_CASES, ids=S.case_id)
def test_comparer_separates_every_stem_mutant(case):
    """each mutant that applies to a case changes an output the GPU test compares, and assert_exact reports it:
      row_wrap, image_wrap, tap_transposed  hi (the forward) and A (the backward)
      relu0_live, drop_tail                 s1 and A
      lo_of_unrounded                       lo
      gram_row_major_full, no_mean_term     the train-mode dW of the finalize"""
    c = built(case)
    for dtn, dt in DTS:
        ref = S.stem_reference(c, dt)
        for m in S.STEM_MUTANTS:
            if m in ("gram_row_major_full", "no_mean_term"):
                continue
            if not S.mutant_applies(c, m):
                mut = S.stem_reference(c, dt, m)
                assert all(torch.equal(mut[k], ref[k]) for k in ("hi", "lo", "s1", "A")), f"{m} does not apply, yet it changes the case"
                continue
            mut = S.stem_reference(c, dt, m)
            outs = {"row_wrap": ("hi", "A"), "image_wrap": ("hi", "A"), "tap_transposed": ("hi", "A"), "relu0_live": ("s1", "A"),
                    "drop_tail": ("s1", "A"), "lo_of_unrounded": ("lo",)}[m]
            for k in outs:
                assert _differs(mut[k], ref[k]), f"{S.case_id(case)} {dtn}: mutant {m} is not told from the reference on {k}"
                with pytest.raises(AssertionError, match="elements differ"):
                    E.assert_exact(mut[k], ref[k], m)
    ref = S.stem_reference(c, torch.float16)
    want = S.stem_finalize_closed(c, ref, True, c["gscale"])["dW"]
    sums = S.stem_pixel_sums(c, ref)
    mag = S.stem_finalize_definition(c, sums, True, c["gscale"])["mag"]
    for m in ("gram_row_major_full", "no_mean_term"):
        assert S.finalize_mutant_applies(c, m, True) and not S.finalize_mutant_applies(c, m, False)
        mut = S.stem_finalize_closed(c, ref, True, c["gscale"], m)["dW"]
        if S.pow2_count(case[0]):
            seen = [i for i, (a, b) in enumerate(zip(mut, want)) if float(a) != float(b)]
        else:                                                              # outside the bound the GPU test allows
            seen = [i for i, (a, b) in enumerate(zip(mut, want)) if abs(a - b) > S.finalize_bound(b, mag[i])]
        assert seen, f"{S.case_id(case)}: mutant {m} is not told from the reference"
        assert S.stem_finalize_closed(c, ref, False, c["gscale"], m)["dW"] == S.stem_finalize_closed(c, ref, False, c["gscale"])["dW"]


@pytest.mark.parametrize("case", S.STEM_CASES, ids=S.case_id)
def test_stored_y_fallback_cases_are_exact_and_tell_their_mutants(case):
    c = S.wgrad_build(case)
    worst = S.wgrad_conditions(c)
    assert worst < E.LIMIT
    ref = S.wgrad_reference(c)
    assert torch.equal(S.wgrad_fp32_shuffled(c, seed=E.case_seed(case)), ref["dw"])
    for m in S.TAP_MUTANTS + ("relu0_live", "drop_tail"):
        mut = S.wgrad_reference(c, m)["dw"]
        if S.mutant_applies(c, m):
            assert _differs(mut, ref["dw"]), f"{S.case_id(case)}: mutant {m} is not told from the reference"
        else:
            assert torch.equal(mut, ref["dw"])
