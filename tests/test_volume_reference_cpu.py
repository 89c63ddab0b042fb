"""CPU checks for the volume transform: the fp64 statements of tests/volume_reference.py agree with torch's own fp32 evaluation of the
reference's transform, the integer cases really have exact sums and carry what they claim to plant, restore inverts prepare, each
stated mutant is told apart by some case, and the six entry points are declared (with their citations), bound, exported with ABI 54
and refuse bad arguments before any device work.  No GPU."""
import os
import re
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import volume_reference as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gs_volume_stats_ws_doubles", "gs_volume_nonzero_stats", "gs_volume_prepare", "gs_volume_restore_labels",
               "gs_label_sums_ws_int64", "gs_label_sums")
REGULAR = [n for n in V.CASES if n not in V.DEGENERATE]

# measured on the CPU over REGULAR + the random case (the figures of the docstring below), asserted at 4x
MEASURED_STAT_REL = 4.96e-8
MEASURED_VOXEL_ABS = 3.16e-6


def torch_transform(item, f, k):
    """the reference's item transform written with torch in fp32: flips, NormalizeIntensity over != 0, pad at the far end"""
    img = item
    for bit, ax in ((1, 1), (2, 2), (4, 3)):
        if f & bit:
            img = torch.flip(img, dims=[ax])
    sel = img != 0
    mean, std = img[sel].mean(), img[sel].std()
    img = (img - mean) / (std + 1e-5)
    _, d, h, w = img.shape
    return F.pad(img, (0, (k - w % k) % k, 0, (k - h % k) % k, 0, (k - d % k) % k)), mean, std


def _flips(name, n):
    return [V.FLIP_PAIRS[(2 + i) % 8][i % 2] for i in range(n)]


def test_fp64_statements_agree_with_torch_fp32():
    """Measured here (torch CPU, fp32, its own summation order) against the fp64 statements, largest over the regular cases and the
    random case: mean / std relative difference 4.96e-8 (130^3; the 1000 +- 5 samples 3.2e-8, random data 1.5e-8), normalised
    voxels |dy| / max(1, |y|) 3.16e-6 (the 1000 +- 5 sample of "flips", |y| <= 312: an fp32 mean of 1000 is off by ~1e-5 of a std
    of 3; everywhere else <= 1.4e-7 at |y| <= 4, the constant sample 1.2e-16 at |y| = 5e5).  Asserted at 4x those figures; the
    degenerate cases must put NaN in the same places."""
    worst_stat, worst_vox = 0.0, 0.0
    sets = [(n, V.build(n), V.CASES[n][1]) for n in V.CASES] + [("random", V.build_random(), 16)]
    for name, x, k in sets:
        pads = V.padded(x.shape, k)
        flips = _flips(name, x.shape[0])
        s64 = V.stats64(x)
        y64 = V.prepare64(x, s64, flips, pads)
        for n in range(x.shape[0]):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                            # torch: std() of fewer than two values
                yt, mean, std = torch_transform(torch.from_numpy(x[n].copy()), flips[n], k)
            yt = yt.numpy().astype(np.float64)
            assert yt.shape == y64[n].shape
            if name in V.DEGENERATE:
                assert np.array_equal(np.isnan(yt), np.isnan(y64[n])) and np.isnan(yt).sum() == x[n].size
                assert np.isnan(float(std)) and np.isnan(s64[n, 2]) and np.isnan(float(mean)) == np.isnan(s64[n, 1])
                continue
            rel = max(abs(float(mean) - s64[n, 1]) / abs(s64[n, 1]), abs(float(std) - s64[n, 2]) / (s64[n, 2] or 1.0))
            vox = float((np.abs(yt - y64[n]) / np.maximum(1.0, np.abs(y64[n]))).max())
            print(f"{name}[{n}] stat rel {rel:.2e} voxel abs {vox:.2e} max|y| {np.abs(y64[n]).max():.1f}")
            worst_stat, worst_vox = max(worst_stat, rel), max(worst_vox, vox)
    print(f"worst: stat rel {worst_stat:.2e} voxel abs {worst_vox:.2e}")
    assert worst_stat <= 4 * MEASURED_STAT_REL and worst_vox <= 4 * MEASURED_VOXEL_ABS


@pytest.mark.parametrize("name", list(V.CASES))
def test_integer_cases_have_exact_sums_and_carry_their_plants(name):
    x = V.build(name)
    shape, k = V.CASES[name]
    assert x.dtype == np.float32 and x.shape == shape and k % 8 == 0
    assert np.array_equal(x, V.build(name))                               # deterministic
    exact = V.exact_stats64(x)
    two_pass = V.stats64(x)
    for n in range(shape[0]):
        cnt, S, Q = V.integer_sums(x[n])                                  # asserts integers, |x| <= 2048, <= 2^22 voxels
        assert Q < 2 ** 53 and abs(S) < 2 ** 53 and x[n].size * V.VMAX ** 2 < 2 ** 53
        # fp64 sums in two different orders are the integers themselves
        v = x[n][x[n] != 0].astype(np.float64)
        for order in (v, v[::-1], np.sort(v)):
            assert float(np.cumsum(order)[-1]) == S and float(np.cumsum(order * order)[-1]) == Q if cnt else True
        if name in V.DEGENERATE:
            assert cnt < 2 and np.isnan(exact[n, 2]) and np.isnan(exact[n, 3])
            continue
        assert np.allclose(exact[n], two_pass[n], rtol=1e-12, atol=0)     # the rational value and the two-pass fp64 statement
        zeros = (x[n] == 0).mean()
        assert 0.25 < zeros < 0.35, zeros
        assert np.signbit(x[n][x[n] == 0]).any() and not np.signbit(x[n][x[n] == 0]).all()   # both zeros occur
    if name in ("pads", "flips"):
        cnt, S, Q = V.integer_sums(x[-1])
        assert (cnt * Q + S * S) / (cnt * Q - S * S) > 1e4               # the cancellation the comparer's bound has to carry
    if name == "big":
        assert x.size > 128 * 256 * 16                                    # more voxels than one pass of the widest grid
    if name == "pads":
        assert x[0].size % 4 == 2 and V.build_mask(name)[0].size % 2 == 1  # sample 1 starts off 16 bytes; its mask at an odd byte


def test_the_case_list_covers_what_it_must():
    assert V.padded(*V.CASES["ref37"]) == (48, 48, 64)
    assert V.padded(*V.CASES["nopad"]) == V.CASES["nopad"][0][2:]
    assert V.padded(*V.CASES["pads"]) == (16, 16, 32)
    assert sorted({a for a, _ in V.FLIP_PAIRS}) == list(range(8)) and all(a != b for a, b in V.FLIP_PAIRS)
    assert sorted({b for _, b in V.FLIP_PAIRS}) == list(range(8))
    for name, (N, n_per) in V.LABEL_CASES.items():
        p, t = V.build_labels(name)
        assert p.shape == t.shape == (N, n_per) and p.dtype == t.dtype == np.uint8
    assert 255 * 255 * V.LABEL_CASES["wrap"][1] > 2 ** 32 and V.LABEL_CASES["tiny"][1] % 2 == 1
    assert V.dice64(V.label_sums(*V.build_labels("zero"))) == 1.0
    p, t = V.build_labels("random")
    pt, tt = torch.from_numpy(p).float().double(), torch.from_numpy(t).float().double()
    assert abs(V.dice64(V.label_sums(p, t)) - float((2. * (pt * tt).sum() + 1e-6) / (pt.sum() + tt.sum() + 1e-6))) < 1e-15


@pytest.mark.parametrize("name", ["flips", "pads", "k8", "ref37"])
def test_restore_inverts_prepare_for_all_eight_flip_masks(name):
    shape, k = V.CASES[name]
    pads = V.padded(shape, k)
    mask = V.build_mask(name)
    x = V.build(name)
    for f in range(8):
        flips = [f, 7 - f][:shape[0]]
        assert np.array_equal(V.restore(V.prepare_mask(mask, flips, pads), flips, shape[2:]), mask)
        y = V.prepare64(x, None, flips, pads)
        for c in range(shape[1]):
            assert np.array_equal(V.restore(y[:, c], flips, shape[2:]), x[:, c].astype(np.float64))
        if f:
            assert not np.array_equal(V.prepare_mask(mask, flips, pads), V.prepare_mask(mask, None, pads))


def _differs(a, b, floor):
    """largest difference between two prepared volumes, NaN-safe; must exceed `floor` to count as told apart"""
    with np.errstate(all="ignore"):
        d = np.abs(a - b)
    return float(np.nanmax(d)) > floor


def test_each_stated_mutant_is_told_apart_by_some_case():
    """the GPU test allows 1 fp32 ulp: a mutant counts as caught only where it moves a voxel by far more (1e-3 absolute at |y| of
    order 1, ~1e4 ulp)"""
    floor = 1e-3
    caught = {m: [] for m in ("biased", "eps_under_root", "bit_test", "pad-norm", "pad-flip", "per_channel")}
    for name in REGULAR:
        x = V.build(name)
        shape, k = V.CASES[name]
        pads = V.padded(shape, k)
        flips = [5, 3][:shape[0]]
        s = V.stats64(x)
        good = V.prepare64(x, s, flips, pads)
        for m in ("biased", "eps_under_root", "bit_test"):
            if _differs(V.prepare64(x, V.stats64(x, **{m: True}), flips, pads), good, floor):
                caught[m].append(name)
        for m in ("pad-norm", "pad-flip"):
            if _differs(V.prepare64(x, s, flips, pads, order=m), good, floor):
                caught[m].append(name)
        if _differs(V.prepare64(x, V.stats64(x, per_channel=True), flips, pads), good, floor):
            caught["per_channel"].append(name)
    print(caught)
    for m, names in caught.items():
        assert names, f"no case tells the mutant {m} apart"
    assert "nopad" not in caught["pad-norm"] and "nopad" not in caught["pad-flip"]       # nothing to pad there: the check is not vacuous
    assert caught["per_channel"] == ["pads"]                                              # the only case with two channels
    # the bit-test mutant on the statistics themselves: -0.0 would be counted
    x = V.build("k8")
    assert V.stats64(x, bit_test=True)[0, 0] > V.stats64(x)[0, 0]


def test_volume_symbols_are_declared_with_citations_bound_and_exported_with_abi_54():
    from semantic_segmentation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gsseg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in gsseg.h"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype in _lib.py"
    assert int(re.search(r"#define GS_ABI_VERSION (\d+)", hdr).group(1)) == 54 == _lib.ABI_VERSION
    for cite in ("GenSeg-3D/transforms.py", "transforms.py:25-29", "transforms.py:42-43", ":47-60", "train_unet.py:46-47",
                 "train_unet.py:39"):
        assert cite in hdr, cite
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.gs_abi_version() == 54
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.gs_volume_stats_ws_doubles(3) >= 3 * 3 and lib.gs_label_sums_ws_int64(3) >= 3 * 3
    assert lib.gs_volume_stats_ws_doubles(0) == 0 == lib.gs_label_sums_ws_int64(-1)


def test_volume_entry_points_refuse_bad_arguments_before_any_device_work():
    """the pointers are never dereferenced (fake, aligned addresses): a launch would fault, a refusal returns GS_EINVAL with the
    entry point's own name in the message"""
    from semantic_segmentation_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    fake = 1 << 20

    def refused(name, *args):
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert name.encode() in lib.gs_last_error(), lib.gs_last_error()

    # statistics: NULL, non-positive sizes, alignment
    for a in ((None, 1, 8, fake, fake), (fake, 1, 8, None, fake), (fake, 1, 8, fake, None), (fake, 0, 8, fake, fake),
              (fake, 1, 0, fake, fake), (fake, -2, 8, fake, fake), (fake + 2, 1, 8, fake, fake), (fake, 1, 8, fake + 4, fake)):
        refused("gs_volume_nonzero_stats", *a, None)
    # prepare: NULL x / out, one of mask / mask_out, non-positive dims, Dp < D and the like, padded dims off 8, unaligned outputs
    ok = dict(x=fake, mask=None, stats=None, flips=None, out=fake, mask_out=None, N=1, C=1, D=5, H=6, W=7, Dp=8, Hp=8, Wp=8)
    bad = [dict(x=None), dict(out=None), dict(mask=fake), dict(mask_out=fake), dict(N=0), dict(C=0), dict(D=0), dict(H=-1), dict(W=0),
           dict(Dp=4), dict(Hp=5), dict(Wp=6), dict(D=9), dict(H=9), dict(W=9), dict(Dp=12), dict(Hp=20), dict(Wp=12), dict(out=fake + 4),
           dict(out=fake + 8), dict(mask=fake, mask_out=fake + 8), dict(N=70000)]
    for b in bad:
        a = dict(ok, **b)
        refused("gs_volume_prepare", *a.values(), None)
    # restore
    ok = dict(lab=fake, flips=None, out=fake, N=1, D=5, H=6, W=7, Dp=8, Hp=8, Wp=8)
    for b in (dict(lab=None), dict(out=None), dict(N=0), dict(D=0), dict(H=0), dict(W=-3), dict(Dp=4), dict(D=9), dict(H=9), dict(W=9),
              dict(Dp=12), dict(Hp=9), dict(Wp=10), dict(lab=fake + 8)):
        a = dict(ok, **b)
        refused("gs_volume_restore_labels", *a.values(), None)
    # label sums: NULL, non-positive sizes, maps that do not share their offset within 16 bytes
    for a in ((None, fake, 1, 9, fake, fake), (fake, None, 1, 9, fake, fake), (fake, fake, 1, 9, None, fake), (fake, fake, 1, 9, fake, None),
              (fake, fake, 0, 9, fake, fake), (fake, fake, 1, 0, fake, fake), (fake, fake + 3, 1, 9, fake, fake)):
        refused("gs_label_sums", *a, None, 1e-6, None)


def test_host_wrappers_refuse_cpu_tensors_and_bad_settings():
    from semantic_segmentation_amd.volume import VolumePrep, label_dice, volume_stats
    x = torch.zeros(1, 1, 3, 5, 7)
    with pytest.raises(RuntimeError):
        VolumePrep().prepare(x)
    with pytest.raises(RuntimeError):
        volume_stats(x)
    with pytest.raises(RuntimeError):
        label_dice(torch.zeros(1, 9, dtype=torch.uint8), torch.zeros(1, 9, dtype=torch.uint8))
    for k in (0, 4, 12, -8):
        with pytest.raises(ValueError):
            VolumePrep(k=k)
    assert VolumePrep(k=24).k == 24
    a, b = VolumePrep(flip_prob=0.5, seed=3).draw_flips(64), VolumePrep(flip_prob=0.5, seed=3).draw_flips(64)
    assert np.array_equal(a, b) and a.dtype == np.int32 and set(a.tolist()) <= set(range(8)) and len(set(a.tolist())) > 4
