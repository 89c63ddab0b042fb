"""csrc/volume.hip on the MI355X against tests/volume_reference.py: the statistics against the exact rational value inside a bound
counted from the kernel's formula, the prepared volume within 1 fp32 ulp (pad voxels exactly +0.0, the geometry bit-exact on an
index volume, every mask byte), restore byte for byte for every flip mask and shape, the label sums equal to numpy's integers."""
import numpy as np
import pytest
import torch

from tests import volume_reference as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_cache = {}


def case(name):
    """(x fp32 numpy, the same on the device), built once and never written"""
    if name not in _cache:
        x = V.build(name)
        x.setflags(write=False)
        _cache[name] = (x, torch.from_numpy(x.copy()).to(DEV))
    return _cache[name]


def raw_prepare(x, mask, stats, flips, pads):
    """gs_volume_prepare through the binding, with host-supplied stats / flips"""
    from semantic_segmentation_amd import _lib
    from semantic_segmentation_amd.ops import _stream
    n, c, d, h, w = x.shape
    out = torch.full((n, c) + tuple(pads), 7.0, dtype=torch.float32, device=DEV)            # poisoned: every voxel must be written
    mout = torch.full((n,) + tuple(pads), 77, dtype=torch.uint8, device=DEV) if mask is not None else None
    st = torch.from_numpy(np.ascontiguousarray(stats)).to(DEV) if stats is not None else None
    fl = torch.tensor(list(flips), dtype=torch.int32, device=DEV) if flips is not None else None
    _lib.call("gs_volume_prepare", x.data_ptr(), mask.data_ptr() if mask is not None else None, st.data_ptr() if st is not None else None,
              fl.data_ptr() if fl is not None else None, out.data_ptr(), mout.data_ptr() if mout is not None else None,
              n, c, d, h, w, *pads, _stream())
    return out.cpu().numpy(), (mout.cpu().numpy() if mout is not None else None)


def flips_of(name):
    n = V.CASES[name][0][0]
    return [V.FLIP_PAIRS[(3 + i) % 8][i % 2] for i in range(n)] if name != "flips" else None


@pytest.mark.parametrize("name", list(V.CASES))
def test_stats_meet_the_exact_value_inside_the_counted_bound_and_repeat_bit_for_bit(name):
    from semantic_segmentation_amd.volume import volume_stats
    x, xd = case(name)
    a = volume_stats(xd)
    b = volume_stats(xd)
    torch.cuda.synchronize()
    got = a.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (x.shape[0], 4)
    assert np.array_equal(got.view(np.uint64), b.cpu().numpy().view(np.uint64)), "two runs differ"
    for row in V.check_stats_exact(got, x):
        print(name, "count %d  mean %.2e <= %.2e  std %.2e <= %.2e  inv %.2e <= %.2e" % row)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_stats_of_samples_that_start_at_any_element(offset):
    """a view that starts `offset` floats into its allocation: peeled heads of 3, 2 and 1 elements, and a tail"""
    from semantic_segmentation_amd.volume import volume_stats
    x, _ = case("pads")
    n, per = x.shape[0], x[0].size
    buf = torch.zeros(offset + n * per + 8, dtype=torch.float32, device=DEV)
    buf[:offset] = 123.0                                           # neighbours that must not be read
    buf[offset + n * per:] = 321.0
    view = buf[offset:offset + n * per].view(n, per)
    view.copy_(torch.from_numpy(x.reshape(n, per).copy()))
    assert view.data_ptr() % 16 == 4 * offset
    V.check_stats_exact(volume_stats(view).cpu().numpy(), x)


def test_stats_of_non_integer_voxels_inside_the_summation_bound():
    from semantic_segmentation_amd.volume import volume_stats
    x = V.build_random()
    got = volume_stats(torch.from_numpy(x).to(DEV)).cpu().numpy()
    want = V.stats64(x)
    for n in range(x.shape[0]):
        bm, bs = V.random_stats_bounds(x[n])
        bm += 8 * V.U * abs(want[n, 1])                            # the fp64 statement's own roundings
        bs += 8 * V.U * want[n, 2] + x[n].size * V.U * want[n, 2]  # its two-pass sum of squares, worst case
        print("random", n, abs(got[n, 1] - want[n, 1]), bm, abs(got[n, 2] - want[n, 2]), bs)
        assert got[n, 0] == want[n, 0]
        assert abs(got[n, 1] - want[n, 1]) <= bm and abs(got[n, 2] - want[n, 2]) <= bs
        assert abs(got[n, 3] - 1.0 / (got[n, 2] + 1e-5)) <= 2 * V.U * got[n, 3]


@pytest.mark.parametrize("name", list(V.CASES))
def test_prepare_with_host_stats_is_within_one_ulp_and_pads_with_plus_zero(name):
    x, xd = case(name)
    shape, k = V.CASES[name]
    pads = V.padded(shape, k)
    stats = V.exact_stats64(x)
    mask = V.build_mask(name)
    md = torch.from_numpy(mask).to(DEV)
    runs = [flips_of(name)] if name != "flips" else [list(p) for p in V.FLIP_PAIRS]
    if name in ("k8", "pads"):
        runs.append(None)                                          # flips == NULL
    for flips in runs:
        got, gm = raw_prepare(xd, md, stats, flips, pads)
        worst = V.check_prepared(got, x, stats, flips, pads)
        print(name, flips, "worst ulp distance", worst)
        assert np.array_equal(gm, V.prepare_mask(mask, flips, pads)), "mask bytes"


@pytest.mark.parametrize("name", ["ref37", "pads", "k8", "flips", "nopad"])
def test_prepare_without_stats_moves_an_index_volume_bit_exactly(name):
    shape, k = V.CASES[name]
    pads = V.padded(shape, k)
    x = np.arange(1, int(np.prod(shape)) + 1, dtype=np.float32).reshape(shape)       # linear index + 1 < 2^24: 0 marks the padding only
    assert x.max() < 2 ** 24
    xd = torch.from_numpy(x).to(DEV)
    for flips in ([list(p) for p in V.FLIP_PAIRS] if shape[0] == 2 else [[f] for f in range(8)]):
        got, gm = raw_prepare(xd, None, None, flips, pads)
        assert gm is None
        want = V.prepare64(x, None, flips, pads).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, flips)


@pytest.mark.parametrize("name", list(V.CASES))
def test_prepare_chained_on_the_kernels_own_stats(name):
    """VolumePrep.prepare: statistics and apply on the device, nothing in between; 1 ulp plus the statistics' bound carried through
    y = (x - mean) inv"""
    from semantic_segmentation_amd.volume import VolumePrep
    x, xd = case(name)
    shape, k = V.CASES[name]
    pads = V.padded(shape, k)
    flips = flips_of(name) if name != "flips" else list(V.FLIP_PAIRS[5])
    mask = V.build_mask(name)
    out, mout, meta = VolumePrep(k=k).prepare(xd, torch.from_numpy(mask).to(DEV), flips=flips)
    assert tuple(out.shape) == shape[:2] + pads and meta.shape == shape and meta.padded == pads
    stats = V.exact_stats64(x)
    extra = []
    for n in range(shape[0]):
        bm, _, bi = V.stats_bounds(*V.integer_sums(x[n]))
        extra.append(V.propagated(stats[n, 1], stats[n, 3], bm, bi))
    V.check_prepared(out.cpu().numpy(), x, stats, flips, pads, extra=extra)
    V.check_stats_exact(meta.stats.cpu().numpy(), x)
    assert np.array_equal(mout.cpu().numpy(), V.prepare_mask(mask, flips, pads))
    if name in V.DEGENERATE:
        got = out.cpu().numpy()
        assert np.isnan(got[:, :, :shape[2], :shape[3], :shape[4]]).all() and np.count_nonzero(np.isnan(got)) == x.size


def test_prepare_accepts_every_documented_rank_and_integer_masks():
    from semantic_segmentation_amd.volume import VolumePrep
    x, xd = case("k8")
    mask = V.build_mask("k8")
    prep = VolumePrep(k=8, normalize=False)
    want = V.prepare64(x, None, None, (8, 8, 8)).astype(np.float32)
    for xi, mi in ((xd[0, 0], torch.from_numpy(mask[0].astype(np.int64)).to(DEV)), (xd[0], torch.from_numpy(mask).to(DEV)),
                   (xd, torch.from_numpy(mask[:, None].astype(np.int32)).to(DEV))):
        out, mout, meta = prep.prepare(xi, mi)
        assert meta.ndim == xi.dim() and meta.flips is None and meta.stats is None
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(mout.cpu().numpy(), V.prepare_mask(mask, None, (8, 8, 8)))
    with pytest.raises(RuntimeError):
        prep.prepare(torch.from_numpy(x.copy()))
    with pytest.raises(ValueError):
        VolumePrep(k=12)


def test_drawn_flips_follow_the_seed_and_the_probability():
    from semantic_segmentation_amd.volume import VolumePrep
    _, xd = case("flips")
    a = VolumePrep(flip_prob=0.5, seed=11).prepare(xd)[2].flips.cpu().numpy()
    b = VolumePrep(flip_prob=0.5, seed=11).prepare(xd)[2].flips.cpu().numpy()
    want = (np.random.default_rng(11).random((2, 3)) < 0.5) @ np.array([1, 2, 4])
    assert a.dtype == np.int32 and np.array_equal(a, b) and np.array_equal(a, want)
    assert VolumePrep(flip_prob=1.0).prepare(xd)[2].flips.cpu().tolist() == [7, 7]
    assert VolumePrep(flip_prob=0.0).prepare(xd)[2].flips is None


@pytest.mark.parametrize("name", list(V.CASES))
def test_restore_is_exact_for_every_flip_mask(name):
    from semantic_segmentation_amd.volume import VolumeMeta, VolumePrep
    shape, k = V.CASES[name]
    pads = V.padded(shape, k)
    n = shape[0]
    lab = V.rng_of(name + "/lab").integers(0, 256, size=(n,) + pads).astype(np.uint8)
    ld = torch.from_numpy(lab).to(DEV)
    prep = VolumePrep(k=k)
    runs = [list(p) for p in V.FLIP_PAIRS] if n == 2 else [[f] for f in range(8)]
    for flips in runs + [None]:
        fl = torch.tensor(flips, dtype=torch.int32, device=DEV) if flips is not None else None
        out = prep.restore(ld, VolumeMeta(shape, pads, fl, None, 5))
        assert out.dtype == torch.uint8 and tuple(out.shape) == (n,) + shape[2:]
        assert np.array_equal(out.cpu().numpy(), V.restore(lab, flips, shape[2:])), (name, flips)


def test_restore_inverts_prepare_on_the_device():
    from semantic_segmentation_amd.volume import VolumePrep
    mask = V.build_mask("flips")
    _, xd = case("flips")
    prep = VolumePrep()
    for flips in V.FLIP_PAIRS:
        _, mout, meta = prep.prepare(xd, torch.from_numpy(mask).to(DEV), flips=list(flips))
        assert np.array_equal(prep.restore(mout, meta).cpu().numpy(), mask)


@pytest.mark.parametrize("name", list(V.LABEL_CASES))
def test_label_sums_equal_numpy_and_dice_is_within_one_ulp(name):
    from semantic_segmentation_amd.volume import label_dice, label_sums
    p, t = V.build_labels(name)
    sums, dice = label_sums(torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV))
    want = V.label_sums(p, t)
    got = sums.cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    d64 = V.dice64(want)
    assert dice.dtype == torch.float32 and dice.dim() == 0
    assert abs(int(V.ordered(dice.cpu().numpy().reshape(1))[0]) - int(V.ordered(np.array([d64], dtype=np.float32))[0])) <= 1
    if name == "zero":
        assert float(dice) == 1.0
    if name == "wrap":
        assert want[0, 0] == 255 * 255 * 48 ** 3 > 2 ** 32
    # class-index targets of another integer type, and the public label_dice
    d2 = label_dice(torch.from_numpy(p).to(DEV), torch.from_numpy(t.astype(np.int64)).to(DEV))
    assert float(d2) == float(dice)


def test_label_sums_of_maps_that_start_at_any_byte():
    from semantic_segmentation_amd.volume import label_sums
    p, t = V.build_labels("tiny")
    for off in (1, 7, 15):
        bp = torch.zeros(p.size + 32, dtype=torch.uint8, device=DEV) + 9
        bt = torch.zeros(p.size + 32, dtype=torch.uint8, device=DEV) + 9
        vp, vt = bp[off:off + p.size].view(p.shape), bt[off:off + p.size].view(p.shape)
        vp.copy_(torch.from_numpy(p))
        vt.copy_(torch.from_numpy(t))
        assert np.array_equal(label_sums(vp, vt)[0].cpu().numpy(), V.label_sums(p, t))
    # different offsets: the wrapper re-bases them, the entry point itself refuses
    vt2 = bt[3:3 + p.size].view(p.shape)
    vt2.copy_(torch.from_numpy(t))
    assert np.array_equal(label_sums(vp, vt2)[0].cpu().numpy(), V.label_sums(p, t))
