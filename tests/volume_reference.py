"""The volume transform in front of UNet3D and the label Dice behind it (csrc/volume.hip: gs_volume_nonzero_stats, gs_volume_prepare,
gs_volume_restore_labels, gs_label_sums) stated in numpy fp64 and exact rational arithmetic, with the case lists and the comparers
of the CPU and GPU tests.  No GPU, no native library.

  stats     over the voxels with x != 0 (IEEE compare: -0.0 out, all channels of a sample together):  n, mean = S / n,
            std = sqrt((n Q - S^2) / (n (n - 1))) (unbiased), inv = 1 / (std + 1e-5);  n == 0: mean NaN, n < 2: std NaN
  prepare   y[n,c,d,h,w] = float32((x[n,c,fd(d),fh(h),fw(w)] - mean_n) inv_n) inside the extent (flip, then normalise), +0.0 in the
            padding, which lies at the far end only (pad AFTER normalising);  flips[n] bit 0 / 1 / 2 mirrors D / H / W
  restore   out[n,d,h,w] = lab[n,fd(d),fh(h),fw(w)] over the original extent
  sums      I = sum p t, P = sum p, T = sum t per sample in integers;  dice = (2 sum I + eps) / (sum P + sum T + eps) in fp64

Integer cases: integer-valued voxels with |x| <= 2048 and at most 2^22 of them, so S (< 2^33) and Q (< 2^44 < 2^53) are exact in
fp64 in ANY order, and the expected statistics come from the integer sums with no rounding at all (fractions.Fraction, the root in
60-digit decimal).  Planted: 30 % exact zeros, a fifth of them -0.0; samples of 1000 +- 5 (mean large against the spread: the
cancellation in n Q - S^2); a two-channel sample whose channels differ (one statistic must cover both).

The comparer of the statistics counts roundings for the formula THE KERNEL USES, var = (n Q - S^2) / (n (n - 1)) in fp64 from exact
n, S, Q: fl(n Q), fl(S^2) and their difference give u (n Q + S^2) / (n Q - S^2) + u relative (u = 2^-53; a fused multiply-subtract
only removes one of them), n (n - 1) is exact below 2^53, the quotient adds u, the root halves the sum and adds u, std + 1e-5 and
the reciprocal add u each."""
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
VMAX = 2048
MAX_VOXELS = 1 << 22

# name -> ((N, C, D, H, W), k)
CASES = {
    "ref37": ((1, 1, 37, 36, 57), 16),      # the reference's own example (transforms.py:113) -> 48 x 48 x 64
    "pads": ((2, 2, 5, 9, 17), 16),         # largest pads, two channels share one statistic, odd W, the second mask starts at an odd byte
    "nopad": ((1, 1, 16, 32, 48), 16),      # no padding at all
    "k8": ((1, 1, 3, 5, 7), 8),
    "one": ((1, 1, 1, 1, 1), 16),           # count == 1: std NaN
    "two": ((1, 1, 2, 1, 1), 16),           # one zero: count == 1
    "none": ((1, 1, 1, 1, 2), 8),           # 0.0 and -0.0: count == 0, mean NaN
    "big": ((1, 1, 130, 130, 130), 8),      # many blocks per sample in the reduction
    "flips": ((2, 1, 6, 10, 19), 16),       # all eight flip masks, a different one per sample
    "const": ((1, 1, 4, 6, 9), 8),          # every non-zero voxel is 5: std == 0 exactly, inv = 1 / 1e-5 (where the 1e-5 is added shows)
}
DEGENERATE = ("one", "two", "none")
FLIP_PAIRS = [(a, (a * 3 + 5) % 8) for a in range(8)]            # every mask on sample 0; sample 1 gets another one each time


def padded(shape, k):
    return tuple(-(-v // k) * k for v in shape[2:])


def rng_of(name):
    return np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(str(name))))


def build(name):
    """fp32 [N, C, D, H, W] of the integer case `name`"""
    shape, _ = CASES[name]
    if name == "one":
        return np.full(shape, 7.0, dtype=np.float32)
    if name == "two":
        return np.array([3.0, 0.0], dtype=np.float32).reshape(shape)
    if name == "none":
        return np.array([0.0, -0.0], dtype=np.float32).reshape(shape)
    g = rng_of(name)
    x = g.integers(-VMAX, VMAX + 1, size=shape).astype(np.float32)
    if name == "const":
        x[:] = 5.0
    if name in ("pads", "flips"):
        x[-1] = 1000 + g.integers(-5, 6, size=shape[1:])              # mean large against the spread
    if name == "pads":
        x[0, 1] = 1500 + g.integers(-5, 6, size=shape[2:])            # the channels of sample 0 differ: one statistic over both
    r = g.random(shape)
    x[r < 0.3] = 0.0
    x[r < 0.06] = -0.0
    return x


def build_mask(name, classes=9):
    shape, _ = CASES[name]
    return rng_of(name + "/mask").integers(0, classes, size=(shape[0],) + shape[2:]).astype(np.uint8)


def build_random(shape=(2, 1, 9, 11, 13)):
    """the non-integer case: normal voxels with an offset, zeros planted"""
    g = rng_of("random")
    x = (g.standard_normal(shape) * 3.0 + 2.0).astype(np.float32)
    x[g.random(shape) < 0.3] = 0.0
    return x


# ------------------------------------------------------------------------------------------------ statistics
def selected(x, bit_test=False):
    """boolean selection of the voxels that count; the bit-test mutant also takes -0.0"""
    if bit_test:
        return x.view(np.uint32) != 0
    return x != 0


def integer_sums(xs):
    """exact (n, S, Q) of one sample of integer-valued voxels"""
    v = xs[xs != 0]
    assert np.array_equal(v, np.round(v)) and (np.abs(v) <= VMAX).all() and xs.size <= MAX_VOXELS
    i = v.astype(np.int64)
    return int(i.size), int(i.sum()), int((i * i).sum())


def exact_stats(n, S, Q):
    """(mean, std) as (Fraction, Decimal) from the integer sums; None where the reference gives NaN"""
    getcontext().prec = 60
    mean = Fraction(S, n) if n > 0 else None
    if n < 2:
        return mean, None
    var = Fraction(n * Q - S * S, n * (n - 1))
    return mean, (Decimal(var.numerator) / Decimal(var.denominator)).sqrt()


def stats_bounds(n, S, Q):
    """relative bounds (mean, std, inv) for the kernel's formula on exact n, S, Q (module docstring); first-order count + 1 u slack"""
    if n < 2 or n * Q == S * S:
        return 2 * U, 2 * U, 4 * U                                  # n Q == S^2: the difference is exactly 0, inv = 1 / fl(1e-5)
    cancel = (n * Q + S * S) / (n * Q - S * S)
    var = U * cancel + 2 * U
    std = var / 2 + U
    return 2 * U, std + U, std + 3 * U


def stats64(x, biased=False, eps_under_root=False, bit_test=False, per_channel=False):
    """fp64 [N, 4] = count, mean, std, inv: the two-pass (well-conditioned) statement.  The keyword arguments are the mutants.
    per_channel returns [N, C, 4]."""
    if per_channel:
        return np.stack([stats64(np.ascontiguousarray(x[:, c:c + 1]), biased, eps_under_root, bit_test) for c in range(x.shape[1])], 1)
    out = np.empty((x.shape[0], 4))
    with np.errstate(all="ignore"):
        for n in range(x.shape[0]):
            xs = np.ascontiguousarray(x[n])
            v = xs[selected(xs, bit_test)].astype(np.float64)
            cnt = v.size
            mean = v.sum() / cnt if cnt else np.nan
            den = cnt if biased else cnt - 1
            var = ((v - mean) ** 2).sum() / den if den > 0 else np.nan
            if eps_under_root:
                std = np.sqrt(var + 1e-5)
                inv = 1.0 / std
            else:
                std = np.sqrt(var)
                inv = 1.0 / (std + 1e-5)
            out[n] = (cnt, mean, std, inv)
    return out


def exact_stats64(x):
    """fp64 [N, 4] rounded once from the exact rational values of an integer case"""
    out = np.empty((x.shape[0], 4))
    for n in range(x.shape[0]):
        cnt, S, Q = integer_sums(x[n])
        mean, std = exact_stats(cnt, S, Q)
        out[n, 0] = cnt
        out[n, 1] = float(mean) if mean is not None else np.nan
        out[n, 2] = float(std) if std is not None else np.nan
        out[n, 3] = float(1 / (std + Decimal("1e-5"))) if std is not None else np.nan
    return out


def rel_err(got, want):
    """|got - want| / |want| with want a Fraction or Decimal and got an fp64 (converted exactly)"""
    if isinstance(want, Fraction):
        g = Fraction(float(got))
        return float(abs(g - want) / abs(want)) if want != 0 else float(abs(g))
    g = Decimal(float(got))
    return float(abs(g - want) / abs(want)) if want != 0 else float(abs(g))


def check_stats_exact(got, x):
    """got fp64 [N, 4] from the kernel on an integer case: count exact, mean / std / inv inside the counted bounds.
    -> list of (count, mean_err, mean_bound, std_err, std_bound, inv_err, inv_bound) per sample, for printing"""
    rows = []
    for n in range(x.shape[0]):
        cnt, S, Q = integer_sums(x[n])
        mean, std = exact_stats(cnt, S, Q)
        bm, bs, bi = stats_bounds(cnt, S, Q)
        assert got[n, 0] == cnt, (n, got[n, 0], cnt)
        if mean is None:
            assert np.isnan(got[n, 1])
            em = 0.0
        else:
            em = rel_err(got[n, 1], mean)
            assert em <= bm, (n, "mean", em, bm)
        if std is None:
            assert np.isnan(got[n, 2]) and np.isnan(got[n, 3]), (n, got[n])
            es = ei = 0.0
        else:
            es = rel_err(got[n, 2], std)
            ei = rel_err(got[n, 3], 1 / (std + Decimal("1e-5")))
            if std == 0:                                        # a constant sample: n Q == S^2 exactly, the kernel's difference is 0
                assert got[n, 2] == 0.0
            else:
                assert es <= bs, (n, "std", es, bs)
            assert ei <= bi, (n, "inv", ei, bi)
        rows.append((cnt, em, bm, es, bs, ei, bi))
    return rows


def random_stats_bounds(xs):
    """absolute bounds (mean, std) for fp64 sums of a NON-integer sample in any order: |dS| <= n u sum|x|, |dQ| <= n u Q (worst case
    of recursive summation), carried through mean = S / n and var = (n Q - S^2) / (n (n - 1)) with the formula's own roundings"""
    v = xs[xs != 0].astype(np.float64)
    n = v.size
    A, S, Q = np.abs(v).sum(), v.sum(), (v * v).sum()
    dS, dQ = n * U * A, n * U * Q
    mean_abs = dS / n + 2 * U * abs(S / n)
    num = n * Q - S * S
    dnum = n * dQ + 2 * abs(S) * dS + 3 * U * (n * Q + S * S)
    var = num / (n * (n - 1.0))
    dvar = dnum / (n * (n - 1.0)) + 2 * U * var
    std = np.sqrt(var)
    return mean_abs, dvar / (2 * std) + 2 * U * std


# ------------------------------------------------------------------------------------------------ geometry
def flip_item(v, f, axes=(-3, -2, -1)):
    for bit, ax in zip((1, 2, 4), axes):
        if f & bit:
            v = np.flip(v, ax)
    return v


def prepare64(x, stats, flips, pads, order="flip-norm-pad"):
    """fp64 [N, C, Dp, Hp, Wp].  stats None: no normalisation.  order names the mutants: "pad-norm" normalises the padded
    volume (pad voxels become (0 - mean) inv), "pad-flip" flips the padded volume (the padding moves to the near end)."""
    N, C, D, H, W = x.shape
    Dp, Hp, Wp = pads
    out = np.zeros((N, C, Dp, Hp, Wp))
    for n in range(N):
        f = int(flips[n]) if flips is not None else 0
        v = x[n].astype(np.float64)
        if stats is not None:
            s = stats[n]
            mean, inv = (s[..., 1], s[..., 3])
            if np.ndim(mean):                                    # per-channel mutant
                mean, inv = mean.reshape(C, 1, 1, 1), inv.reshape(C, 1, 1, 1)
        if order == "flip-norm-pad":
            v = flip_item(v, f)
            if stats is not None:
                with np.errstate(all="ignore"):
                    v = (v - mean) * inv
            out[n, :, :D, :H, :W] = v
        elif order == "pad-norm":
            out[n, :, :D, :H, :W] = flip_item(v, f)
            with np.errstate(all="ignore"):
                out[n] = (out[n] - mean) * inv
        elif order == "pad-flip":
            with np.errstate(all="ignore"):
                out[n, :, :D, :H, :W] = (v - mean) * inv if stats is not None else v
            out[n] = flip_item(out[n], f)
        else:
            raise ValueError(order)
    return out


def prepare_mask(mask, flips, pads):
    N, D, H, W = mask.shape
    out = np.zeros((N,) + tuple(pads), dtype=np.uint8)
    for n in range(N):
        out[n, :D, :H, :W] = flip_item(mask[n], int(flips[n]) if flips is not None else 0)
    return out


def restore(lab, flips, dhw):
    D, H, W = dhw
    return np.stack([flip_item(lab[n, :D, :H, :W], int(flips[n]) if flips is not None else 0) for n in range(lab.shape[0])])


def ordered(a):
    """fp32 -> int64 that orders like the floats (adjacent floats differ by 1; -0.0 and +0.0 coincide)"""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def check_prepared(got, x, stats, flips, pads, extra=None):
    """got fp32 [N, C, Dp, Hp, Wp] against prepare64 on fp64 stats: in-extent voxels within 1 fp32 ulp of float32(y64) (one rounding
    plus the freedom -ffp-contract=fast takes); with `extra` (per sample a function of y64, see propagated()) within one fp32
    spacing plus that absolute allowance; NaN where y64 is NaN; every pad voxel exactly +0.0.  -> largest ulp distance seen"""
    N, C, D, H, W = x.shape
    y = prepare64(x, stats, flips, pads)
    inside = np.zeros(y.shape, dtype=bool)
    inside[:, :, :D, :H, :W] = True
    assert got.dtype == np.float32 and got.shape == y.shape
    assert (got[~inside].view(np.uint32) == 0).all(), "a pad voxel is not +0.0"
    worst = 0
    for n in range(N):
        g, e = got[n][inside[n]], y[n][inside[n]]
        nan = np.isnan(e)
        assert np.array_equal(np.isnan(g), nan), "NaNs are not where the reference has them"
        g, e = g[~nan], e[~nan]
        if g.size == 0:
            continue
        e32 = e.astype(np.float32)
        if extra is None:
            dist = np.abs(ordered(g) - ordered(e32))
            worst = max(worst, int(dist.max()))
            assert dist.max() <= 1, (n, int(dist.max()))
        else:
            tol = np.spacing(np.abs(e32)).astype(np.float64) + extra[n](e)
            err = np.abs(g.astype(np.float64) - e)
            assert (err <= tol).all(), (n, float((err - tol).max()))
    return worst


def propagated(mean, inv, mean_rel, inv_rel):
    """absolute change of y = (x - mean) inv under relative errors of mean and inv: |mean| mean_rel |inv| + |y| inv_rel"""
    return lambda y: abs(mean) * mean_rel * abs(inv) * (1 + inv_rel) + np.abs(y) * inv_rel


# ------------------------------------------------------------------------------------------------ label sums
LABEL_CASES = {
    "random": (2, 75924),                   # odd-offset second sample, several blocks
    "tiny": (3, 105),                       # n_per odd: the bases fall on bytes 0, 9 and 2 of a 16-byte line
    "wrap": (1, 48 ** 3),                   # all 255: 255^2 n passes 2^32 at n = 66 052
    "zero": (2, 4099),                      # all-zero maps: dice = eps / eps = 1
}


def build_labels(name):
    N, n_per = LABEL_CASES[name]
    if name == "wrap":
        return np.full((N, n_per), 255, np.uint8), np.full((N, n_per), 255, np.uint8)
    if name == "zero":
        return np.zeros((N, n_per), np.uint8), np.zeros((N, n_per), np.uint8)
    g = rng_of("labels/" + name)
    return g.integers(0, 9, size=(N, n_per)).astype(np.uint8), g.integers(0, 9, size=(N, n_per)).astype(np.uint8)


def label_sums(p, t):
    """int64 [N, 3] = sum p t, sum p, sum t"""
    p, t = p.reshape(p.shape[0], -1).astype(np.int64), t.reshape(t.shape[0], -1).astype(np.int64)
    return np.stack([(p * t).sum(1), p.sum(1), t.sum(1)], 1)


def dice64(sums, eps=1e-6):
    I, P, T = (int(v) for v in np.asarray(sums).reshape(-1, 3).sum(0))
    return (2.0 * I + eps) / (P + T + eps)
