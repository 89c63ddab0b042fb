"""The one-channel 3x3 stem whose convolution output is never stored (csrc/direct.hip: gs_stem_fwd_bn, gs_stem_fwd_bn_pair,
gs_stem_bwd_onepass[_strided], gs_stem_bwd_finalize, and the stored-y fallback gs_stem_bn_bwd_wgrad) stated in fp64 without
tiles, lanes or strips, on operands for which every fp32 sum a kernel forms is exact in any order (tests/exact_reference.py
gives the method).  Plain torch on the CPU: no GPU, no native library.

  forward    v = conv(x, w) * scale + shift;  z = act(v);  hi = round16(z);  lo = round16(z - hi);  hi + lo == z
  one pass   g = dz * act'(v) (the kernel takes the sign of the stored z);  s1[c] = sum_p g;  A[c][t] = sum_p g x_t(p)
  finalize   the DEFINITION, pixel by pixel: y = conv(x, w), xhat = (y - mean) invstd, c1 = s1 / count, c2 = sum g xhat / count,
             dy = scale (g - c1 - xhat c2), dW[c][t] = gscale sum_p dy x_t, dgamma = gscale sum g xhat, dbeta = gscale s1.
             The pixel sums (sum g x_t, sum x_t, sum xhat x_t, sum g, sum g xhat) are exact in fp64 on these operands; they are
             combined in exact rational arithmetic (fractions.Fraction), so the expected value carries NO rounding at all.
             stem_finalize_closed is the kernel's closed form (tap sums S and tap Gram matrix G of the image) in the same
             arithmetic: the CPU test shows it equal to the definition, counts the significant bits of its intermediates and
             derives the mutants from it.
  fallback   gs_stem_bn_bwd_wgrad on a stored 16-bit y of its own (exact_reference._bn_operands): dw = gscale sum_p dy x_t

Operands: image T = {-1, 0, 1} at density 1/2 or P = {0, 1, 2} (no cancellation in the tap sums and Gram entries: the DC offset
of real inputs), non-zero pixels planted at both ends of the first two and last two rows of every image (all corners and both
sides of every image seam); weights integers in [-4, 4] (times 5 under LeakyReLU); invstd and |gamma| powers of two in [1/2, 2],
gamma negative on every third channel, mean small integers, shift integers with +300 / +2100 on a quarter of the channels each;
on the channels c % 4 == 0 (|scale| = 1) the shift is minus the scaled y of one pixel, so v == 0 there (and wherever y repeats),
with a gradient on it; dz integers of set S (times 5 under LeakyReLU).

stem_bwd_ppb / stem_bwd_blocks / stem_lds_bytes restate the host formulas of csrc/direct.hip; the GPU test compares them with
gs_stem_bwd_tiles and with the refusal of the library."""
from fractions import Fraction

import torch
import torch.nn.functional as F

from tests.exact_reference import (LIMIT, _bn_operands, act_bwd64, act_fwd64, draw, expect16, generator, require_channel_sums,
                                   require_dyadic, require_fifths, require_integers, require_pow2)

C = 64
SC_TILE = 1024                      # pixels per forward tile (csrc/direct.hip)
SC_GROUP = 4                        # forward tiles per block of gs_stem_stats
STEM_BWD_BLOCKS = 512               # GSSEG_STEM_BWD_BLOCKS, read once per process: the tests run at its default
LDS_LIMIT = 64 * 1024
LOOP_STEP = 128                     # pixels per iteration of the backward kernels' loop: 32 pixel lanes x 4 unroll slots


def stem_bwd_ppb(M: int) -> int:
    return max(64, -(-M // STEM_BWD_BLOCKS))


def stem_bwd_blocks(M: int) -> int:
    return -(-M // stem_bwd_ppb(M))


def stem_fwd_tiles(M: int) -> int:
    return -(-M // SC_TILE)


def stem_lds_bytes(N: int, H: int, W: int) -> int:
    """dynamic LDS of stem_bwd_onepass_kernel / stem_bn_bwd_wgrad_kernel: the image strip, padded to four floats, + [256][25]"""
    return (((stem_bwd_ppb(N * H * W) + 2 * W + 2 + 3) & ~3) + 256 * 25) * 4


def widest_accepted(N: int, H: int) -> int:
    W = 1
    while stem_lds_bytes(N, H, W + 1) <= LDS_LIMIT:
        W += 1
    return W


# ------------------------------------------------------------------------------------------------ cases
# (N, H, W) -> (pixels per backward block, backward blocks, forward tiles): asserted against the formulas by the CPU test, so
# that the list cannot silently stop reaching its edge
STEM_SHAPES = {
    (1, 1, 1): (64, 1, 1), (1, 1, 5): (64, 1, 1), (1, 7, 1): (64, 1, 1), (2, 3, 3): (64, 1, 1),     # every pixel on a border; ppb > M
    (1, 32, 32): (64, 16, 1),             # exactly one forward tile; count a power of two
    (2, 18, 22): (64, 13, 1),             # one ragged tile
    (2, 64, 64): (64, 128, 8),            # 8 full tiles; blocks coincide with rows; count a power of two
    (3, 45, 53): (64, 112, 7),            # tiles no multiple of SC_GROUP; blocks straddle rows and image seams
    (3, 160, 150): (141, 511, 71),        # ppb = 141: a second loop iteration for 13 of the 32 pixel lanes; last block 90 pixels
    (2, 224, 224): (196, 512, 98),        # ppb = 196 = 128 + 68: two iterations, all four unroll slots
    (1, 2, 4959): (64, 155, 10),          # the widest strip accepted: exactly 64 KiB
}
STEM_REFUSED = (1, 2, 4960)
STEM_ALL_ACTS = [(2, 18, 22), (3, 45, 53), (2, 64, 64)]
ACTS = {"none": 0, "relu": 1, "leaky": 2}
IMAGE_SETS = ("T", "P")
# (shape, act, image set): dz sits in a channel slice (stride 128, offset 64) under T and dense under P; gscale 0.5 under T, 1 under P
STEM_CASES = [(s, a, i) for s in STEM_SHAPES for a in (("relu", "none", "leaky") if s in STEM_ALL_ACTS else ("relu",)) for i in IMAGE_SETS]
STEM_MUTANTS = ("row_wrap", "image_wrap", "tap_transposed", "relu0_live", "drop_tail", "gram_row_major_full", "no_mean_term",
                "lo_of_unrounded")
TAP_MUTANTS = ("row_wrap", "image_wrap", "tap_transposed")


def case_id(case) -> str:
    s, a, i = case
    return "x".join(str(v) for v in s) + f"-{a}-{i}"


def pow2_count(shape) -> bool:
    M = shape[0] * shape[1] * shape[2]
    return M & (M - 1) == 0


def dz_layout(case):
    """(stride, channel offset) of the gradient buffer"""
    return (128, 64) if case[2] == "T" else (64, 0)


def gscale_of(case) -> float:
    return 0.5 if case[2] == "T" else 1.0


def stem_image(g, shape, iset) -> torch.Tensor:
    N, H, W = shape
    x = draw(g, "T", "a", (N, 1, H, W), 0.5) if iset == "T" else torch.randint(0, 3, (N, 1, H, W), generator=g).float()
    rows = sorted({r for r in (0, 1, H - 2, H - 1) if 0 <= r < H})
    for r in rows:
        for col in (0, W - 1):
            keep = x[:, 0, r, col] != 0
            x[:, 0, r, col] = torch.where(keep, x[:, 0, r, col], torch.ones(N))
    return x


def _coefficients(g, m):
    """per-channel BatchNorm coefficients in the style of exact_reference._bn_operands (m: 5 under LeakyReLU, else 1)"""
    c = torch.arange(C)
    invstd = 2.0 ** torch.randint(-1, 2, (C,), generator=g).double()
    gmag = torch.where(c % 4 == 0, 1.0 / invstd, 2.0 ** torch.randint(-1, 2, (C,), generator=g).double())
    sign = torch.where(c % 3 == 1, -1.0, 1.0).double()
    small = torch.randint(-2, 3, (C,), generator=g).double()
    shift = (small + torch.where(c % 4 == 1, 300.0, 0.0) + torch.where(c % 4 == 2, 2100.0, 0.0)) * m
    mean = torch.randint(-2, 3, (C,), generator=g).double()
    for t in (invstd, gmag):
        for s in t.unique().tolist():
            require_pow2(s)
    return invstd, sign * gmag * invstd, shift, mean


def planted_pixel(c: int, M: int) -> int:
    """the pixel whose v is made zero on channel c (c % 4 == 0)"""
    return (7 * (c // 4) + 3) % M


def stem_build(case):
    """operands of one case, NCHW on the CPU, with the conditions that make every fp32 intermediate exact asserted on them"""
    shape, act, iset = case
    N, H, W = shape
    M = N * H * W
    g = generator(("stem_family",) + tuple(case))
    m = 5.0 if act == "leaky" else 1.0
    x = stem_image(g, shape, iset)
    w = draw(g, "S", "w", (C, 1, 3, 3)) * m
    invstd, scale, shift, mean = _coefficients(g, m)
    dz = draw(g, "S", "a", (N, C, H, W)) * m
    y = F.conv2d(x.double(), w.double(), None, padding=1)
    yf, dzf = y.permute(0, 2, 3, 1).reshape(M, C), dz.permute(0, 2, 3, 1).reshape(M, C)      # copies, pixel-major
    for c in range(0, C, 4):
        p = planted_pixel(c, M)
        shift[c] = -scale[c] * yf[p, c]                      # |scale| = 1 here: v == 0 at pixel p (and wherever y repeats)
        if dzf[p, c] == 0:
            dzf[p, c] = m
    last = min(stem_bwd_ppb(M), M) - 1                       # a gradient on the last pixel of the first and of the last block
    for p in (last, M - 1):                                  # (channel 1: shift near +300, v > 0 under every activation)
        if dzf[p, 1] == 0:
            dzf[p, 1] = m
    dz = dzf.view(N, H, W, C).permute(0, 3, 1, 2).contiguous()
    require_integers(x, w, mean.float(), dz)
    assert torch.equal(shift, shift.round()) and float(x.abs().max()) <= 2 and float(w.abs().max()) <= 4 * m
    v = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    require_dyadic(v, case_id(case) + " v", 2)
    if act == "leaky":
        require_fifths(w, shift.float(), v, dz)
    # sums over ALL pixels of |g| and |g| |x_t| <= |dz| * 2 stay below 2^24: every sub-sum a block, lane or slot forms is exact
    require_channel_sums(dz * 2, case_id(case) + " A", squares=False)
    return {"case": case, "act": act, "x": x, "w": w, "scale": scale.float(), "shift": shift.float(), "mean": mean.float(),
            "invstd": invstd.float(), "dz": dz, "gscale": gscale_of(case), "zero_share": float((v == 0).double().mean())}


# ------------------------------------------------------------------------------------------------ the operation
def stem_taps(x: torch.Tensor, mutant=None) -> torch.Tensor:
    """X[p][t] = x_t(p), the image value under tap t = ky * 3 + kx of pixel p (flat over n, y, x), 0 outside its image.
    Stated on the flat image with a row mask and a column mask, as the backward kernels read their strip.  Mutants: row_wrap (no
    column mask: the flat neighbour in the previous / next row), image_wrap (rows masked against all N * H rows instead of the
    image's H: the neighbouring image), tap_transposed (ky and kx swapped)."""
    N, _, H, W = x.shape
    M = N * H * W
    flat = x.double().reshape(-1)
    p = torch.arange(M)
    ox, r = p % W, p // W
    oy = r % H
    out = torch.zeros(M, 9, dtype=torch.float64)
    for t in range(9):
        ky, kx = divmod(t, 3)
        if mutant == "tap_transposed":
            ky, kx = kx, ky
        dy, dx = ky - 1, kx - 1
        row_ok = ((r + dy >= 0) & (r + dy < N * H)) if mutant == "image_wrap" else ((oy + dy >= 0) & (oy + dy < H))
        col_ok = torch.ones(M, dtype=torch.bool) if mutant == "row_wrap" else ((ox + dx >= 0) & (ox + dx < W))
        idx = p + dy * W + dx
        ok = row_ok & col_ok & (idx >= 0) & (idx < M)
        out[:, t] = torch.where(ok, flat[idx.clamp(0, M - 1)], torch.zeros(M, dtype=torch.float64))
    return out


def _cols(c):
    return tuple(c[k].double().view(1, C) for k in ("scale", "shift", "mean", "invstd"))


def dropped_pixels(M: int) -> torch.Tensor:
    """drop_tail: the last pixel of every backward block whose pixel count is no multiple of the loop step (its last iteration has
    masked slots)"""
    ppb = stem_bwd_ppb(M)
    ends = [min(b * ppb + ppb, M) for b in range(stem_bwd_blocks(M))]
    return torch.tensor([e - 1 for b, e in enumerate(ends) if (e - b * ppb) % LOOP_STEP != 0], dtype=torch.long)


def stem_reference(c, dt, mutant=None):
    """fp64 expected values of case c for the 16-bit dtype dt.  hi, lo: [N, H, W, 64] of dtype dt; z: the unrounded act(v), fp64;
    s1 [64], A [64][9]: fp64, exact integers.  mutant: one of STEM_MUTANTS that acts on these outputs."""
    N, _, H, W = c["x"].shape
    M = N * H * W
    scale, shift, mean, invstd = _cols(c)
    w9 = c["w"].double().view(C, 9)
    X = stem_taps(c["x"])
    Xm = stem_taps(c["x"], mutant) if mutant in TAP_MUTANTS else X
    z = act_fwd64((Xm @ w9.t()) * scale + shift, c["act"])
    hi = expect16(z.view(N, H, W, C), dt)
    lo = torch.zeros_like(hi) if mutant == "lo_of_unrounded" else expect16(z.view(N, H, W, C) - hi.double(), dt)
    v = (X @ w9.t()) * scale + shift                                   # the backward reads the TRUE stored activation
    dz = c["dz"].double().permute(0, 2, 3, 1).reshape(M, C)
    g = act_bwd64(dz, v, c["act"], 1.0 if mutant == "relu0_live" else 0.0)
    if mutant == "drop_tail":
        g = g.clone()
        g[dropped_pixels(M)] = 0
    return {"hi": hi, "lo": lo, "z": z.view(N, H, W, C), "v": v, "g": g, "X": X, "s1": g.sum(0), "A": g.t() @ Xm}


def stem_pixel_sums(c, ref):
    """the pixel sums of the definition, each exact in fp64: with xhat = (conv(x, w) - mean) * invstd per pixel,
    s1 = sum g, s2 = sum g xhat, P1[c][t] = sum g x_t, P2[t] = sum x_t, P3[c][t] = sum xhat x_t"""
    N, _, H, W = c["x"].shape
    M = N * H * W
    _, _, mean, invstd = _cols(c)
    y = F.conv2d(c["x"].double(), c["w"].double(), None, padding=1).permute(0, 2, 3, 1).reshape(M, C)
    xhat = (y - mean) * invstd
    g, X = ref["g"], ref["X"]
    out = {"s1": g.sum(0), "s2": (g * xhat).sum(0), "P1": g.t() @ X, "P2": X.sum(0), "P3": xhat.t() @ X}
    for k, t in out.items():                                  # multiples of 1/2 far below 2^53: no fp64 sum rounded
        assert torch.equal(t * 2, (t * 2).round()) and float(t.abs().max()) < 2.0 ** 50, k
    out["bound"] = {"s1": g.abs().sum(0), "s2": (g * xhat).abs().sum(0), "P1": g.abs().t() @ X.abs(), "P3": xhat.abs().t() @ X.abs()}
    for k, t in out["bound"].items():
        assert float(t.max()) < 2.0 ** 50, k
    return out


def _fr(t: torch.Tensor):
    return [Fraction(v) for v in t.reshape(-1).tolist()]


def stem_finalize_definition(c, sums, train: bool, gscale: float):
    """exact rational dW [64][9], dgamma [64], dbeta [64] of the definition (train: batch statistics, c1 and c2 as defined; else
    constants, c1 = c2 = 0), and per dW entry the magnitudes of the three terms of A - c1 S_t - c2 (sum xhat x_t)"""
    count = Fraction(c["x"].numel())
    gs = Fraction(gscale)
    scale = _fr(c["scale"])
    s1, s2, P1, P2, P3 = _fr(sums["s1"]), _fr(sums["s2"]), _fr(sums["P1"]), _fr(sums["P2"]), _fr(sums["P3"])
    dW, mag = [], []
    for ch in range(C):
        c1, c2 = (s1[ch] / count, s2[ch] / count) if train else (Fraction(0), Fraction(0))
        for t in range(9):
            a, b, d = P1[ch * 9 + t], c1 * P2[t], c2 * P3[ch * 9 + t]
            dW.append(gs * scale[ch] * (a - b - d))
            mag.append((abs(gs * scale[ch]), abs(a), abs(b), abs(d)))
    return {"dW": dW, "dgamma": [gs * v for v in s2], "dbeta": [gs * v for v in s1], "mag": mag}


def sig_bits(v: Fraction) -> float:
    """significant bits of a dyadic rational (inf for any other: it is no binary floating-point number of any width)"""
    if v == 0:
        return 0
    d = v.denominator
    if d & (d - 1):
        return float("inf")
    n = abs(v.numerator)
    return (n // (n & -n)).bit_length()


def gram_index(t: int, u: int) -> int:
    """index of G[t][u] in the 45 packed entries: the upper triangle, row-major"""
    lo, hi = min(t, u), max(t, u)
    return lo * 9 - lo * (lo - 1) // 2 + (hi - lo)


def stem_finalize_closed(c, ref, train: bool, gscale: float, mutant=None):
    """stem_bwd_finalize_kernel's formula, step by step, in exact rational arithmetic, from the image's tap sums S[9] and packed tap
    Gram matrix G[45] and the one-pass sums s1 and A:
        wA = sum_u w_u A_u;  s2 = invstd (wA - mean s1);  c1 = s1 / count;  c2 = s2 / count;  wg = sum_u w_u G[u][t]
        r = A_t - c1 S_t - c2 invstd (wg - mean S_t);  dW = gscale scale r
    Returns dW and `bits`, the largest number of significant bits of any intermediate (every partial sum of wA and wg included).
    Mutants: gram_row_major_full (G[t][u] read at packed index t * 9 + u, zero past the 45 entries), no_mean_term (- mean S_t
    left out)."""
    X = ref["X"]
    Gfull = X.t() @ X
    packed = torch.zeros(45, dtype=torch.float64)
    for t in range(9):
        for u in range(t, 9):
            packed[gram_index(t, u)] = Gfull[t, u]
    return finalize_closed_from_sums(c, X.sum(0), packed, ref["s1"], ref["A"], c["x"].numel(), train, gscale, mutant)


def finalize_closed_from_sums(c, S, packed, s1, A, count, train: bool, gscale: float, mutant=None):
    """the formula of stem_finalize_closed on given totals: S [9] and packed G [45] (over the forward tiles), s1 [64] and A [64][9]
    (over the backward blocks); c gives w, scale, mean, invstd.  `mag`: per dW entry (|gscale scale|, |A_t|, |c1 S_t|, |X|)."""
    S, packed = _fr(S), _fr(packed)
    count, gs = Fraction(count), Fraction(gscale)
    w, scale, mean, invstd = _fr(c["w"]), _fr(c["scale"]), _fr(c["mean"]), _fr(c["invstd"])
    s1v, Av = _fr(s1), _fr(A)
    seen = []
    dW, mag, s2v = [], [], []
    for ch in range(C):
        s1, mu, is_ = s1v[ch], mean[ch], invstd[ch]
        wA = Fraction(0)
        for u in range(9):
            wA += w[ch * 9 + u] * Av[ch * 9 + u]
            seen.append(wA)
        s2 = is_ * (wA - mu * s1)
        s2v.append(s2)
        c1, c2 = (s1 / count, s2 / count) if train else (Fraction(0), Fraction(0))
        seen += [mu * s1, wA - mu * s1, s2, c1, c2, c2 * is_]
        for t in range(9):
            wg = Fraction(0)
            for u in range(9):
                if mutant == "gram_row_major_full":
                    gv = packed[t * 9 + u] if t * 9 + u < 45 else Fraction(0)
                else:
                    gv = packed[gram_index(t, u)]
                wg += w[ch * 9 + u] * gv
                seen.append(wg)
            inner = wg if mutant == "no_mean_term" else wg - mu * S[t]
            r = Av[ch * 9 + t] - c1 * S[t] - c2 * is_ * inner
            seen += [c1 * S[t], Av[ch * 9 + t] - c1 * S[t], mu * S[t], inner, c2 * is_ * inner, r, gs * scale[ch], gs * scale[ch] * r]
            dW.append(gs * scale[ch] * r)
            mag.append((abs(gs * scale[ch]), abs(Av[ch * 9 + t]), abs(c1 * S[t]), abs(c2 * is_ * inner)))
    return {"dW": dW, "mag": mag, "dgamma": [gs * v for v in s2v], "dbeta": [gs * v for v in s1v], "bits": max(sig_bits(v) for v in seen)}


# gs_stem_bwd_finalize alone on synthetic integer partials, for the reduction loops no image of the case list is large enough to
# reach: 16 lanes with an 8-deep unroll over the forward tiles need more than 112 tiles.  (N, H, W) only sets the counts here:
#   (1, 128, 1024)  131072 pixels, a power of two: 128 tiles (one unrolled round on every lane, no tail), 512 blocks
#   (1, 140, 1024)  143360 pixels: 140 tiles (one unrolled round, then a tail on 12 of the 16 lanes), 512 blocks of 280 pixels
FINALIZE_SYNTHETIC = [(1, 128, 1024), (1, 140, 1024)]


def finalize_synthetic_build(shape):
    """fp32 integer partials in the layouts gs_stem_stats and gs_stem_bwd_onepass write, with their fp64 totals, and coefficients as
    in stem_build.  They are the sums of no image: the reference is the kernel's formula in exact rational arithmetic, which
    test_stem_reference_cpu.py shows equal to the definition on every case that has pixels."""
    M = shape[0] * shape[1] * shape[2]
    g = generator(("stem_finalize_synthetic",) + tuple(shape))
    nb, nsg = stem_bwd_blocks(M), stem_fwd_tiles(M)
    w = draw(g, "S", "w", (C, 1, 3, 3))
    invstd, scale, shift, mean = _coefficients(g, 1.0)
    taps = torch.randint(0, 65, (nsg, 54), generator=g).float()
    s1p = torch.randint(-64, 65, (nb, C), generator=g).float()
    ws = torch.randint(-64, 65, (nb, C * 9), generator=g).float()
    tot = taps.double().sum(0)
    return {"w": w, "scale": scale.float(), "mean": mean.float(), "invstd": invstd.float(), "taps": taps, "s1p": s1p, "ws": ws, "count": M,
            "S": tot[:9], "packed": tot[9:], "s1": s1p.double().sum(0), "A": ws.double().sum(0).view(C, 9), "nb": nb, "nsg": nsg}


def finalize_mutant_applies(c, mutant, train: bool) -> bool:
    """both act on the train-mode c2 term only; no_mean_term needs a channel with a non-zero mean"""
    return train and (mutant == "gram_row_major_full" or bool((c["mean"] != 0).any()))


def mutant_applies(c, mutant) -> bool:
    """whether `mutant` changes what case c asks of stem_reference (otherwise it IS the reference there)"""
    N, _, H, W = c["x"].shape
    return {"row_wrap": N * H > 1,                      # a previous / next row exists in the flat image
            "image_wrap": N > 1,
            "tap_transposed": H * W > 1,                # with one pixel only the centre tap is inside
            "relu0_live": c["act"] == "relu",
            "drop_tail": True,                          # no shape here has a block of a multiple of 128 pixels
            "lo_of_unrounded": True}[mutant]


# fp64 roundings of stem_bwd_finalize_kernel on the way to dW, per term of r = A_t - c1 S_t - X, X = c2 invstd (wg - mean S_t);
# each at most 2^-53 of the magnitude of the term it touches.  wA, mean * s1, wg and mean * S_t are sums and products of integers
# below 2^53 and invstd is a power of two: s2 and (wg - mean S_t) are exact and are not counted.
#   A     4   the two subtractions of `const double r = tot[..] - c1 * St - c2 * is * (wg - mu * St)`, and the two products of
#             `(double)gscale * (double)scale[c] * r`
#   c1St  6   `s1 / count`, `c1 * St`, then the four above
#   X     6   `s2 / count`, `c2 * is`, `(c2 * is) * (wg - mu * St)`, the second subtraction, the two final products
# + 1 on every term for the second-order products of these roundings (each 2^-53 of a first-order one)
STEM_FINALIZE_ROUNDINGS = {"A": 4 + 1, "c1St": 6 + 1, "X": 6 + 1}


def finalize_bound(exact: Fraction, mag) -> Fraction:
    """the largest |error| of one dW entry on a count that is no power of two: one fp32 rounding of the result and the kernel's
    fp64 roundings, nothing measured"""
    k, a, b, d = mag
    r = STEM_FINALIZE_ROUNDINGS
    return abs(exact) * Fraction(1, 2 ** 24) + k * (r["A"] * a + r["c1St"] * b + r["X"] * d) * Fraction(1, 2 ** 53)


# ------------------------------------------------------------------------------------------------ fp32, shuffled
def _runs32(rows: torch.Tensor, X: torch.Tensor, perm: torch.Tensor, run: int = 64):
    """sum_p rows[p][c] and sum_p rows[p][c] X[p][t] over the permuted pixels: products, runs of `run` pixels and the sum of the runs
    all in fp32"""
    f = torch.float32
    M = rows.shape[0]
    pad = (-M) % run
    r = torch.cat([rows[perm], torch.zeros(pad, rows.shape[1], dtype=f)]).view(-1, run, rows.shape[1])
    xs = torch.cat([X[perm], torch.zeros(pad, 9, dtype=f)]).view(-1, run, 9)
    s1 = r.sum(1, dtype=f).sum(0, dtype=f)
    A = torch.einsum("rpc,rpt->rct", r, xs).sum(0, dtype=f)
    assert s1.dtype == A.dtype == f
    return s1, A


def stem_fp32_shuffled(c, dt, seed):
    """the forward and the one-pass backward the way a kernel may form them: every elementwise step in fp32 (the convolution as nine
    fp32 products summed in a random tap order, v, the slope product), the pixel sums over a random permutation in runs of 64, in
    fp32.  Equal to stem_reference bit for bit is what entitles the GPU test to zero tolerance."""
    f = torch.float32
    N, _, H, W = c["x"].shape
    M = N * H * W
    gen = torch.Generator().manual_seed(seed)
    X = stem_taps(c["x"]).to(f)
    w9 = c["w"].view(C, 9)
    y = torch.zeros(M, C, dtype=f)
    for t in torch.randperm(9, generator=gen).tolist():
        y = y + X[:, t:t + 1] * w9[:, t].view(1, C)
    v = y * c["scale"].view(1, C) + c["shift"].view(1, C)
    slope = torch.tensor({"none": 1.0, "relu": 0.0, "leaky": 0.2}[c["act"]], dtype=f)
    one = torch.tensor(1.0, dtype=f)
    z = torch.where(v > 0, v, v * slope)
    hi = z.to(dt)
    lo = (z - hi.to(f)).to(dt)
    g = c["dz"].permute(0, 2, 3, 1).reshape(M, C) * torch.where(hi.to(f) > 0, one, slope)      # the sign of the STORED z
    s1, A = _runs32(g, X, torch.randperm(M, generator=gen))
    assert v.dtype == z.dtype == g.dtype == f
    return {"hi": hi.view(N, H, W, C), "lo": lo.view(N, H, W, C), "z": z.view(N, H, W, C), "s1": s1, "A": A}


# ------------------------------------------------------------------------------------------------ the stored-y fallback
def wgrad_build(case):
    """gs_stem_bn_bwd_wgrad: a stored 16-bit y of its own (not conv(x, w): the kernel's contract does not tie them) with zeros of
    v planted, c1 / c2 multiples of 1/4, dz in the layout of the case, the image of the case's set"""
    shape, act, iset = case
    N, H, W = shape
    g = generator(("stem_wgrad",) + tuple(case))
    m = 5.0 if act == "leaky" else 1.0
    c = _bn_operands(g, (N, H, W, C), act, False)
    x = stem_image(g, shape, iset)
    dz = draw(g, "S", "a", (N, C, H, W)) * m
    dz.view(-1)[0] = m                                        # a gradient on the planted v == 0 of pixel 0, channel 0
    require_integers(x, dz)
    if act == "leaky":
        require_fifths(dz, c["y"], c["shift"])
    c.update(case=case, act=act, x=x, dz=dz, gscale=gscale_of(case))
    return c


def wgrad_dy(c, mutant=None):
    """dy [M][64] in fp64 as exact_reference.bn_reference states it (dz_a only, no pool, no keep mask)"""
    M = c["x"].numel()
    flat = lambda t: t.double().permute(0, 2, 3, 1).reshape(M, C)                   # noqa: E731
    col = lambda k: c[k].double().view(1, C)                                        # noqa: E731
    y = flat(c["y"])
    v = y * col("scale") + col("shift")
    gh = act_bwd64(flat(c["dz"]), v, c["act"], 1.0 if mutant == "relu0_live" else 0.0)
    xh = (y - col("mean")) * col("invstd")
    dy = col("scale") * (gh - col("c1") - xh * col("c2"))
    if mutant == "drop_tail":
        dy = dy.clone()
        dy[dropped_pixels(M)] = 0
    return dy


def wgrad_reference(c, mutant=None):
    """dw [64][9] = float32(gscale * sum_p dy x_t): the kernel sums a block in fp32 (exact: wgrad_conditions), the blocks in fp64
    (exact) and rounds the scaled total once"""
    dy = wgrad_dy(c, mutant)
    X = stem_taps(c["x"], mutant if mutant in TAP_MUTANTS else None)
    total = dy.t() @ X
    assert torch.equal(total * 256, (total * 256).round()) and float(total.abs().max()) < 2.0 ** 40        # the fp64 sum is exact
    return {"dy": dy, "X": X, "dw": (total * c["gscale"]).float().view(C, 1, 3, 3)}


def wgrad_conditions(c):
    """per backward block and channel, the sum of |dy| * max_t |x_t| in units of dy's last bit stays below 2^24: the fp32 sums of a
    block over its 32 pixel lanes, four slots and loop iterations are exact in any order.  Returns the largest such sum."""
    M = c["x"].numel()
    dy = wgrad_dy(c)
    k = require_dyadic(dy, "dy", 8)
    ppb, nb = stem_bwd_ppb(M), stem_bwd_blocks(M)
    units = dy.abs() * 2.0 ** k * stem_taps(c["x"]).abs().amax(1, keepdim=True)
    units = torch.cat([units, torch.zeros(nb * ppb - M, C, dtype=torch.float64)]).view(nb, ppb, C).permute(1, 0, 2).reshape(ppb, nb * C)
    require_channel_sums(units, "stem wgrad block sums", squares=False)          # [ppb][nb * 64]: a "channel" per block and channel
    return float(units.sum(0).max())


def wgrad_fp32_shuffled(c, seed):
    """dy elementwise in fp32, every block's sums in fp32 over a random order of its pixels, the blocks in fp64, one rounding"""
    f = torch.float32
    M = c["x"].numel()
    flat = lambda t: t.to(f).permute(0, 2, 3, 1).reshape(M, C)                       # noqa: E731
    col = lambda k: c[k].to(f).view(1, C)                                            # noqa: E731
    y = flat(c["y"])
    v = y * col("scale") + col("shift")
    slope = torch.tensor({"none": 1.0, "relu": 0.0, "leaky": 0.2}[c["act"]], dtype=f)
    gh = flat(c["dz"]) * torch.where(v > 0, torch.tensor(1.0, dtype=f), slope)
    xh = (y - col("mean")) * col("invstd")
    dy = col("scale") * (gh - col("c1") - xh * col("c2"))
    assert dy.dtype == f
    X = stem_taps(c["x"]).to(f)
    ppb, nb = stem_bwd_ppb(M), stem_bwd_blocks(M)
    gen = torch.Generator().manual_seed(seed)
    order = torch.cat([b * ppb + torch.randperm(min(ppb, M - b * ppb), generator=gen) for b in range(nb)])
    pad = nb * ppb - M
    d = torch.cat([dy[order], torch.zeros(pad, C, dtype=f)]).view(nb, ppb, C)
    xs = torch.cat([X[order], torch.zeros(pad, 9, dtype=f)]).view(nb, ppb, 9)
    blocks = torch.einsum("bpc,bpt->bct", d, xs)
    assert blocks.dtype == f
    return (blocks.double().sum(0) * c["gscale"]).float().view(C, 1, 3, 3)


assert LIMIT == 2 ** 24
