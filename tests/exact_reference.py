"""Exact-integer references for the 16-bit convolution, data-gradient, weight-gradient and reduction kernels, in plain
torch on the CPU (no GPU, no native library).

Give a kernel integer-valued operands: every product of two small integers is exact in fp32, and a sum of such products
is exact in fp32 in ANY order as long as the sum of the absolute products stays below 2^24.  MFMA accumulation order,
split-K, atomics, slab reductions and persistent-grid scheduling then all have to produce the one exact integer, and a
16-bit store has to produce its one correctly rounded value: a single missing, doubled or misplaced product anywhere is a
mismatch.  There is no tolerance in this file, and no function here takes one.

  value sets   S dense signed, P dense positive, T(d) sparse ternary (draw)
  conditions   integer operands |v| <= 256, sums of absolute products < 2^24, per-channel sums of |y| and y^2 < 2^24 where
               partial sums are checked, power-of-two scales (require_*; a violated condition is a wrong case list: it fails)
  references   the operation in fp64 (autograd); fp32 only behind require_products, where it equals fp64 bit for bit
  expected     expect32 / expect16 / expect_leaky16: the reference times the scale; one round-to-nearest-even to the dtype
  comparer     assert_exact: count, share and coordinates of the mismatching elements

The case lists at the end are shared by tests/test_exact_kernels_gpu.py (kernel against reference) and
tests/test_exact_reference_cpu.py (every case meets its conditions; the reference is order independent; the comparer sees
what the norm-wise metric of tests/test_gpu_kernels.py cannot)."""
import math
import zlib

import torch
import torch.nn.functional as F

LIMIT = 2 ** 24                     # integers up to here are exact in fp32
DTS = [("f16", torch.float16), ("bf16", torch.bfloat16)]


# ------------------------------------------------------------------------------------------------ value sets
def case_seed(case_id) -> int:
    return zlib.crc32(repr(case_id).encode()) & 0x7FFFFFFF


def generator(case_id) -> torch.Generator:
    return torch.Generator().manual_seed(case_seed(case_id))


RANGES = {"S": {"a": (-8, 8), "w": (-4, 4)}, "P": {"a": (0, 8), "w": (0, 4)}}


def draw(g, vset: str, kind: str, shape, d: float = None) -> torch.Tensor:
    """fp32 tensor of integers: kind "a" (activation / gradient) or "w" (weight) of value set S / P, or T with density d."""
    shape = tuple(shape)
    if vset == "T":
        assert d is not None and 0 < d <= 1
        nz = torch.rand(shape, generator=g) < d
        sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
        return (nz * sign).float()
    lo, hi = RANGES[vset][kind]
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def density(pixels: int, products: int) -> float:
    """T(d) for a case whose per-channel sums over `pixels` outputs of `products` products each are checked: every product is
    +-1 with probability d^2, so E[sum y^2] = pixels * products * d^2; the largest d in 1/2 .. 1/64 that keeps this expectation
    under 2^23 (a factor 2 for the spread across channels).  tests/test_exact_reference_cpu.py proves each choice on the
    reference."""
    for k in (1, 2, 3, 4, 5, 6):
        d = 0.5 ** k
        if pixels * products * d * d < LIMIT / 2:
            return d
    raise AssertionError(("no density for", pixels, products))


# ------------------------------------------------------------------------------------------------ exactness conditions
def require_integers(*tensors):
    for t in tensors:
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 256, "operands must be integers with |v| <= 256"


def require_products(n_products: int, a: torch.Tensor, b: torch.Tensor, what: str = ""):
    """The same operation on absolute values stays below 2^24: n_products * max|a| * max|b| bounds every output of it."""
    bound = n_products * float(a.abs().max()) * float(b.abs().max())
    assert bound < LIMIT, f"{what}: {n_products} products x {float(a.abs().max())} x {float(b.abs().max())} = {bound} >= 2^24"


def require_channel_sums(y: torch.Tensor, what: str = "", squares: bool = True):
    """y [N, C, ...]: per channel, the sums over all pixels of |y| and y^2 stay below 2^24 (any sub-sum a kernel forms per
    tile, block or split is then exact too).  Returns the exact sums (sum y, sum y^2) in fp64.  squares=False: only the sum
    of |y| is part of the case (sum y^2 is neither bounded nor returned)."""
    yd = y.double()
    dims = [0] + list(range(2, y.dim()))
    sa = float(yd.abs().sum(dims).max())
    if not squares:
        assert sa < LIMIT, f"{what}: max sum |y| = {sa} >= 2^24"
        return yd.sum(dims), None
    s2 = (yd * yd).sum(dims)
    assert sa < LIMIT and float(s2.max()) < LIMIT, f"{what}: max sum y^2 = {float(s2.max())} >= 2^24"
    return yd.sum(dims), s2


def require_pow2(v: float):
    assert v > 0 and math.frexp(v)[0] == 0.5, f"scale {v} is not a power of two"


# ------------------------------------------------------------------------------------------------ references
def autograd(fn, args, dy=None, dtype=torch.float64, wrt=None):
    """y = fn(*args) and, with dy, the gradients with respect to the arguments `wrt` (indices; default all), evaluated in
    `dtype` (fp64; fp32 only where require_products has been asserted for every sum involved).  Gradients not asked for are None."""
    wrt = list(range(len(args))) if wrt is None else list(wrt)
    leaves = [a.detach().to(dtype, copy=True).requires_grad_(dy is not None and i in wrt) for i, a in enumerate(args)]
    y = fn(*leaves)
    if dy is None or not wrt:
        return y.detach(), [None] * len(args)
    got = torch.autograd.grad(y, [leaves[i] for i in wrt], dy.to(dtype))
    grads = [None] * len(args)
    for i, gr in zip(wrt, got):
        grads[i] = gr
    return y.detach(), grads


def channels_last(t: torch.Tensor) -> torch.Tensor:
    """[N, C, *spatial] -> [N, *spatial, C] contiguous: the kernels' layout, so that mismatch coordinates read (n, [d,] y, x, c)."""
    return t.permute(0, *range(2, t.dim()), 1).contiguous()


def chunked_conv2d_fp32(x, w, pad, chunk, perm_seed):
    """fp32 conv2d accumulated in permuted `chunk`-wide groups of input channels: a stand-in for a kernel's accumulation order."""
    order = torch.randperm(x.shape[1], generator=torch.Generator().manual_seed(perm_seed))
    acc = None
    for c0 in range(0, x.shape[1], chunk):
        idx = order[c0:c0 + chunk]
        part = F.conv2d(x[:, idx].float(), w[:, idx].float(), None, padding=pad)
        acc = part if acc is None else acc + part
    return acc


# ------------------------------------------------------------------------------------------------ expected values
def expect32(ref: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """fp32 output: the reference times a power-of-two scale, which must itself be an fp32 number."""
    require_pow2(scale)
    want = (ref.double() * scale).float()
    assert torch.equal(want.double(), ref.double() * scale), "the expected value is not representable in fp32"
    return want


def expect16(ref: torch.Tensor, dt) -> torch.Tensor:
    """16-bit output: ONE round-to-nearest-even from the exactly representable fp32 value."""
    return expect32(ref).to(dt)


def leaky_ok(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """Mask of acceptable elements of a LeakyReLU(0.2) output `got` (16-bit) for the exact pre-activation `ref`: positive
    outputs equal the rounded reference; a negative one is y * 0.2f rounded in fp32 and then to the dtype, so it may differ
    from (y32 * 0.2f).to(dt) by one unit in the last place of the dtype."""
    y32 = expect32(ref)
    want = torch.where(y32 >= 0, y32, y32 * 0.2).to(got.dtype).to(got.device)
    exact = got == want
    ulp = (got.view(torch.int16).int() - want.view(torch.int16).int()).abs() <= 1          # same sign: adjacent bit patterns
    neg = (y32 < 0).to(got.device)
    return exact | (neg & ulp & (got < 0))


# ------------------------------------------------------------------------------------------------ comparer
def mismatches(got: torch.Tensor, want: torch.Tensor, ok: torch.Tensor = None) -> torch.Tensor:
    """Coordinates [n][ndim] of the elements where got != want (values compared: +0 == -0, a NaN never equals)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = ~(got == want.to(got.device)) if ok is None else ~ok
    return bad.nonzero()


def assert_exact(got: torch.Tensor, want: torch.Tensor, what: str, ok: torch.Tensor = None):
    """got must EQUAL want.  On failure: the number of mismatching elements, their share, and the first and last few
    coordinates (for channels-last tensors: n, [d,] y, x, c) with got / want -- where the wrong elements sit is the diagnosis."""
    idx = mismatches(got, want, ok)
    if idx.shape[0] == 0:
        return
    n, total = idx.shape[0], got.numel()
    pick = idx if n <= 12 else torch.cat([idx[:6], idx[-6:]])
    wd = want.to(got.device)
    lines = []
    for k, row in enumerate(pick.cpu().tolist()):
        if n > 12 and k == 6:
            lines.append("    ...")
        lines.append(f"    {tuple(row)}: got {float(got[tuple(row)])!r} want {float(wd[tuple(row)])!r}")
    lo, hi = idx.min(0).values.cpu().tolist(), idx.max(0).values.cpu().tolist()
    raise AssertionError(f"{what}: {n} of {total} elements differ ({100.0 * n / total:.4f} %), shape {tuple(got.shape)}, "
                         f"coordinates from {tuple(lo)} to {tuple(hi)}\n" + "\n".join(lines))


def assert_leaky_exact(got: torch.Tensor, ref: torch.Tensor, what: str):
    y32 = expect32(ref)
    want = torch.where(y32 >= 0, y32, y32 * 0.2).to(got.dtype)
    assert_exact(got, want, what, ok=leaky_ok(got, ref))


# ------------------------------------------------------------------------------------------------ builders
def conv_case(case_id, vset, x_shape, w_shape, fn, products_y, products_dx=None, products_dw=None, stats=False, d=None,
              fast=False, bias=False):
    """Operands and fp64 references of one convolution-like case.  x [N, Cin, ...], w as `fn` takes it, y = fn(x, w);
    products_*: products per element of y / dx / dw (dx, dw are formed when given).  stats: the per-channel sums of y are part
    of the case.  fast: evaluate in fp32 (the conditions asserted first make that equal to fp64)."""
    g = generator((case_id, vset))
    x = draw(g, vset, "a", x_shape, d)
    w = draw(g, vset, "w", w_shape, d)
    require_integers(x, w)
    require_products(products_y, x, w, f"{case_id} {vset} y")
    out = {"x": x, "w": w}
    dtype = torch.float32 if fast else torch.float64
    want_grads = products_dx is not None or products_dw is not None
    if want_grads:
        y0, _ = autograd(fn, (x[:1], w))                                 # the output shape, from one sample
        dy = draw(g, vset, "a", (x.shape[0],) + tuple(y0.shape[1:]), d)
        require_integers(dy)
        if products_dx is not None:
            require_products(products_dx, dy, w, f"{case_id} {vset} dx")
        if products_dw is not None:
            require_products(products_dw, dy, x, f"{case_id} {vset} dw")
        out["dy"] = dy
        wrt = [i for i, p in enumerate((products_dx, products_dw)) if p is not None]
        y, (dx, dw) = autograd(fn, (x, w), dy, dtype, wrt)
        out["dx"], out["dw"] = dx, dw
    else:
        y, _ = autograd(fn, (x, w), None, dtype)
    out["y"] = y
    if bias:
        out["b"] = draw(g, "S", "a", (y.shape[1],))
        require_integers(out["b"])
        assert products_y * float(x.abs().max()) * float(w.abs().max()) + float(out["b"].abs().max()) < LIMIT
    if stats:
        out["s1"], out["s2"] = require_channel_sums(y, f"{case_id} {vset}")
    return out


# ------------------------------------------------------------------------------------------------ A: 2-D 3x3 halo kernels
ALL_FORMS = (-1, 0, 4, 8, 44)


def conv3x3_dma_shape(W, Cin, Cout) -> bool:
    """shapes the LDS-DMA form of the 3x3 kernel takes (include/gsseg.h, gs_conv3x3_q8_ok states the same rule)"""
    return W >= 24 and Cin % 64 == 0 and Cout % 8 == 0


# (N, H, W, Cin, Cout): every shape runs forward + partials, bias + ReLU, the data gradient; `wgrad` says whether the weight
# gradient runs under the dense sets too (not on the multi-item shapes: 64 * pixels must stay below 2^24 for dense values;
# under T(d) it runs on every shape, conv3x3_wgrad_runs)
_A_FWD = [(2, 13, 9, 64, 64), (1, 16, 16, 128, 192), (2, 37, 41, 64, 64), (1, 40, 33, 128, 128), (3, 7, 20, 72, 40),
          (1, 32, 64, 192, 64)]
_A_WGRAD = [(1, 40, 33, 128, 64), (4, 64, 64, 64, 128)]
_A_FORMS = [(1, 17, 33, 128, 72), (3, 9, 100, 64, 128), (2, 48, 32, 192, 64), (2, 33, 40, 128, 256)]
_A_MULTI = [(24, 96, 128, 64, 64), (10, 104, 96, 64, 128), (20, 64, 96, 128, 64), (20, 100, 70, 64, 64), (12, 100, 70, 64, 136)]
_A_EDGES = [(2, 9, 23, 64, 64), (2, 9, 24, 64, 64), (2, 9, 25, 64, 64),           # the LDS-DMA kernel starts at W = 24
            (2, 1, 40, 64, 64), (1, 2, 33, 64, 72), (3, 1, 1, 64, 64),             # H = 1, H = 2, one pixel
            (2, 5, 1, 64, 64), (1, 1, 23, 8, 8),                                   # W = 1 (register-staged kernel)
            (1, 15, 31, 64, 64), (2, 17, 63, 64, 40), (1, 31, 65, 64, 64), (1, 33, 33, 128, 64), (1, 16, 32, 64, 64),
            (2, 10, 12, 8, 64), (1, 12, 30, 8, 64), (1, 20, 28, 72, 64),           # Cin = 8, Cin = 72: a K tail
            (1, 12, 26, 64, 8), (1, 9, 29, 64, 136)]                               # Cout = 8, 136: a partial cout tile (40 above)
CONV3X3_CASES = ([(s, True) for s in _A_FWD + _A_WGRAD + _A_FORMS + _A_EDGES] + [(s, False) for s in _A_MULTI])
# persistent grid: (blocks, shape) -- many items per block and a short last round on a small tensor
GRID_SHAPE = (3, 40, 70, 64, 72)
GRID_BLOCKS_REFUSED = (1, 2, 3)
GRID_BLOCKS = (8, 9, 11)


def conv3x3_sets(shape, wgrad):
    """value sets of a case: y under S and P, y and the partial sums under T(d)"""
    N, H, W, Cin, Cout = shape
    return [("S", None), ("P", None), ("T", density(N * H * W, 9 * Cin))]


def conv3x3_wgrad_runs(wgrad, vset) -> bool:
    """the weight gradient runs under every set where `wgrad` says the dense sets are exact (64 * pixels < 2^24), and under T(d)
    on every shape: there the bound is pixels * 1 * 1, below 2^24 for the multi-item shapes too"""
    return wgrad or vset == "T"


def conv3x3_build(shape, wgrad, vset, d):
    N, H, W, Cin, Cout = shape
    px = N * H * W
    fast = px * Cin * Cout >= 2 ** 27            # fp32 reference for the large shapes, behind the asserted conditions
    c = conv_case(("conv3x3",) + tuple(shape), vset, (N, Cin, H, W), (Cout, Cin, 3, 3), lambda x, w: F.conv2d(x, w, None, padding=1),
                  9 * Cin, 9 * Cout, px if conv3x3_wgrad_runs(wgrad, vset) else None, stats=(vset == "T"), d=d, fast=fast, bias=True)
    return c


# ------------------------------------------------------------------------------------------------ B: generic implicit GEMM
def dense_sets(pixels, products, dtn, stats=True):
    """value sets of a case for dtype name dtn: S always; P in bf16 always and in fp16 while its outputs (about 8 per product)
    stay finite there (products <= 4096); T(d) where sums are checked"""
    sets = [("S", None)]
    if products <= 4096 or dtn == "bf16":
        sets.append(("P", None))
    if stats:
        sets.append(("T", density(pixels, products)))
    return sets


def out_size(i, k, s, p):
    return (i + 2 * p - k) // s + 1


def _fwd(N, IH, IW, Cin, Cout, k, s, p, act="none", in_extra=0, in_coff=0, out_extra=0, out_coff=0):
    return dict(N=N, IH=IH, IW=IW, Cin=Cin, Cout=Cout, k=k, s=s, p=p, act=act, in_extra=in_extra, in_coff=in_coff,
                out_extra=out_extra, out_coff=out_coff)


def igemm_fuzz_cases(n=10):
    """the first n valid draws of the geometry generator of test_igemm_weight_streaming_fuzz (same seed, same draw order); its
    tanh epilogue is not exact on integers and is drawn as no activation"""
    import random
    rng = random.Random(20261004)
    cases = []
    while len(cases) < n:
        rng.choice([0, 1])                                   # the dtype draw of the original: both dtypes run here
        k = rng.choice([1, 2, 3, 4]); s = rng.choice([1, 2]); p = rng.choice([0, 1, 2])
        N = rng.choice([1, 2, 3]); IH = rng.randint(1, 24); IW = rng.randint(1, 24)
        Cin = 64 * rng.randint(1, 6); Cout = 32 * rng.randint(1, 10)
        OH, OW = out_size(IH, k, s, p), out_size(IW, k, s, p)
        if OH < 1 or OW < 1 or p >= k:
            continue
        in_extra, out_extra = rng.choice([0, 64]), rng.choice([0, 32])
        in_coff, out_coff = rng.choice([0, in_extra]), rng.choice([0, out_extra])
        act = rng.choice(["none", "relu", "leaky", "none"])
        cases.append(_fwd(N, IH, IW, Cin, Cout, k, s, p, act, in_extra, in_coff, out_extra, out_coff))
    return cases


IGEMM_FWD_CASES = (
    # 3x3 / s1 / p1 with BatchNorm partials (test_conv3x3_fwd_bn_partials), bias + ReLU on the first launch
    [_fwd(N, H, W, Cin, Cout, 3, 1, 1, "relu") for (N, H, W, Cin, Cout) in
     [(2, 13, 9, 64, 64), (1, 16, 16, 128, 192), (3, 7, 20, 72, 40), (1, 32, 32, 256, 128), (2, 21, 17, 8, 128), (1, 5, 6, 8, 72)]]
    # 4x4 / s2 / p1, bias + LeakyReLU, channel-sliced input and output (test_conv_strided_io_bias_act)
    + [_fwd(2, 12, 10, 64, 96, 4, 2, 1, "leaky", 16, 8, 32, 32)]
    # split-K / weight-streaming shapes (test_igemm_split_k_skinny)
    + [_fwd(N, h, h, Cin, Cout, k, s, p, "leaky") for (N, h, Cin, Cout, k, s, p) in
       [(2, 2, 512, 512, 4, 2, 1), (2, 4, 512, 256, 4, 2, 1), (1, 8, 1024, 128, 3, 1, 1), (2, 16, 512, 512, 4, 2, 1),
        (2, 12, 256, 384, 4, 2, 1), (3, 5, 192, 256, 3, 1, 1), (2, 16, 320, 192, 4, 2, 1)]]
    + igemm_fuzz_cases(10))


def fwd_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if v not in (0, "none"))


def igemm_fwd_sets(c, dtn):
    OH, OW = out_size(c["IH"], c["k"], c["s"], c["p"]), out_size(c["IW"], c["k"], c["s"], c["p"])
    return dense_sets(c["N"] * OH * OW, c["k"] ** 2 * c["Cin"], dtn)


def igemm_fwd_build(cid, vset, d):
    c = dict(cid)
    return conv_case(("igemm",) + tuple(cid), vset, (c["N"], c["Cin"], c["IH"], c["IW"]), (c["Cout"], c["Cin"], c["k"], c["k"]),
                     lambda x, w: F.conv2d(x, w, None, stride=c["s"], padding=c["p"]), c["k"] ** 2 * c["Cin"], stats=(vset == "T"),
                     d=d, bias=True)


# gradients: (N, h, w, Cin, Cout, k, s, p, single_pass) -- data gradient (s1: one launch of the flipped geometry; s2: the four
# sub-pixel classes, single and batched), weight gradient atomic / assigned (single_pass: what gs_conv_wgrad_single_pass must
# answer -- few-pixel layers, at most 64 logical pixels here, are not split over K) / deterministic
IGEMM_GRAD_CASES = [(2, 13, 9, 64, 64, 3, 1, 1, False), (1, 16, 16, 128, 192, 3, 1, 1, False), (2, 8, 8, 256, 64, 3, 1, 1, False),
                    (3, 9, 5, 72, 40, 3, 1, 1, False),
                    (2, 96, 80, 64, 64, 3, 1, 1, False),                       # test_wgrad_large_k_split
                    (2, 4, 4, 128, 256, 4, 2, 1, True), (2, 8, 8, 512, 512, 4, 2, 1, True), (1, 3, 3, 64, 72, 3, 1, 1, True),
                    (2, 12, 10, 64, 96, 4, 2, 1, True), (8, 64, 64, 64, 64, 3, 1, 1, False)]


def igemm_grad_build(case, vset, d=None):
    N, h, w, Cin, Cout, k, s, p, _ = case
    OH, OW = out_size(h, k, s, p), out_size(w, k, s, p)
    return conv_case(("igemm_grad",) + tuple(case), vset, (N, Cin, h, w), (Cout, Cin, k, k),
                     lambda x, wt: F.conv2d(x, wt, None, stride=s, padding=p), k * k * Cin, k * k * Cout, N * OH * OW,
                     fast=N * h * w * Cin * Cout >= 2 ** 27)


# transposed conv k / s2 / pad through its four sub-pixel classes (geom_convT_class), single and batched, + the batched
# deterministic weight gradient: (N, h, Cin, Cout, k, pad)
CONVT_CASES = [(2, 4, 128, 64, 4, 1), (2, 5, 64, 72, 4, 1), (2, 8, 256, 128, 8, 3), (2, 2, 512, 256, 8, 3), (8, 32, 64, 64, 8, 3)]


def convt_sets(case, dtn):
    N, h, Cin, Cout, k, pad = case
    return dense_sets(N * h * h, (k // 2) ** 2 * Cin, dtn)         # per class: (k/2)^2 taps, N*h*h pixels


def convt_build(case, vset, d=None):
    N, h, Cin, Cout, k, pad = case
    c = conv_case(("convT",) + tuple(case), vset, (N, Cin, h, h), (Cin, Cout, k, k),
                  lambda x, wt: F.conv_transpose2d(x, wt, None, stride=2, padding=pad), (k // 2) ** 2 * Cin, None, N * h * h,
                  d=d, bias=True)
    if vset == "T":                                            # per class sums over the class's pixels
        c["cls_sums"] = [require_channel_sums(c["y"][:, :, (cls >> 1)::2, (cls & 1)::2]) for cls in range(4)]
    return c



# ------------------------------------------------------------------------------------------------ C: ConvTranspose 2x2 / s2
def pow2(v):
    return v > 0 and v & (v - 1) == 0


def upconv_dma_fwd_shape(N, h, w, Cin, Cout):
    """shapes the LDS-DMA pointwise GEMM takes (csrc/pwgemm.hip; include/gsseg.h at gs_upconv2x2_dgrad states the same rule)"""
    return pow2(h) and pow2(w) and (N * h * w) % 256 == 0 and Cin % 128 == 0 and Cout % 64 == 0


def upconv_dma_wgrad_shape(N, h, w, Cin, Cout):
    """include/gsseg.h at gs_upconv2x2_wgrad_slabs: power-of-two maps, IW >= 16, Cin % 128 == 0, Cout % 64 == 0"""
    return Cout % 64 == 0 and pow2(h) and pow2(w) and w >= 16 and Cin % 128 == 0


# (N, h, w, Cin, Cout, (pad_y, pad_x)): the F.pad of unet_parts.py:58-61 puts the up-sampled map at (pad // 2) of a 2h+pad map
UPCONV_FWD_CASES = [(2, 5, 6, 128, 64, (0, 0)), (2, 5, 6, 128, 64, (1, 1)), (1, 16, 16, 1024, 512, (0, 0)), (3, 7, 3, 64, 8, (2, 3)),
                    (2, 8, 16, 128, 64, (0, 0)), (4, 16, 8, 256, 192, (2, 2)), (8, 32, 32, 128, 64, (1, 0)), (1, 16, 16, 384, 128, (0, 0))]
UPCONV_DGRAD_CASES = [(2, 8, 16, 128, 64, (0, 0)), (4, 16, 8, 256, 192, (2, 2)), (8, 32, 32, 128, 64, (1, 0)),
                      (1, 16, 16, 384, 128, (0, 0)), (2, 5, 6, 128, 64, (1, 1))]
# ... + pair: the layer input is the hi plane of a [hi | lo] buffer
UPCONV_WGRAD_CASES = [(2, 16, 16, 128, 64, (0, 0), False), (4, 32, 64, 256, 128, (0, 0), True), (3, 64, 32, 128, 64, (2, 2), False),
                      (8, 16, 16, 1024, 512, (0, 0), False), (1, 8, 16, 256, 192, (1, 1), False), (2, 5, 6, 128, 64, (0, 0), False)]


def upconv_build(case, vset, grads):
    """grads: "" (forward only), "x" or "w" """
    N, h, w, Cin, Cout, pad = case[:6]
    pt, pl = pad[0] // 2, pad[1] // 2

    def fn(x, wt):
        return F.pad(F.conv_transpose2d(x, wt, None, stride=2), [pl, pad[1] - pl, pt, pad[0] - pt])
    c = conv_case(("upconv",) + tuple(case[:6]), vset, (N, Cin, h, w), (Cin, Cout, 2, 2), fn, Cin, 4 * Cout if grads == "x" else None,
                  N * h * w if grads == "w" else None, fast=N * h * w * Cin * Cout >= 2 ** 26, bias=True)
    inner = torch.zeros_like(c["y"], dtype=torch.bool)
    inner[:, :, pt:pt + 2 * h, pl:pl + 2 * w] = True
    c["inner"] = inner
    return c


# ------------------------------------------------------------------------------------------------ D: 3-D
# (NB, D, H, W, Cin, Cout): the shapes of test_conv3d_3x3x3_halo_fwd_dgrad_wgrad, then D = 1 and D = 2 with two volumes (depth taps
# must not leak across volumes) and one shape the LDS-DMA kernel takes
CONV3D_CASES = [(1, 4, 8, 8, 64, 64), (2, 3, 9, 13, 128, 72), (1, 1, 16, 16, 64, 8), (1, 5, 33, 20, 192, 64), (1, 4, 12, 12, 32, 64),
                (1, 3, 8, 8, 72, 32), (2, 1, 9, 11, 64, 64), (2, 2, 9, 11, 64, 64), (2, 2, 8, 32, 64, 64), (3, 2, 5, 40, 64, 72)]


def conv3d_sets(case):
    NB, D, H, W, Cin, Cout = case
    return [("S", None), ("P", None), ("T", density(NB * D * H * W, 27 * Cin))]


def conv3d_build(case, vset, d=None):
    NB, D, H, W, Cin, Cout = case
    return conv_case(("conv3d",) + tuple(case), vset, (NB, Cin, D, H, W), (Cout, Cin, 3, 3, 3), lambda x, w: F.conv3d(x, w, None, padding=1),
                     27 * Cin, 27 * Cout, NB * D * H * W, stats=(vset == "T"), d=d)


# ConvTranspose3d(k2, s2): (N, D, h, w, Cin, Cout); the first on the merged kernel, the others on the LDS-DMA GEMM
UPCONV3D_CASES = [(2, 3, 4, 5, 64, 64), (1, 4, 8, 8, 128, 64), (2, 2, 8, 16, 256, 128), (1, 8, 16, 16, 128, 128)]


def upconv3d_build(case, vset):
    N, D, h, w, Cin, Cout = case
    return conv_case(("upconv3d",) + tuple(case), vset, (N, Cin, D, h, w), (Cin, Cout, 2, 2, 2),
                     lambda x, wt: F.conv_transpose3d(x, wt, None, stride=2), Cin, bias=True)


# ------------------------------------------------------------------------------------------------ E: ends of the nets, reductions
# direct small-Cin convolution (fp32 NCHW image, fp32 weight): (Cin, k, s, p, bias, H, W); N = 2, Cout = 64
SMALLCIN_CASES = [(Cin, k, s, p, bias, H, W) for (Cin, k, s, p, bias) in
                  [(1, 3, 1, 1, False), (1, 3, 1, 1, True), (2, 4, 2, 1, True), (1, 4, 2, 1, False), (3, 3, 1, 1, False)]
                  for (H, W) in [(18, 22), (45, 53)]]


def smallcin_sets(case):
    Cin, k, s, p, bias, H, W = case
    return [("S", None), ("P", None), ("T", density(2 * out_size(H, k, s, p) * out_size(W, k, s, p), k * k * Cin))]


def smallcin_build(case, vset, d=None):
    Cin, k, s, p, bias, H, W = case
    N, Cout = 2, 64
    return conv_case(("smallcin",) + tuple(case), vset, (N, Cin, H, W), (Cout, Cin, k, k),
                     lambda x, w: F.conv2d(x, w, None, stride=s, padding=p), k * k * Cin, k * k * Cout,
                     N * out_size(H, k, s, p) * out_size(W, k, s, p), stats=(vset == "T"), d=d, bias=True)


# small-Cout convolution (the heads): (Cin, Cout, k, p); N, H, W = 2, 11, 9
SMALLCOUT_CASES = [(64, 2, 1, 0), (64, 1, 1, 0), (512, 1, 4, 1)]


def smallcout_build(case, vset):
    Cin, Cout, k, p = case
    N, H, W = 2, 11, 9
    c = conv_case(("smallcout",) + tuple(case), vset, (N, Cin, H, W), (Cout, Cin, k, k), lambda x, w: F.conv2d(x, w, None, padding=p),
                  k * k * Cin, k * k * Cout, N * H * W, bias=True)
    c["db"] = c["dy"].double().sum((0, 2, 3))
    return c


# the one-channel stem whose convolution output is never stored: (N, H, W); image T(1/2), weights dense +-1
STEM_CASES = [(2, 18, 22), (3, 45, 53), (2, 64, 96)]


def stem_build(case):
    """y = conv(x, w) is formed nowhere: the tile partials come from the image's tap sums S and tap Gram matrix G (w.S and
    w^T G w).  With x in {-1, 0, 1} and w in {-1, 1} every G entry is an integer <= pixels and the 81-term form stays below
    81 * pixels < 2^24."""
    N, H, W = case
    g = generator(("stem",) + tuple(case))
    x = draw(g, "T", "a", (N, 1, H, W), 0.5)
    w = draw(g, "T", "w", (64, 1, 3, 3), 1.0)
    require_integers(x, w)
    assert 81 * N * H * W < LIMIT
    y, _ = autograd(lambda a, b: F.conv2d(a, b, None, padding=1), (x, w))
    s1, s2 = require_channel_sums(y, f"stem {case}")
    return {"x": x, "w": w, "y": y, "s1": s1, "s2": s2}


# 1x1 head on relu(y * scale + shift): (N, H, W, ncls); scale a power of two per channel, shift an integer
HEAD_CASES = [(2, 18, 22, 2), (3, 45, 53, 1), (1, 64, 64, 4)]


def head_build(case):
    N, H, W, ncls = case
    g = generator(("head",) + tuple(case))
    y = draw(g, "S", "a", (N, 64, H, W))
    scale = 2.0 ** torch.randint(-1, 2, (64,), generator=g).float()
    shift = draw(g, "S", "a", (64,))
    wh, bh = draw(g, "S", "w", (ncls, 64, 1, 1)), draw(g, "S", "a", (ncls,))
    dl = draw(g, "S", "a", (N, ncls, H, W))
    require_integers(y, shift, wh, bh, dl)
    for s in scale.tolist():
        require_pow2(s)
    zmax = 8 * 2 + 8                                                     # |y * scale + shift|, a multiple of 1/2
    assert 2 * (64 * zmax * 4 + 8) < LIMIT and 2 * N * H * W * 8 * zmax < LIMIT

    def fn(wh_, bh_):
        z = F.relu(y.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
        return F.conv2d(z, wh_, bh_)
    logits, (dw, db) = autograd(fn, (wh, bh), dl)
    return {"y": y, "scale": scale, "shift": shift, "wh": wh, "bh": bh, "dl": dl, "logits": logits, "dw": dw, "db": db}


# column sums of a sub-rectangle of a channel slice: (N, H, W, stride, coff, C, y0, x0, h, w, gscale)
COLSUM_CASES = [(2, 11, 13, 128, 64, 64, 0, 0, 10, 12, 1.0), (2, 11, 13, 128, 64, 64, 1, 1, 10, 12, 0.5), (3, 64, 64, 72, 8, 64, 0, 0, 64, 64, 0.25),
                (1, 17, 9, 16, 8, 8, 1, 0, 16, 8, 2.0), (2, 160, 160, 128, 64, 64, 0, 0, 160, 160, 0.5)]
# column sums out of tile partials: (ntiles, Cfull, coff, C, gscale)
PARTIALS_COLSUM_CASES = [(1, 64, 32, 32, 0.5), (7, 128, 64, 64, 1.0), (300, 128, 0, 128, 0.25), (1200, 64, 32, 32, 0.5), (33, 72, 8, 64, 2.0)]
# the up-conv bias gradient out of the partials of the data-gradient convolution: (N, H, W, Cin, Cout), set T(d)
BIAS_FROM_DGRAD_CASES = [(2, 32, 32, 128, 64), (2, 160, 160, 128, 64), (1, 16, 16, 64, 64)]


def bias_from_dgrad_build(case):
    N, H, W, Cin, Cout = case
    d = density(N * H * W, 9 * Cout)
    g = generator(("bias_from_dgrad",) + tuple(case))
    w = draw(g, "T", "w", (Cout, Cin, 3, 3), d)
    dy = draw(g, "T", "a", (N, Cout, H, W), d)
    require_integers(w, dy)
    require_products(9 * Cout, dy, w)
    dx, _ = autograd(lambda a, b: F.conv_transpose2d(a, b, None, padding=1), (dy, w), None, torch.float32)   # = the data gradient
    s1, s2 = require_channel_sums(dx, f"bias_from_dgrad {case}")
    assert float(dx.abs().max()) <= 256                                   # the stored 16-bit tensor holds dx exactly (bf16 too)
    return {"w": w, "dy": dy, "dx": dx, "s1": s1, "s2": s2, "d": d}


# max pooling with many ties: values from a set of three or four integers
MAXPOOL2D_CASES = [(2, 16, 24, 64, 0), (1, 17, 9, 72, 8), (3, 64, 64, 128, 128)]          # (N, H, W, C, extra channels)
MAXPOOL3D_CASES = [(2, 6, 5, 8, 16), (1, 4, 6, 8, 64), (2, 2, 4, 10, 32), (1, 8, 8, 8, 128)]      # (NB, D, H, W, C)
POOL_ROUTE_CASES = [(2, 8, 6, 64), (2, 9, 7, 64), (1, 4, 4, 1024), (3, 5, 5, 128)]          # (N, H, W, C)


def tied_values(g, shape, values):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), tuple(shape), generator=g)]


def maxpool3d_build(case):
    NB, D, H, W, C = case
    g = generator(("maxpool3d",) + tuple(case))
    z = tied_values(g, (NB, C, D, H, W), (0, 1, 2))
    dzp = draw(g, "S", "a", (NB, C, D // 2, H // 2, W // 2))
    dres = draw(g, "S", "a", (NB, C, D, H, W))
    zp, (routed,) = autograd(lambda a: F.max_pool3d(a, 2), (z,), dzp)
    zw = z.unfold(2, 2, 2).unfold(3, 2, 2).unfold(4, 2, 2)                # [NB, C, D/2, H/2, W/2, 2, 2, 2]
    ties = float(((zw == zw.amax((-3, -2, -1), keepdim=True)).sum((-3, -2, -1)) > 1).double().mean())
    return {"z": z, "dzp": dzp, "dres": dres, "zp": zp, "dz": routed + dres.double(), "ties": ties}


def pool_route_build(case):
    """y integer with ties among the positive values and a positive value in every pooled window; z = relu(y); the gradient
    of sum(z * dz) + sum(max_pool2d(z) * dzp) with respect to y: dy = dz * act'(y) + dzp routed to the first maximum"""
    N, H, W, C = case
    g = generator(("pool_route",) + tuple(case))
    y = tied_values(g, (N, C, H, W), (-2, 1, 2, 3))
    win = y[:, :, :H // 2 * 2, :W // 2 * 2]
    dead = F.max_pool2d(win, 2) < 0
    y[:, :, 1:H // 2 * 2:2, 1:W // 2 * 2:2][dead] = 1.0                  # a window of negatives gets a positive last element
    dz = draw(g, "S", "a", (N, C, H, W))
    dzp = draw(g, "S", "a", (N, C, H // 2, W // 2))
    yl = y.double().requires_grad_(True)
    z = F.relu(yl)
    ((z * dz.double()).sum() + (F.max_pool2d(z, 2) * dzp.double()).sum()).backward()
    assert float(F.max_pool2d(y[:, :, :H // 2 * 2, :W // 2 * 2], 2).min()) > 0
    return {"y": y, "dz": dz, "dzp": dzp, "dy": yl.grad.detach()}


# ------------------------------------------------------------------------------------------------ F: Pix2Pix packs
SOFTMAX3 = (0.5, 0.25, 0.25)                                 # dyadic architecture weights of W4, W6, W8
MERGE_CASES = [(128, 64), (64, 8), (32, 72)]                 # (Cin, Cout)
SPLIT_CASES = [(64, 64, 1), (64, 64, 4), (32, 8, 3), (96, 40, 1)]      # (Cin, Cout, nparts)
IMAGE_FWD_CASES = [(2, 16, 24, 128, 1), (1, 9, 20, 64, 3), (3, 8, 8, 128, 1)]       # (N, h, w, Cin, Cout)
IMAGE_WGRAD_CASES = [(2, 16, 24, 128), (1, 9, 70, 128), (3, 8, 8, 256)]             # (N, h, w, Cin)


def class_tap_of(ky, kx):
    """(class, tap) of kernel element (ky, kx) of the merged 8x8 / s2 / p3 transposed conv (include/gsseg.h: class = py*2+px,
    tap = a*4+b with ky = 2a+1-py, kx = 2b+1-px)"""
    py, px = 1 - ky % 2, 1 - kx % 2
    return py * 2 + px, ((ky - 1 + py) // 2) * 4 + (kx - 1 + px) // 2


def merged_to_classes(wm: torch.Tensor) -> torch.Tensor:
    """[Cin][Cout][8][8] -> [4][16][Cout][Cin]"""
    out = torch.empty(4, 16, wm.shape[1], wm.shape[0], dtype=wm.dtype)
    for ky in range(8):
        for kx in range(8):
            c, t = class_tap_of(ky, kx)
            out[c, t] = wm[:, :, ky, kx].t()
    return out


def classes_to_merged(pc: torch.Tensor) -> torch.Tensor:
    wm = torch.empty(pc.shape[3], pc.shape[2], 8, 8, dtype=pc.dtype)
    for ky in range(8):
        for kx in range(8):
            c, t = class_tap_of(ky, kx)
            wm[:, :, ky, kx] = pc[c, t].t()
    return wm


def merge_build(case):
    Cin, Cout = case[:2]
    g = generator(("merge",) + tuple(case))
    w4, w6, w8 = (draw(g, "S", "w", (Cin, Cout, k, k)) for k in (4, 6, 8))
    require_integers(w4, w6, w8)
    for s in SOFTMAX3:
        require_pow2(s)
    wm = SOFTMAX3[2] * w8.double() + SOFTMAX3[1] * F.pad(w6.double(), (1, 1, 1, 1)) + SOFTMAX3[0] * F.pad(w4.double(), (2, 2, 2, 2))
    return {"w4": w4, "w6": w6, "w8": w8, "wm": wm}


def split_build(case):
    """dwm = the sum of nparts integer slabs; dots: Cin * Cout * k^2 products of |dwm| <= 8 and |w| <= 4 below 2^24"""
    Cin, Cout, nparts = case
    r = merge_build(case)
    g = generator(("split",) + tuple(case))
    lo = 8 // nparts
    slabs = torch.randint(-lo, lo + 1, (nparts, 4, 16, Cout, Cin), generator=g).float()
    dwm = slabs.double().sum(0)
    assert Cin * Cout * 64 * float(dwm.abs().max()) * 4 < LIMIT
    dm = classes_to_merged(dwm)                                            # [Cin][Cout][8][8]
    wins = {4: dm[:, :, 2:6, 2:6], 6: dm[:, :, 1:7, 1:7], 8: dm}
    r.update(slabs=slabs, dwm=dwm, wins=wins,
             dots=torch.stack([(wins[k] * r[f"w{k}"].double()).sum() for k in (4, 6, 8)]))
    return r


def image_fwd_build(case):
    N, h, w, Cin, Cout = case
    g = generator(("image_fwd",) + tuple(case))
    x = draw(g, "S", "a", (N, Cin, h, w))
    wm = draw(g, "S", "w", (Cin, Cout, 8, 8))
    b = draw(g, "S", "a", (Cout,))
    require_integers(x, wm, b)
    require_products(16 * Cin + 1, x, wm)
    y, _ = autograd(lambda a, c: F.conv_transpose2d(a, c, None, stride=2, padding=3), (x, wm))
    wpad = torch.zeros(Cin, 8, 8, 8)
    wpad[:, :Cout] = wm
    return {"x": x, "wm": wm, "b": b, "y": y + b.double().view(1, -1, 1, 1), "pack": merged_to_classes(wpad)}


def image_wgrad_build(case):
    N, h, w, Cin = case
    g = generator(("image_wgrad",) + tuple(case))
    x = draw(g, "S", "a", (N, Cin, h, w))
    du = draw(g, "S", "a", (N, 1, 2 * h, 2 * w))
    require_integers(x, du)
    require_products(N * h * w, x, du)
    wm = torch.zeros(Cin, 1, 8, 8)
    _, (_, dwm) = autograd(lambda a, c: F.conv_transpose2d(a, c, None, stride=2, padding=3), (x, wm), du, wrt=[1])
    return {"x": x, "du": du, "dwm": merged_to_classes(dwm)}


# ------------------------------------------------------------------------------------------------ G: BatchNorm / activation
# csrc/bn.hip stated without tiles or lanes, in fp64:
#   forward   z = act(y * scale + shift) [* (keep ? keep_scale : 0)], rounded ONCE to the 16-bit dtype; the pooled output is
#             the max over the ROUNDED z of every complete 2x2 window
#   backward  v = y * scale + shift;  gh = (keep * dz_a + dzp routed to the first maximum of the rounded z) * act'(v) + dz_b * act_b'(v)
#             s1 = sum gh, s2 = sum gh * xh with xh = (y - mean) * invstd;  dy = bn ? scale * (gh - c1 - xh * c2) : gh
#             act'(0): ReLU 0, LeakyReLU 0.2 (v > 0 ? 1 : slope)
# Operands: y integers of range S (times 5 under LeakyReLU), mean small integers, invstd and |gamma| powers of two (gamma
# negative on every third channel), shift integers (near 300 and 2100 on a quarter of the channels each, so that z rounds in
# bf16 and in fp16 and the rounding makes ties), c1 / c2 multiples of 1/4, keep bytes from {0, 1, 255}, keep_scale 2.
KEEP_SCALE = 2.0
BN_LARGE = 32768                    # pixels from which the gradients are drawn sparse, T(d) times the multiplier
BN_MUTANTS = ("relu0", "last", "keep_on_b", "slope_b", "unrounded", "drop63")


def require_dyadic(t: torch.Tensor, what: str = "", max_bits: int = 8) -> int:
    """every element is a multiple of 2^-k for a k <= max_bits and |t| * 2^k < 2^24: t is an fp32 number.  Returns that k."""
    td = t.double()
    for k in range(max_bits + 1):
        s = td * 2.0 ** k
        if torch.equal(s, s.round()):
            assert float(s.abs().max()) < LIMIT if s.numel() else True, f"{what}: {float(s.abs().max())} * 2^-{k} has more than 24 bits"
            return k
    raise AssertionError(f"{what}: not a multiple of 2^-{max_bits}")


def require_fifths(*tensors):
    """LeakyReLU(0.2) operands: x / 5 is a dyadic number and float32(x) * float32(0.2) is exactly that number (true for every
    multiple of 5, or of 5 * 2^-k, in the ranges used here; false for general integers), so the slope needs no allowance."""
    slope = torch.tensor(0.2, dtype=torch.float32)
    for t in tensors:
        q = t.double() / 5
        require_dyadic(q, "x / 5", 4)
        assert torch.equal((t.float() * slope).double(), q), "float32(x) * float32(0.2) is not the exact x / 5"


def act_fwd64(v: torch.Tensor, act: str) -> torch.Tensor:
    if act == "none":
        return v
    return torch.where(v > 0, v, torch.zeros_like(v) if act == "relu" else v / 5)


def act_bwd64(g: torch.Tensor, v: torch.Tensor, act: str, relu_at_0: float = 0.0) -> torch.Tensor:
    """g * act'(v) with act'(0) = 0 for ReLU (relu_at_0: the mutant's value) and 0.2 for LeakyReLU"""
    if act == "none":
        return g
    if act == "relu":
        return torch.where(v > 0, g, torch.where(v == 0, g * relu_at_0, torch.zeros_like(g)))
    return torch.where(v > 0, g, g / 5)


def route_pool2(zr: torch.Tensor, dzp: torch.Tensor, last: bool = False):
    """dzp [N, C, H/2, W/2] routed to the first (last: the mutant) maximum of every complete 2x2 window of zr [N, C, H, W] in
    scan order (0,0) (0,1) (1,0) (1,1).  Returns the routed gradient [N, C, H, W] and the share of windows with a tied maximum."""
    N, C, H, W = zr.shape
    PH, PW = H // 2, W // 2
    win = zr[:, :, :2 * PH, :2 * PW].reshape(N, C, PH, 2, PW, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, PH, PW, 4)
    is_max = win == win.amax(-1, keepdim=True) if win.numel() else torch.zeros_like(win, dtype=torch.bool)
    order = is_max.flip(-1) if last else is_max
    pick = order & (order.cumsum(-1) == 1)
    if last:
        pick = pick.flip(-1)
    routed = pick * dzp.double().unsqueeze(-1)
    out = torch.zeros_like(zr, dtype=torch.float64)
    out[:, :, :2 * PH, :2 * PW] = routed.reshape(N, C, PH, PW, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * PH, 2 * PW)
    ties = float((is_max.sum(-1) > 1).double().mean()) if win.numel() else 0.0
    return out, ties


def _bnv(act="relu", dza="slice", dzb=None, keep=False, bn=True, ident=False):
    return dict(act=act, dza=dza, dzb=dzb, keep=keep, bn=bn, ident=ident)


# dza: "slice" (channels [C, 2C) of a 2C-wide buffer, poison outside), "dense" or None; dzb: None or its activation act_b
BN_VARIANTS = {
    "relu": _bnv(),
    "none_dense": _bnv(act="none", dza="dense"),
    "leaky": _bnv(act="leaky"),
    "b_only": _bnv(dza=None, dzb="none"),
    "b_leaky": _bnv(dza="dense", dzb="leaky"),                    # the Pix2Pix down path
    "keep_b": _bnv(keep=True, dzb="none"),                        # the mask must not touch dz_b
    "keep_b_leaky": _bnv(dza="dense", keep=True, dzb="leaky"),
    "keep_bn0": _bnv(act="none", dza="dense", keep=True, bn=False),
    "ident": _bnv(dza="dense", bn=False, ident=True),             # scale / shift NULL
    "leaky_bn0": _bnv(act="leaky", dza="dense", bn=False),
    "pool_only": _bnv(dza=None),                                  # pooled shapes: dzp is the only source
}
_BN_PLAIN = [v for v in BN_VARIANTS if v != "pool_only"]
_BN_POOLED = [v for v, s in BN_VARIANTS.items() if s["dzb"] is None and not s["keep"]]
BN_SHAPES = [(1, 1, 1, 8), (2, 9, 7, 24), (2, 33, 31, 72), (2, 64, 64, 64), (1, 5, 5, 1024), (1, 4, 4, 2048), (1, 192, 192, 8),
             (3, 160, 150, 8)]
BN_FULL_SHAPES = [(2, 9, 7, 24), (2, 64, 64, 64), (3, 160, 150, 8)]             # every variant
BN_POOLED_SHAPES = [(2, 9, 7, 64), (1, 65, 33, 128), (2, 64, 64, 64)]            # every variant that is legal with a pool
BN_TWO_STAGE_SHAPES = [(1, 192, 192, 8), (3, 160, 150, 8)]                      # more than 512 tiles (576 and 1015): gs_bn_bwd_coeffs in two stages
# (shape, pooled, variant): the other plain shapes run "relu" and one more variant each, in turn
BN_CASES = ([(s, False, v) for s in BN_FULL_SHAPES for v in _BN_PLAIN]
            + [(s, False, v) for i, s in enumerate(x for x in BN_SHAPES if x not in BN_FULL_SHAPES)
               for v in ("relu", [x for x in _BN_PLAIN if x != "relu"][(2 * i) % (len(_BN_PLAIN) - 1)])]
            + [(s, True, v) for s in BN_POOLED_SHAPES for v in _BN_POOLED])
BN_FWD_ONLY_CASES = [((2, 96, 96, 512), False, "leaky"), ((2, 96, 96, 512), False, "keep_bn0")]
BN_HEAD_CASES = [(2, 18, 22, 64, 2), (3, 45, 53, 64, 1), (2, 40, 40, 32, 4)]
BN_HEAD_TWO_CHUNKS = (1, 1472, 1472, 8, 3)                    # fp16 only: 2116 pixels per tile, a second LDS chunk of 68
BN_REV_CASES = [((2, 9, 7, 24), False, "keep_b_leaky"), ((2, 33, 31, 72), False, "relu"), ((2, 9, 7, 64), True, "leaky")]


def _bn_density(pixels, act, fan=1):
    """gradient density of a case.  Target: per channel, sum over the pixels of |gh| * |xh| in units of its last bit < 2^24 (the
    s2 condition of _bn_finish; s1 is the weaker one).  Dense below BN_LARGE weighted pixels, density() of them from there on:
      weight = 4 * fan   act = LeakyReLU: y and the gradients both carry the factor 5, so the products |gh * xh| are larger
      weight = fan / 4   otherwise (a LeakyReLU on act_b alone puts the 5 on the gradients only; y keeps its range)
      fan                1 for tensor sources; the head source sums `classes` products with |w_head| up to 4.
    The weights are rough on purpose: density() moves in steps of 4 in the sum it bounds.
    This only picks a starting point: _bn_finish proves every choice on the operands with require_channel_sums, and a choice
    that were too dense fails there, on the CPU."""
    weight = 4 * fan if act == "leaky" else max(1, fan // 4)
    return density(pixels * weight, 2048) if pixels * weight >= BN_LARGE else None


def bn_pixel63(shape, pooled=False):
    """(n, y, x) of pixel 63 of an [N, H, W, C] tensor -- the last of the first 64-pixel run -- or of its 2x2 window"""
    N, H, W, C = shape
    n, rem = divmod(63, H * W)
    yy, xx = divmod(rem, W)
    return (n, yy // 2, xx // 2) if pooled else (n, yy, xx)


def _at63(shape, pooled=False):
    """index of channel 0 of pixel 63 (of its window) in an NCHW operand"""
    n, yy, xx = bn_pixel63(shape, pooled)
    return (n, 0, yy, xx)


def bn_id(case):
    shape, pooled, v = case
    return "x".join(str(i) for i in shape) + ("-pool-" if pooled else "-") + v


def _bn_operands(g, shape, act, ident):
    """y and the per-channel coefficients of one case; zeros of v planted on the channels c % 4 == 0 (|scale| = 1 there)"""
    N, H, W, C = shape
    m = 5.0 if act == "leaky" else 1.0
    c = torch.arange(C)
    invstd = 2.0 ** torch.randint(-1, 2, (C,), generator=g).double()
    gmag = torch.where(c % 4 == 0, 1.0 / invstd, 2.0 ** torch.randint(-1, 2, (C,), generator=g).double())
    sign = torch.where(c % 3 == 1, -1.0, 1.0).double()
    small = torch.randint(-2, 3, (C,), generator=g).double()
    shift = (small + torch.where(c % 4 == 1, 300.0, 0.0) + torch.where(c % 4 == 2, 2100.0, 0.0)) * m
    scale = sign * gmag * invstd
    mean = torch.randint(-2, 3, (C,), generator=g).double()
    c1 = torch.randint(-16, 17, (C,), generator=g).double() / 4
    c2 = torch.randint(-16, 17, (C,), generator=g).double() / 4
    y = tied_values(g, (N, C, H, W), tuple(range(-8, 9))).double() * m
    if not ident:
        plant = (torch.rand((N, C, H, W), generator=g) < 0.125)
        plant[0, :, 0, 0] = True
        plant &= (c % 4 == 0).view(1, -1, 1, 1)
        y = torch.where(plant, (-shift * sign).view(1, -1, 1, 1).expand_as(y), y)
    if N * H * W >= 64:
        y[_at63(shape)] = 8.0 * m           # pixel 63, channel 0 (scale +1): v > 0, the largest z of its window
    require_integers(y, mean)
    assert torch.equal(shift, shift.round())
    for t in (invstd, gmag):
        for s in t.unique().tolist():
            require_pow2(s)
    assert float(c1.abs().max()) <= 4 and float(c2.abs().max()) <= 4 and require_dyadic(torch.cat([c1, c2])) <= 2
    out = {"y": y.float(), "mean": mean.float(), "invstd": invstd.float(), "c1": c1.float(), "c2": c2.float(),
           "scale": None if ident else scale.float(), "shift": None if ident else shift.float(), "gamma_negative": int((sign < 0).sum())}
    return out


def _col(t, C, default):
    return (torch.full((C,), default, dtype=torch.float64) if t is None else t.double()).view(1, -1, 1, 1)


def _bn_finish(c, what):
    """the conditions every intermediate of the kernel has to meet, asserted on the operands of case c (in place: adds the
    shares of v == 0 and of tied windows)"""
    y = c["y"].double()
    C = y.shape[1]
    scale, shift, mean, invstd = _col(c["scale"], C, 1.0), _col(c["shift"], C, 0.0), _col(c["mean"], C, 0.0), _col(c["invstd"], C, 1.0)
    v = y * scale + shift
    require_dyadic(v, what + " v")
    xh = (y - mean) * invstd
    kx = require_dyadic(xh, what + " xh")
    leaky = "leaky" in (c["act"], c["act_b"] if c["dzb"] is not None else None)
    grads = [t for t in (c["dza"], c["dzb"], c["dzp"]) if t is not None]
    for t in grads:
        require_dyadic(t, what + " gradient operand", 1)
        assert float(t.abs().max()) <= 2560
    if leaky:
        require_fifths(*grads)
    if c["act"] == "leaky":
        require_fifths(c["y"], v)
        if c["shift"] is not None:
            require_fifths(c["shift"])
    require_pow2(c["keep_scale"])
    if c["keep"] is not None:
        assert set(c["keep"].unique().tolist()) <= {0, 1, 255}
    # |gh| <= keep_scale |dz_a| + |dz_b| + |dzp| at ONE pixel of its window: the channel totals of this bound (for s2: times |xh|,
    # the routed part times the largest |xh| of the window) are exact, so every sub-sum a kernel forms is
    bound = torch.zeros_like(y)
    if c["dza"] is not None:
        bound += c["dza"].double().abs() * (c["keep_scale"] if c["keep"] is not None else 1.0)
    if c["dzb"] is not None:
        bound += c["dzb"].double().abs()
    b1, b2 = bound.clone(), bound * xh.abs()
    if c["dzp"] is not None and c["dzp"].numel():
        PH, PW = c["dzp"].shape[2:]
        b1[:, :, 0:2 * PH:2, 0:2 * PW:2] += c["dzp"].double().abs()
        b2[:, :, 0:2 * PH:2, 0:2 * PW:2] += c["dzp"].double().abs() * F.max_pool2d(xh.abs(), 2)
    kg = require_dyadic(b1 / (5.0 if leaky else 1.0), what + " gh")
    require_channel_sums(b1 * 2.0 ** kg, what + " s1", squares=False)
    require_channel_sums(b2 * 2.0 ** (kg + kx), what + " s2", squares=False)
    c["zero_share"] = float((v == 0).double().mean())
    c["tie_share"] = route_pool2(act_fwd64(v, c["act"]), torch.zeros(1), False)[1] if c["pooled"] else 0.0
    return c


def bn_build(shape, pooled, vname):
    """operands of one case of BN_CASES / BN_FWD_ONLY_CASES, NCHW on the CPU; bn_reference gives the expected values"""
    N, H, W, C = shape
    s = BN_VARIANTS[vname]
    g = generator(("bn", tuple(shape), pooled, vname))
    px = N * H * W
    leaky = "leaky" in (s["act"], s["dzb"])
    gm = 5.0 if leaky else 1.0
    d = _bn_density(px, s["act"])

    def grad(shp, pool=False):
        t = (draw(g, "T", "a", shp, d) if d else draw(g, "S", "a", shp)) * gm
        if t.numel():
            t.view(-1)[0] = gm                   # a gradient on the planted v == 0 of pixel 0, channel 0
        if px >= 64:
            t[_at63(shape, pool)] = gm        # and on pixel 63 (its window), where v > 0
        return t
    c = _bn_operands(g, shape, s["act"], s["ident"])
    c.update(act=s["act"], act_b=s["dzb"] or "none", bn=s["bn"], pooled=pooled, dza_kind=s["dza"], keep_scale=KEEP_SCALE, d=d,
             dza=grad((N, C, H, W)) if s["dza"] else None, dzb=grad((N, C, H, W)) if s["dzb"] else None,
             dzp=grad((N, C, H // 2, W // 2), True) if pooled else None, keep=None)
    if s["keep"]:
        assert not pooled
        c["keep"] = torch.tensor([0, 1, 255], dtype=torch.uint8)[torch.randint(0, 3, (N, C, H, W), generator=g)]
        if px >= 64:
            c["keep"][_at63(shape)] = 255
    return _bn_finish(c, bn_id((shape, pooled, vname)))


def bn_head_build(case):
    """the head source: dz_a[p][c] = sum_k dl[n][k][hw] * w_head[k][c] (fp32 in the kernel, never rounded to 16 bits), dl integer
    (multiples of 5 under LeakyReLU, sparse on the large case), w_head powers of two on the even and small integers on the odd
    channels; ReLU for 1 to 3 classes, LeakyReLU for 4"""
    N, H, W, C, ncls = case
    g = generator(("bn_head",) + tuple(case))
    px = N * H * W
    act = "leaky" if ncls == 4 else "relu"
    gm = 5.0 if act == "leaky" else 1.0
    d = _bn_density(px, act, 4 * ncls)
    dl = (draw(g, "T", "a", (N, ncls, H, W), d) if d else draw(g, "S", "a", (N, ncls, H, W))) * gm
    dl[0, :, 0, 0] = gm
    dl[(bn_pixel63((N, H, W, C))[0], slice(None)) + bn_pixel63((N, H, W, C))[1:]] = gm
    wp = (torch.randint(0, 2, (ncls, C), generator=g) * 2 - 1) * 2.0 ** torch.randint(-1, 2, (ncls, C), generator=g).double()
    wi = draw(g, "S", "w", (ncls, C)).double()
    wh = torch.where(torch.arange(C) % 2 == 0, wp, wi)
    wh[:, 0] = 1.0
    require_integers(dl)
    require_dyadic(wh, "w_head", 1)
    assert ncls * float(dl.abs().max()) * float(wh.abs().max()) * 2 < LIMIT        # every partial sum over k, in halves
    dza = torch.einsum("nkhw,kc->nchw", dl.double(), wh)
    c = _bn_operands(g, (N, H, W, C), act, False)
    c.update(act=act, act_b="none", bn=True, pooled=False, dza_kind="head", keep_scale=KEEP_SCALE, d=d, dza=dza, dzb=None, dzp=None,
             keep=None, dl=dl, w_head=wh.float(), ncls=ncls)
    return _bn_finish(c, "head " + "x".join(str(i) for i in case))


def bn_mutant_applies(c, mutant, dt=None) -> bool:
    """whether `mutant` changes what case c asks of the kernel (otherwise it IS the reference there)"""
    pixels = c["y"].shape[0] * c["y"].shape[2] * c["y"].shape[3]
    return {"relu0": c["act"] == "relu" and (c["dza"] is not None or c["pooled"]),
            "last": c["pooled"],
            "keep_on_b": c["keep"] is not None and c["dzb"] is not None,
            "slope_b": c["dzb"] is not None and c["act_b"] != c["act"],
            # without scale / shift z = act(y) holds |y| <= 8 exactly in both dtypes: rounded and unrounded z are the same numbers
            "unrounded": c["pooled"] and c["scale"] is not None,
            "drop63": pixels >= 64}[mutant]


def bn_reference(c, dt, mutant=None):
    """fp64 expected values of case c for the 16-bit dtype dt: z, zp (forward), gh, s1, s2 (tile-free sums) and dy computed with
    the c1 / c2 of the case.  mutant: one of BN_MUTANTS, a reference that is wrong in one stated way (the CPU test shows that the
    comparer tells each from the reference)."""
    assert mutant is None or mutant in BN_MUTANTS
    y = c["y"].double()
    N, C, H, W = y.shape
    scale, shift, mean, invstd = _col(c["scale"], C, 1.0), _col(c["shift"], C, 0.0), _col(c["mean"], C, 0.0), _col(c["invstd"], C, 1.0)
    v = y * scale + shift
    z = act_fwd64(v, c["act"])
    kf = None if c["keep"] is None else torch.where(c["keep"] != 0, c["keep_scale"], 0.0).double()
    out = {"z": expect16(z if kf is None else z * kf, dt)}
    g = torch.zeros_like(y)
    if c["dza"] is not None:
        g = c["dza"].double() if kf is None else c["dza"].double() * kf
    if c["pooled"]:
        zr = out["z"].double()
        out["zp"] = F.max_pool2d(zr, 2).to(dt) if H >= 2 and W >= 2 else zr.new_zeros((N, C, H // 2, W // 2)).to(dt)
        g = g + route_pool2(z if mutant == "unrounded" else zr, c["dzp"], last=(mutant == "last"))[0]
    gh = act_bwd64(g, v, c["act"], 1.0 if mutant == "relu0" else 0.0)
    if c["dzb"] is not None:
        gb = c["dzb"].double()
        if mutant == "keep_on_b":
            gb = gb * kf
        gh = gh + act_bwd64(gb, v, c["act"] if mutant == "slope_b" else c["act_b"])
    if mutant == "drop63":
        flat = gh.permute(0, 2, 3, 1).reshape(-1, C).clone()
        flat[63] = 0                                        # the last pixel of the first 64-pixel run, every channel
        gh = flat.view(N, H, W, C).permute(0, 3, 1, 2)
    xh = (y - mean) * invstd
    out["gh"] = gh
    out["s1"], out["s2"] = gh.sum((0, 2, 3)), (gh * xh).sum((0, 2, 3))
    out["dy"] = scale * (gh - _col(c["c1"], C, 0.0) - xh * _col(c["c2"], C, 0.0)) if c["bn"] else gh
    return out


def bn_fp32_shuffled(c, dt, seed):
    """the backward of case c the way a kernel may form it: every elementwise step in fp32 (v, the slope product, the keep
    factor, xh, the terms, dy), the sums over a random permutation of the pixels in runs of 64 summed in fp32, then the run sums
    in fp32.  Equal to bn_reference bit for bit is what entitles the GPU test to zero tolerance."""
    f = torch.float32
    y = c["y"].to(f)
    N, C, H, W = y.shape
    col = lambda t, dflt: (torch.full((C,), dflt, dtype=f) if t is None else t.to(f)).view(1, -1, 1, 1)     # noqa: E731
    scale, shift, mean, invstd = col(c["scale"], 1.0), col(c["shift"], 0.0), col(c["mean"], 0.0), col(c["invstd"], 1.0)
    slope = {"none": 1.0, "relu": 0.0, "leaky": 0.2}
    sa, sb = torch.tensor(slope[c["act"]], dtype=f), torch.tensor(slope[c["act_b"]], dtype=f)
    one = torch.tensor(1.0, dtype=f)
    v = y * scale + shift
    g = torch.zeros_like(y)
    if c["dza"] is not None:
        g = c["dza"].to(f)
        if c["keep"] is not None:
            g = g * torch.where(c["keep"] != 0, c["keep_scale"], 0.0).to(f)
    if c["pooled"]:
        zr = torch.where(v > 0, v, v * sa).to(dt).double()
        g = g + route_pool2(zr, c["dzp"])[0].to(f)
    gh = g * torch.where(v > 0, one, sa)
    if c["dzb"] is not None:
        gh = gh + c["dzb"].to(f) * torch.where(v > 0, one, sb)
    xh = (y - mean) * invstd
    dy = scale * (gh - col(c["c1"], 0.0) - xh * col(c["c2"], 0.0)) if c["bn"] else gh
    perm = torch.randperm(N * H * W, generator=torch.Generator().manual_seed(seed))
    sums = []
    for t in (gh, gh * xh):
        rows = t.permute(0, 2, 3, 1).reshape(-1, C)[perm]
        acc = torch.zeros(C, dtype=f)
        for run in rows.split(64):
            part = torch.zeros(C, dtype=f)
            for r in run.split(16):
                part = part + r.sum(0, dtype=f)
            acc = acc + part
        sums.append(acc)
    assert v.dtype == gh.dtype == dy.dtype == sums[0].dtype == f
    return {"gh": gh, "s1": sums[0], "s2": sums[1], "dy": dy}


# ---- tanh (the Pix2Pix output layer): not exact; per element, the correctly rounded 16-bit value or its neighbour
TANH_CASES = [((2, 9, 7, 24), False), ((2, 33, 31, 72), False), ((2, 9, 7, 64), True), ((1, 65, 33, 128), True)]     # (shape, pooled)
TANH_NEIGHBOUR_SHARE = 0.01


def tanh_build(shape, pooled):
    """y multiples of 1/8 with |y| <= 1.5 (exact in both dtypes, with ties), integer dz; z = tanh(y), dy = dz * (1 - tanh(y)^2).
    Why |y| <= 1.5: 1 - t^2 cancels, an error e of t becomes 2 t e / (1 - t^2) relative, at most 9 e here."""
    N, H, W, C = shape
    g = generator(("tanh", tuple(shape), pooled))
    y = tied_values(g, (N, C, H, W), tuple(k / 8 for k in range(-12, 13)))
    dz = draw(g, "S", "a", (N, C, H, W))
    t = torch.tanh(y.double())
    return {"y": y, "dz": dz, "z": t, "dy": dz.double() * (1 - t * t)}


def ordered16(t: torch.Tensor) -> torch.Tensor:
    """a 16-bit float tensor as integers whose order is the order of the values (+0 and -0 both 0): neighbours differ by 1"""
    b = t.view(torch.int16).int()
    return torch.where(b < 0, -(b & 0x7FFF), b)


def neighbour16(got: torch.Tensor, ref64: torch.Tensor):
    """(ok, share): ok marks the elements of `got` that are the 16-bit value nearest to the fp64 reference or adjacent to it;
    share is the fraction that sit on the neighbour"""
    want = ref64.to(got.dtype).to(got.device)
    exact = got == want
    ok = exact | ((ordered16(got) - ordered16(want)).abs() <= 1)
    return ok, float((ok & ~exact).double().mean())


# ---- gs_bn_finalize / gs_bn_eval_coeffs against numpy fp64: bounds from the count of fp32 roundings, see the GPU test
BN_FINALIZE_C = (24, 64, 72)
BN_FINALIZE_TILES = (1, 2, 512, 513, 1200)
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
# fp32 roundings on the way to each output of gs_bn_finalize, counted in the docstring of its GPU test
BN_FINALIZE_ROUNDINGS = {"mean": 1, "invstd": 1, "scale": 2, "shift": 5, "rm": 3, "rv": 3}
BN_EVAL_ROUNDINGS = {"mean": 0, "invstd": 3, "scale": 4, "shift": 6}


def bn_finalize_build(C, ntiles, count_one=False):
    """fp32 tile partials [ntiles][2][C] of `ntiles` tiles of 64 pixels (count_one: one tile of one pixel): channel 0 is constant
    (its sum of squares one fp32 step BELOW count * value^2, so the variance comes out negative and must clamp at 0), channel 1 has
    |mean| = 100 * std; gamma, beta and running statistics"""
    import numpy as np
    rng = np.random.default_rng(case_seed(("bn_finalize", C, ntiles, count_one)))
    T = 1 if count_one else 64
    mean = rng.uniform(-2, 2, C)
    std = rng.uniform(0.5, 2, C)
    mean[1], std[1] = 50.0, 0.5
    tm = mean + std * rng.standard_normal((ntiles, C)) / np.sqrt(T)            # tile means
    tv = std ** 2 * rng.uniform(0.5, 1.5, (ntiles, C))                          # tile variances
    if count_one:
        tv[:] = 0.0
    s1 = (T * tm).astype(np.float32)
    s2 = (T * (tv + tm ** 2)).astype(np.float32)
    s1[:, 0] = 3.0 * T
    s2[:, 0] = np.nextafter(np.float32(9.0 * T), np.float32(0))
    part = np.stack([s1, s2], 1)
    return {"partials": torch.from_numpy(part), "count": float(ntiles * T),
            "gamma": torch.from_numpy(rng.uniform(-2, 2, C).astype(np.float32)), "beta": torch.from_numpy(rng.uniform(-1, 1, C).astype(np.float32)),
            "rm": torch.from_numpy(rng.uniform(-1, 1, C).astype(np.float32)), "rv": torch.from_numpy(rng.uniform(0.5, 2, C).astype(np.float32))}


def bn_finalize_reference(r, with_affine=True):
    """numpy fp64 from the fp32 partials: the outputs of gs_bn_finalize and, per output, the sum of the magnitudes of its terms
    (what one fp32 rounding of that output is relative to)"""
    import numpy as np
    p = r["partials"].numpy().astype(np.float64)
    n, count = p.shape[0], r["count"]
    C = p.shape[2]
    gamma = r["gamma"].numpy().astype(np.float64) if with_affine else np.ones(C)
    beta = r["beta"].numpy().astype(np.float64) if with_affine else np.zeros(C)
    rm, rv = r["rm"].numpy().astype(np.float64), r["rv"].numpy().astype(np.float64)
    eps, mom = float(np.float32(BN_EPS)), float(np.float32(BN_MOMENTUM))
    S1, S2 = p[:, 0].sum(0), p[:, 1].sum(0)
    mean = S1 / count
    raw = S2 / count - mean * mean
    var = np.maximum(raw, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    unb = var * (count / (count - 1.0)) if count > 1 else var
    keep = float(np.float32(1.0) - np.float32(BN_MOMENTUM))
    return {"mean": mean, "invstd": invstd, "scale": scale, "shift": beta - mean * scale, "rm": keep * rm + mom * mean, "rv": keep * rv + mom * unb,
            "raw_var": raw,
            "mag": {"mean": np.abs(mean), "invstd": invstd, "scale": np.abs(scale), "shift": np.abs(beta) + np.abs(mean * scale),
                    "rm": np.abs(keep * rm) + np.abs(mom * mean), "rv": np.abs(keep * rv) + np.abs(mom * unb)}}


def coeff_bound(ref, name, roundings):
    """the largest |error| of output `name`: roundings[name] fp32 roundings, each at most 2^-24 of the magnitudes of its terms"""
    return ref["mag"][name] * (roundings[name] * 2.0 ** -24)
