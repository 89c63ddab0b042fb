"""fp64 reference of the hi/lo pair forward, in plain torch on the CPU (no GPU, no native library).

A pair kernel computes a dot product of 16-bit values accumulated in fp32: per output element
    y[co] = sum over taps t and K indices k of  x[pixel + tap t][channel(k)] * pack[t][co][k]
where the K extent walks the input channels [0, wrap) of the kernel's window and wraps once (k_channels), and the pack
holds, per segment, the hi halves, the lo halves or zeros of a channel range of the fp32 weight (expected_pack).  The
functions below state exactly that in fp64 on the 16-bit values themselves, so a kernel may differ from them only by
its fp32 accumulation and the rounding of the result to a pair: pair_tol.

The case lists at the end are shared by tests/test_pair_kernels_gpu.py (kernel against reference) and
tests/test_pair_reference_cpu.py (the reference is precise enough for pair_tol, and a missing or misplaced segment is
far larger than pair_tol)."""
import math

import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ numbers
def split(v32: torch.Tensor, dt):
    """fp32 -> (hi, lo) of dtype dt: hi = round(v), lo = round(v - hi), the residual formed in fp32 (split8, csrc/common.hpp)."""
    v32 = v32.float()
    hi = v32.to(dt)
    lo = (v32 - hi.float()).to(dt)
    return hi, lo


def pair_tol(dt, scale: float) -> float:
    """Bound on |y_hi + y_lo - fp64 reference| for an output of magnitude `scale`.
    fp16: 3e-6 * scale + 2e-6 -- what test_conv3x3_q8_matches_its_arithmetic asserts for this kernel family against its own
    arithmetic (fp32 accumulation of up to 9 * 1024 products; an fp16 pair carries 2^-22 per element).
    bf16: 2^-16 * scale + 2e-6 -- a bf16 pair carries 2^-18 per element with the residual formed in fp32; measured on the CPU
    model 5.1e-6 = 2^-17.6 of scale, so 2^-16 leaves a factor 3.  tests/test_pair_reference_cpu.py keeps both honest."""
    if dt == torch.float16:
        return 3e-6 * scale + 2e-6
    if dt == torch.bfloat16:
        return 2.0 ** -16 * scale + 2e-6
    raise TypeError(dt)


# ------------------------------------------------------------------------------------------------ packs and K indices
def expected_pack(w32: torch.Tensor, segs, transposed: bool, dt) -> torch.Tensor:
    """The [taps][Cout][sum len] pack pack_weight_segs must write for the fp32 weight w32 = [Cout][Cin][...] (transposed:
    [Cin][Cout][...]; the trailing dims are the taps in row-major order): per segment (kind, ci0, len) the channels
    [ci0, ci0 + len) of hi(w) (kind 0), lo(w) (kind 1) or zeros (kind 2)."""
    a, b = w32.shape[0], w32.shape[1]
    w = w32.float().reshape(a, b, -1)
    if transposed:
        w = w.transpose(0, 1)
    w = w.permute(2, 0, 1).contiguous()                      # [taps][Cout][Cin]
    hi, lo = split(w, dt)
    parts = []
    for kind, ci0, ln in segs:
        if kind == 2:
            parts.append(torch.zeros(w.shape[0], w.shape[1], ln, dtype=dt))
        else:
            src = hi if kind == 0 else lo
            assert 0 <= ci0 and ci0 + ln <= src.shape[2], (kind, ci0, ln)
            parts.append(src[..., ci0:ci0 + ln])
    return torch.cat(parts, dim=2).contiguous()


def k_channels(K: int, wrap: int, wrap_to: int = 0) -> torch.Tensor:
    """input channel (inside the kernel's window) each K index reads: k below wrap, then wrap_to + k - wrap."""
    assert wrap <= K <= 2 * wrap and wrap_to + (K - wrap) <= wrap, (K, wrap, wrap_to)
    k = torch.arange(K)
    return torch.where(k < wrap, k, wrap_to + k - wrap)


def seg_ranges(segs):
    """[(kind, k0, k1)]: the K range of every segment"""
    out, k0 = [], 0
    for kind, _, ln in segs:
        out.append((kind, k0, k0 + ln))
        k0 += ln
    return out


# ------------------------------------------------------------------------------------------------ the convolution
def _act(y, act):
    if act is None:
        return y
    if act == "relu":
        return torch.relu(y)
    raise ValueError(act)


def _conv_fp32_model(xk, pk, taps, out_hw, off, chunk=32):
    """The same sum the way an MFMA kernel forms it: the products of one tap and `chunk` consecutive K indices (one matrix
    instruction) summed exactly, these partial sums added one after the other to an fp32 accumulator."""
    cout, K = pk.shape[1], pk.shape[2]
    sp = xk.shape[1:-1]                                       # spatial dims
    nd = len(sp)
    if taps == 4:
        N, IH, IW = xk.shape[:3]
        y = torch.zeros(N, out_hw[0], out_hw[1], cout, dtype=torch.float32)
        for t in range(4):
            acc = torch.zeros(N, IH, IW, cout, dtype=torch.float32)
            for k0 in range(0, K, chunk):
                acc = acc + (xk[..., k0:k0 + chunk] @ pk[t, :, k0:k0 + chunk].t()).float()
            ky, kx = t // 2, t % 2
            y[:, off[0] + ky:off[0] + ky + 2 * IH:2, off[1] + kx:off[1] + kx + 2 * IW:2] = acc
        return y
    xp = F.pad(xk, (0, 0) + (1, 1) * nd)
    acc = torch.zeros(*xk.shape[:-1], cout, dtype=torch.float32)
    for t in range(taps):
        o = [(t // 3 ** (nd - 1 - i)) % 3 for i in range(nd)]
        idx = (slice(None),) + tuple(slice(o[i], o[i] + sp[i]) for i in range(nd))
        xs = xp[idx]
        for k0 in range(0, K, chunk):
            acc = acc + (xs[..., k0:k0 + chunk] @ pk[t, :, k0:k0 + chunk].t()).float()
    return acc


def pair_conv_ref(xwin, pack, taps, wrap_to=0, bias=None, act=None, ksel=None, dtype=torch.float64, out_hw=None, off=(0, 0)):
    """The convolution of the gathered 16-bit input channels with the 16-bit pack values, evaluated in `dtype` (fp64).
      taps = 9 : 3x3, pad 1.            xwin [N, H, W, wrap]     -> [N, H, W, Cout]
      taps = 27: 3x3x3, pad 1.          xwin [NB, D, H, W, wrap] -> [NB, D, H, W, Cout]
      taps = 4 : ConvTranspose 2x2 s2.  xwin [N, IH, IW, wrap]   -> [N, OH, OW, Cout] with out_hw = (OH, OW), off = (ooy, oox):
                 input pixel (y, x), tap (ky, kx) -> output pixel (2y + ky + ooy, 2x + kx + oox); pixels no input owns stay 0
                 (upconv_owned tells which).
    pack [taps][Cout][K]; K index k reads channel k_channels(K, wrap, wrap_to)[k] of xwin.  ksel: K indices to keep (the
    contribution of one segment); bias [Cout] and act ("relu") are applied after the sum.  dtype = torch.float32: the fp32
    accumulation model of _conv_fp32_model instead of fp64."""
    K, wrap = pack.shape[2], xwin.shape[-1]
    assert pack.shape[0] == taps
    kc = k_channels(K, wrap, wrap_to)
    pk = pack.double()
    if ksel is not None:
        kc, pk = kc[ksel], pk[..., ksel]
    xk = xwin.double()[..., kc]                               # [..., K']
    cout = pk.shape[1]
    if dtype == torch.float32:
        y = _conv_fp32_model(xk, pk, taps, out_hw, off)
    elif taps == 9:
        w = pk.reshape(3, 3, cout, -1).permute(2, 3, 0, 1)
        y = F.conv2d(xk.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    elif taps == 27:
        w = pk.reshape(3, 3, 3, cout, -1).permute(3, 4, 0, 1, 2)
        y = F.conv3d(xk.permute(0, 4, 1, 2, 3), w, padding=1).permute(0, 2, 3, 4, 1)
    elif taps == 4:
        N, IH, IW = xk.shape[:3]
        OH, OW = out_hw
        w = pk.reshape(2, 2, cout, -1).permute(3, 2, 0, 1)    # conv_transpose2d weight [Cin][Cout][ky][kx]
        up = F.conv_transpose2d(xk.permute(0, 3, 1, 2), w, stride=2).permute(0, 2, 3, 1)
        y = torch.zeros(N, OH, OW, cout, dtype=torch.float64)
        y[:, off[0]:off[0] + 2 * IH, off[1]:off[1] + 2 * IW] = up
    else:
        raise ValueError(taps)
    if bias is not None:
        b = bias.to(y.dtype)
        if taps == 4:
            y[:, off[0]:off[0] + 2 * xk.shape[1], off[1]:off[1] + 2 * xk.shape[2]] += b
        else:
            y = y + b
    return _act(y, act).contiguous()


def upconv_owned(IH, IW, OH, OW, ooy, oox) -> torch.Tensor:
    """[OH, OW] bool: the output pixels the transposed conv writes"""
    m = torch.zeros(OH, OW, dtype=torch.bool)
    m[ooy:ooy + 2 * IH, oox:oox + 2 * IW] = True
    return m


# ------------------------------------------------------------------------------------------------ inputs
def make_values(g, *shape):
    """activations like those behind a ReLU: half-normal * 1.5"""
    return torch.randn(*shape, generator=g).abs() * 1.5


def make_weight(g, cout, cin, *k, transposed=False, fan=None):
    """uniform in +-1/sqrt(fan) (fan = products per output element: cin * taps of a conv, cin of a k2/s2 transposed conv)"""
    taps = int(math.prod(k))
    fan = fan if fan is not None else (cin if transposed else cin * taps)
    shape = (cin, cout, *k) if transposed else (cout, cin, *k)
    return (torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(fan)


def make_window(v32, dt, lo0, lo_len, wrap, fill=0.0):
    """The window a pair kernel reads for a layer input v32 [..., cin]: [hi (cin) | lo of channels [lo0, lo0 + lo_len) | fill]
    cut / padded to `wrap` channels (a window of wrap = cin channels is the hi plane alone).  fill: a finite value for the
    channels only a zero segment multiplies."""
    hi, lo = split(v32, dt)
    cin = v32.shape[-1]
    win = torch.cat([hi, lo[..., lo0:lo0 + lo_len]], dim=-1)[..., :wrap]
    if win.shape[-1] < wrap:
        pad = torch.full((*win.shape[:-1], wrap - win.shape[-1]), fill, dtype=dt)
        win = torch.cat([win, pad], dim=-1)
    assert wrap >= cin
    return win.contiguous()


def pad_only_channels(segs, K, wrap, wrap_to=0):
    """window channels that only zero (kind 2) segments multiply"""
    kc = k_channels(K, wrap, wrap_to)
    zero, other = set(), set()
    for kind, k0, k1 in seg_ranges(segs):
        (zero if kind == 2 else other).update(kc[k0:k1].tolist())
    return sorted(zero - other)


DTYPES = [("f16", torch.float16), ("bf16", torch.bfloat16)]

# ------------------------------------------------------------------------------------------------ case lists
# conv3x3_segs: layouts from unet_engine._segs(mode, cin, lo_len).  form: conv3x3_set_kernel_form (-1 auto, 0 register-staged,
# 4 / 8 / 44 LDS-DMA forms).  The LDS-DMA kernel takes W >= 24 and Cout % 8 == 0; its work item is 32 x 16 pixels.
#   id                N  H   W   cin  lo_len cout mode  form in_coff out_coff bias   act
CONV2D_CASES = [
    ("dma_xw",        2, 37, 41, 64,  None,  64,  "xw",  -1,  8,     8,     False, None),
    ("dma_xw_half",   1, 17, 33, 128, 64,    72,  "xw",  -1,  16,    8,     False, None),    # decoder entry: lo_len = cin / 2
    ("dma_x_192",     2, 17, 33, 64,  None,  192, "x",   -1,  8,     16,    False, None),
    ("dma_w",         1, 37, 41, 64,  None,  64,  "w",   -1,  8,     8,     False, None),
    ("dma_1",         2, 24, 40, 128, None,  72,  "1",   -1,  8,     8,     False, None),
    ("narrow_xw",     2, 13, 20, 64,  None,  64,  "xw",  -1,  8,     16,    False, None),    # W < 24: the register-staged kernel
    ("narrow_xwm",    3, 9,  17, 128, 64,    72,  "xw-", -1,  16,    8,     False, None),
    ("form0_xw",      1, 37, 41, 64,  None,  64,  "xw",  0,   8,     8,     False, None),    # ... and pinned at a DMA shape
    ("form0_x_half",  2, 17, 33, 128, 64,    192, "x",   0,   8,     8,     False, None),
    ("form4_xwm",     2, 37, 41, 128, 64,    64,  "xw-", 4,   8,     8,     False, None),
    ("form8_xw",      1, 17, 33, 64,  None,  72,  "xw",  8,   16,    8,     False, None),
    ("form44_w",      2, 24, 40, 64,  None,  64,  "w",   44,  8,     8,     False, None),
    ("dma_xw_bias",   1, 17, 33, 64,  None,  64,  "xw",  -1,  8,     8,     True,  None),
    ("dma_xw_relu",   2, 17, 33, 64,  None,  72,  "xw",  -1,  8,     8,     True,  "relu"),
]

# conv3d3_segs: layouts from unet3d_engine.segs3d(mode, cin, lo0, lo_len); the output is dense.  The two "tail" layouts put a
# zero segment over channels BEHIND the valid lo channels: segs3d refuses them (the engine never writes those channels), the
# kernel must still multiply whatever finite values sit there by zero.
CONV3D_LAYOUTS = {
    "tail_x":      ([(0, 0, 136), (0, 96, 40), (2, 0, 16)], 192, 192),
    "tail_xw_mid": ([(0, 0, 128), (0, 88, 40), (2, 0, 24), (1, 0, 128)], 320, 192),
}
#   id               NB D  H   W   cin  lo0  lo_len cout mode
CONV3D_CASES = [
    ("c32_xw",       2, 3, 9,  13, 32,  0,   None,  64,  "xw"),      # the 32-channel conv: K padded to 128 by a zero segment
    ("c32_xw_dma",   1, 2, 8,  24, 32,  0,   None,  64,  "xw"),
    ("c40_1",        1, 3, 8,  24, 40,  0,   None,  64,  "1"),       # hi plane + a zero segment over the first lo channels
    ("res_xwm",      1, 4, 8,  24, 192, 128, 64,    64,  "xw-"),     # wrap_to = lo0
    ("res_xwm_nb",   2, 2, 9,  13, 192, 128, 64,    72,  "xw-"),
    ("d1_x",         2, 1, 9,  25, 64,  0,   None,  72,  "x"),
    ("d2_w",         1, 2, 16, 24, 64,  0,   None,  64,  "w"),
    ("tail_x",       1, 2, 8,  24, 136, 96,  40,    64,  "x"),       # zero segment over channels past the valid lo channels
    ("tail_xw_mid",  2, 3, 7,  11, 128, 88,  40,    64,  "xw"),      # four segments, the zero segment in the middle
    ("c160_xw_res",  1, 2, 8,  12, 160, 128, 32,    64,  "xw"),      # four segments, the zero segment behind w_lo
]

# upconv2x2_fwd_segs / upconv2x2_fwd_precise: (OH, OW) = (2 IH + 1, 2 IW + 1); layouts from unet_engine._segs(mode, cin);
# mode "split" = pack_weight_split + upconv2x2_fwd_precise.  Shapes of test_upconv2x2_dma_gemm_path plus a ragged one.
#   id             N  IH  IW  cin  cout mode     (ooy, oox)
UPCONV_CASES = [
    ("u128_xw",    2, 8,  16, 128, 64,  "xw",    (0, 0)),
    ("u256_x",     4, 16, 8,  256, 192, "x",     (0, 1)),
    ("u128_split", 8, 32, 32, 128, 64,  "split", (1, 0)),
    ("u384_w",     1, 16, 16, 384, 128, "w",     (0, 1)),
    ("u64_ragged", 3, 5,  7,  64,  72,  "xw",    (1, 0)),
    ("u128_1",     2, 5,  6,  128, 64,  "1",     (0, 0)),
]


def build_conv2d(case, dt):
    """inputs of a CONV2D_CASES entry, all on the CPU: dict(win, w32, segs, K, wrap, bias)"""
    from semantic_segmentation_amd.unet.unet_engine import _segs
    name, N, H, W, cin, lo_len, cout, mode, form, in_coff, out_coff, has_bias, act = case
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    segs, K, wrap = _segs(mode, cin, lo_len)
    v = make_values(g, N, H, W, cin)
    w32 = make_weight(g, cout, cin, 3, 3)
    bias = (torch.rand(cout, generator=g) - 0.5) * 0.2 if has_bias else None
    ll = cin if lo_len is None else lo_len
    return dict(win=make_window(v, dt, 0, ll, wrap), w32=w32, segs=segs, K=K, wrap=wrap, wrap_to=0, bias=bias, act=act, taps=9)


def build_conv3d(case, dt, fill=0.25):
    from semantic_segmentation_amd.unet3d.unet3d_engine import segs3d
    name, NB, D, H, W, cin, lo0, lo_len, cout, mode = case
    g = torch.Generator().manual_seed(2000 + sum(map(ord, name)))
    segs, K, wrap = CONV3D_LAYOUTS[name] if name in CONV3D_LAYOUTS else segs3d(mode, cin, lo0, lo_len)
    v = make_values(g, NB, D, H, W, cin)
    w32 = make_weight(g, cout, cin, 3, 3, 3)
    ll = cin if lo_len is None else lo_len
    return dict(win=make_window(v, dt, lo0, ll, wrap, fill), w32=w32, segs=segs, K=K, wrap=wrap,
                wrap_to=lo0 if mode == "xw-" else 0, bias=None, act=None, taps=27)


def build_upconv(case, dt):
    from semantic_segmentation_amd.unet.unet_engine import _segs
    name, N, IH, IW, cin, cout, mode, off = case
    g = torch.Generator().manual_seed(3000 + sum(map(ord, name)))
    segs, K, wrap = ([(0, 0, cin), (0, 0, cin), (1, 0, cin)], 3 * cin, 2 * cin) if mode == "split" else _segs(mode, cin)
    v = make_values(g, N, IH, IW, cin)
    w32 = make_weight(g, cout, cin, 2, 2, transposed=True)
    bias = (torch.rand(cout, generator=g) - 0.5) * 0.2
    return dict(win=make_window(v, dt, 0, cin, wrap), w32=w32, segs=segs, K=K, wrap=wrap, wrap_to=0, bias=bias, act=None, taps=4,
                out_hw=(2 * IH + 1, 2 * IW + 1), off=off, transposed=True)


def case_ref(c, dt, **kw):
    """the fp64 reference of a built case (kw: overrides such as ksel / dtype / a changed window or pack)"""
    pack = kw.pop("pack", None)
    if pack is None:
        pack = expected_pack(c["w32"], c["segs"], c.get("transposed", False), dt)
    args = dict(wrap_to=c["wrap_to"], bias=c["bias"], act=c["act"])
    if c["taps"] == 4:
        args.update(out_hw=c["out_hw"], off=c["off"])
    args.update(kw)
    win = args.pop("win", c["win"])
    return pair_conv_ref(win, pack, c["taps"], **args)
