"""The kernels of the hi/lo pair forward, each against the fp64 reference of tests/pair_reference.py.

Every comparison is max |(y_hi + y_lo) - ref64| < pair_tol(dt, max |ref64|): a few 1e-6 of the output scale, 20 to 100 times
below the effect of one missing or misplaced correction segment (tests/test_pair_reference_cpu.py proves both on the CPU, for
the case lists used here).  Inputs come from a seeded CPU generator; input channels outside the window a kernel may read hold
NaN, output channels / pixels it must not write hold a sentinel that has to survive bit for bit.  GPU only (`-m gpu`)."""
import pytest
import torch

from tests import pair_reference as pr

pytestmark = pytest.mark.gpu

SENT = 7.0                                                   # finite sentinel in output buffers
ACT = {None: 0, "relu": 1}                                   # _lib.ACT_NONE / ACT_RELU


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


def ids(cases):
    return [c[0] for c in cases]


def in_buffer(win, in_coff, extra=8):
    """the window inside a wider buffer whose other channels are NaN"""
    buf = torch.full((*win.shape[:-1], in_coff + win.shape[-1] + extra), float("nan"), dtype=win.dtype)
    buf[..., in_coff:in_coff + win.shape[-1]] = win
    return buf.to(dev())


def device_pack(w32, segs, transposed, dt):
    from semantic_segmentation_amd import ops
    cout = w32.shape[1] if transposed else w32.shape[0]
    taps = w32[0, 0].numel()
    pack = torch.full((taps, cout, sum(s[2] for s in segs)), SENT, dtype=dt, device=dev())
    ops.pack_weight_segs([(w32.to(dev()).contiguous(), pack, transposed, segs)])
    return pack


def check_pair(y_hi, y_lo, ref, dt, what=""):
    got = y_hi.double().cpu() + y_lo.double().cpu()
    assert torch.isfinite(got).all(), what
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"{what}: max err {err:.3e} tol {pr.pair_tol(dt, scale):.3e} scale {scale:.3f}")
    assert err < pr.pair_tol(dt, scale), (what, err, pr.pair_tol(dt, scale))
    return got


def check_stat_rows(part, nt, cout, got):
    """BatchNorm partial rows [nt][2][Cout]: slot 0 sums to the column sums of y = y_hi + y_lo, slot 1 to those of y^2"""
    p = part[:nt * 2 * cout].view(nt, 2, cout).double().sum(0).cpu()
    y = got.reshape(-1, cout)
    s1, s2 = y.sum(0), (y * y).sum(0)
    assert float((p[0] - s1).abs().max()) < 1e-5 * float(y.abs().sum(0).max()), float((p[0] - s1).abs().max())
    assert float((p[1] - s2).abs().max()) < 1e-3 * float(s2.max()), float((p[1] - s2).abs().max())


# ------------------------------------------------------------------------------------------------ packs
def _pack_layouts():
    """every layout unet_engine._segs / unet3d_engine.segs3d can return: modes 1, x, w, xw, xw-; lo_len < cin; lo0 > 0; zero
    segments; four segments"""
    from semantic_segmentation_amd.unet.unet_engine import _segs
    from semantic_segmentation_amd.unet3d.unet3d_engine import segs3d
    lay = []
    for mode in ("1", "x", "w", "xw", "xw-"):
        lay.append((64, _segs(mode, 64)[0]))
        lay.append((128, _segs(mode, 128, 64)[0]))
    for mode, cin, lo0, ll in (("1", 40, 0, None), ("w", 32, 0, None), ("xw", 32, 0, None), ("xw", 160, 128, 32),
                               ("xw-", 192, 128, 64), ("xw-", 320, 256, 64), ("w", 104, 64, 40)):
        lay.append((cin, segs3d(mode, cin, lo0, ll)[0]))
    lay += [(136, pr.CONV3D_LAYOUTS["tail_x"][0]), (128, pr.CONV3D_LAYOUTS["tail_xw_mid"][0])]
    assert any(len(s) == 4 for _, s in lay) and any(k == 2 for _, s in lay for k, _, _ in s)
    return lay


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
def test_pack_weight_segs_bit_equal_to_definition(dtn, dt):
    """gs_pack_weight_segs, many descriptors in ONE launch (test_pack_weight_multi_matches_single is the model): 9, 27 and 4 taps,
    transposed or not, every segment layout of the engines -- bit-equal to pair_reference.expected_pack; and gs_pack_weight_split
    == the [hi | hi | lo] segment pack"""
    from semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(77)
    items, want = [], []
    for j, (cin, segs) in enumerate(_pack_layouts()):
        for shape, tr in (((72, cin, 3, 3), False), ((40, cin, 27, 1), False), ((cin, 24, 2, 2), True)):
            w = torch.randn(*shape, generator=g) * (0.05 if j % 2 else 3.0)
            cout = shape[1] if tr else shape[0]
            pack = torch.full((shape[2] * shape[3], cout, sum(s[2] for s in segs)), SENT, dtype=dt, device=dev())
            items.append((w.to(dev()), pack, tr, segs))
            want.append(pr.expected_pack(w, segs, tr, dt))
    ops.pack_weight_segs(items)
    torch.cuda.synchronize()
    for (w, pack, tr, segs), exp in zip(items, want):
        assert pack.shape == exp.shape
        assert torch.equal(bits(pack.cpu()), bits(exp)), (tuple(w.shape), tr, segs)
    for shape, tr in (((72, 64, 3, 3), False), ((128, 40, 2, 2), True), ((8, 128, 27, 1), False)):
        w = torch.randn(*shape, generator=g)
        cin, cout = (shape[0], shape[1]) if tr else (shape[1], shape[0])
        pack = torch.full((shape[2] * shape[3], cout, 3 * cin), SENT, dtype=dt, device=dev())
        ops.pack_weight_split(w.to(dev()), pack, tr)
        exp = pr.expected_pack(w, [(0, 0, cin), (0, 0, cin), (1, 0, cin)], tr, dt)
        assert torch.equal(bits(pack.cpu()), bits(exp)), (shape, tr)


# ------------------------------------------------------------------------------------------------ conv3x3_segs / conv3x3_precise
def run_conv2d(case, dt, c=None, precise=False):
    from semantic_segmentation_amd import ops
    name, N, H, W, cin, lo_len, cout, mode, form, in_coff, out_coff, has_bias, act = case
    c = c or pr.build_conv2d(case, dt)
    K, wrap = c["K"], c["wrap"]
    xbuf = in_buffer(c["win"], in_coff)
    ostr = out_coff + cout + 8
    y_hi = torch.full((N, H, W, ostr), SENT, dtype=dt, device=dev())
    y_lo = torch.full((N, H, W, ostr), SENT, dtype=dt, device=dev())
    bias = c["bias"].to(dev()) if c["bias"] is not None else None
    if precise:
        pack = torch.empty(9, cout, 3 * cin, dtype=dt, device=dev())
        ops.pack_weight_split(c["w32"].to(dev()), pack, False)
    else:
        pack = device_pack(c["w32"], c["segs"], False, dt)
    ops.conv3x3_set_kernel_form(form)
    try:
        nt = ops.conv3x3_stat_rows(N, H, W, K, cout, pair=True)       # after the form is pinned: the row count depends on it
        rows = max(nt, ops.conv3x3_mtiles(N, H, W, cout))             # "a buffer of conv3x3_mtiles() rows always suffices"
        part = torch.zeros(ops.bn_partials_numel(rows, cout), dtype=torch.float32, device=dev()) if not has_bias else None
        if precise:
            ops.conv3x3_precise(xbuf, pack, y_hi, y_lo, N, H, W, cin, cout, xbuf.shape[-1], in_coff, ostr, out_coff, bias, part, ACT[act])
        else:
            ops.conv3x3_segs(xbuf, pack, y_hi, y_lo, N, H, W, K, wrap, cin, cout, xbuf.shape[-1], in_coff, ostr, out_coff, bias,
                             part, ACT[act])
        torch.cuda.synchronize()
    finally:
        ops.conv3x3_set_kernel_form(-1)
    return c, y_hi, y_lo, part, nt


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("case", pr.CONV2D_CASES, ids=ids(pr.CONV2D_CASES))
def test_conv3x3_segs_vs_fp64(case, dtn, dt):
    """conv3x3_segs on every segment layout of unet_engine._segs: the LDS-DMA kernel with ragged 32 x 16 items, the register-staged
    kernel (W < 24, and pinned by form 0), forms 4 / 8 / 44, Cout 64 / 72 / 192, N > 1, channel offsets and strides wider than
    the window, bias and ReLU -- against the fp64 dot product of the same 16-bit values; BatchNorm partial rows"""
    name, N, H, W, cin, lo_len, cout, mode, form, in_coff, out_coff, has_bias, act = case
    c, y_hi, y_lo, part, nt = run_conv2d(case, dt)
    ref = pr.case_ref(c, dt)
    sl = slice(out_coff, out_coff + cout)
    got = check_pair(y_hi[..., sl], y_lo[..., sl], ref, dt, f"conv3x3_segs {name} {dtn}")
    for y in (y_hi, y_lo):                                           # the channels around the slice: bit-unchanged
        assert bool((y[..., :out_coff] == SENT).all()) and bool((y[..., out_coff + cout:] == SENT).all())
    if part is not None:
        check_stat_rows(part, nt, cout, got)


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("case", [c for c in pr.CONV2D_CASES if c[0] in ("dma_xw", "narrow_xw", "form0_xw", "form8_xw", "dma_xw_relu")],
                         ids=lambda c: c[0])
def test_conv3x3_precise_is_the_hi_hi_lo_segment_conv(case, dtn, dt):
    """conv3x3_precise on a pack_weight_split pack is BIT-IDENTICAL to conv3x3_segs on the [hi | hi | lo] segment pack ("xw")"""
    assert case[7] == "xw" and case[5] is None
    c, a_hi, a_lo, pa, nt = run_conv2d(case, dt)
    _, b_hi, b_lo, pb, _ = run_conv2d(case, dt, c=c, precise=True)
    assert torch.equal(bits(a_hi), bits(b_hi)) and torch.equal(bits(a_lo), bits(b_lo))
    if pa is not None:
        assert torch.equal(pa, pb)


# ------------------------------------------------------------------------------------------------ conv3d3_segs
def run_conv3d(case, dt, fill, in_coff=8):
    from semantic_segmentation_amd import ops
    name, NB, D, H, W, cin, lo0, lo_len, cout, mode = case
    c = pr.build_conv3d(case, dt, fill)
    K, wrap = c["K"], c["wrap"]
    xbuf = in_buffer(c["win"].reshape(NB * D, H, W, wrap), in_coff)
    y_hi = torch.full((NB * D, H, W, cout), SENT, dtype=dt, device=dev())
    y_lo = torch.full((NB * D, H, W, cout), SENT, dtype=dt, device=dev())
    pack = device_pack(c["w32"].reshape(cout, cin, 27, 1), c["segs"], False, dt)
    nt = ops.conv3x3_stat_rows(NB * D, H, W, K, cout, pair=True)
    rows = max(nt, ops.conv3x3_mtiles(NB * D, H, W, cout))
    part = torch.zeros(ops.bn_partials_numel(rows, cout), dtype=torch.float32, device=dev())
    ops.conv3d3_segs(xbuf, pack, y_hi, y_lo, NB, D, H, W, K, wrap, cin, cout, xbuf.shape[-1], in_coff, part, wrap_to=c["wrap_to"])
    torch.cuda.synchronize()
    return c, y_hi, y_lo, part, nt


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("case", pr.CONV3D_CASES, ids=ids(pr.CONV3D_CASES))
def test_conv3d3_segs_vs_fp64(case, dtn, dt):
    """conv3d3_segs on the layouts of unet3d_engine.segs3d: D = 1 .. 4, NB > 1, the 32-channel conv (K padded to 128 by zero
    segments), "xw-" with wrap_to = lo0, zero segments over channels past the valid lo channels -- against the fp64 reference.
    A zero segment must not let the channels under it through: two launches with different finite values there give
    bit-identical pairs"""
    name, NB, D, H, W, cin, lo0, lo_len, cout, mode = case
    c, y_hi, y_lo, part, nt = run_conv3d(case, dt, 0.25)
    ref = pr.case_ref(c, dt).reshape(NB * D, H, W, cout)
    got = check_pair(y_hi, y_lo, ref, dt, f"conv3d3_segs {name} {dtn}")
    check_stat_rows(part, nt, cout, got)
    if pr.pad_only_channels(c["segs"], c["K"], c["wrap"], c["wrap_to"]):
        _, z_hi, z_lo, _, _ = run_conv3d(case, dt, -1000.0)
        assert torch.equal(bits(y_hi), bits(z_hi)) and torch.equal(bits(y_lo), bits(z_lo))


# ------------------------------------------------------------------------------------------------ transposed conv
@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("case", pr.UPCONV_CASES, ids=ids(pr.UPCONV_CASES))
def test_upconv2x2_pair_vs_fp64(case, dtn, dt):
    """upconv2x2_fwd_segs / upconv2x2_fwd_precise (ConvTranspose2d k2 s2 + bias on pairs) written into both planes of a wider
    concat buffer at a channel offset, the 2 IH x 2 IW patch placed at (ooy, oox) inside a (2 IH + 1) x (2 IW + 1) output.  The
    pair kernel runs on the implicit-GEMM engine, which scatters to the pixels it owns: border pixels and the other channels are
    left alone (test_conv_transpose2x2_fwd_bwd / test_upconv2x2_dma_gemm_path pre-zero the buffer and find zeros there)."""
    from semantic_segmentation_amd import ops
    name, N, IH, IW, cin, cout, mode, (ooy, oox) = case
    c = pr.build_upconv(case, dt)
    OH, OW = c["out_hw"]
    in_coff, out_coff = 8, 16
    xbuf = in_buffer(c["win"], in_coff)
    ctot = out_coff + cout + 8                                       # one plane of the concat buffer
    g = torch.Generator().manual_seed(9)
    cat0 = (torch.randn(N, OH, OW, 2 * ctot, generator=g) + SENT).to(dt)
    cat = cat0.to(dev())
    bias = c["bias"].to(dev())
    if mode == "split":
        pack = torch.empty(4, cout, 3 * cin, dtype=dt, device=dev())
        ops.pack_weight_split(c["w32"].to(dev()), pack, True)
        ops.upconv2x2_fwd_precise(xbuf, pack, bias, cat, cat[..., ctot:], N, IH, IW, cin, cout, OH, OW, xbuf.shape[-1], in_coff,
                                  2 * ctot, out_coff, ooy, oox)
    else:
        pack = device_pack(c["w32"], c["segs"], True, dt)
        ops.upconv2x2_fwd_segs(xbuf, pack, bias, cat, cat[..., ctot:], N, IH, IW, c["K"], c["wrap"], cin, cout, OH, OW,
                               xbuf.shape[-1], in_coff, 2 * ctot, out_coff, ooy, oox)
    torch.cuda.synchronize()
    out = cat.cpu()
    own = pr.upconv_owned(IH, IW, OH, OW, ooy, oox)
    ref = pr.case_ref(c, dt)
    y_hi, y_lo = out[..., out_coff:out_coff + cout], out[..., ctot + out_coff:ctot + out_coff + cout]
    check_pair(y_hi[:, own], y_lo[:, own], ref[:, own], dt, f"upconv2x2 {name} {dtn}")
    keep = torch.ones(N, OH, OW, 2 * ctot, dtype=torch.bool)
    keep[:, own, out_coff:out_coff + cout] = False
    keep[:, own, ctot + out_coff:ctot + out_coff + cout] = False
    assert torch.equal(bits(out)[keep], bits(cat0)[keep]), "pixels / channels the kernel does not own must stay bit-unchanged"


# ------------------------------------------------------------------------------------------------ elementwise and edge kernels
def _bn_ref(v64, sc, sh, act):
    t = v64 * sc.double() + sh.double()
    return torch.relu(t) if act == "relu" else t


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("N,H,W,C,z_coff,pool,with_lo,act", [(2, 9, 7, 72, 8, True, True, "relu"), (1, 8, 10, 64, 0, True, False, "relu"),
                                                              (3, 5, 11, 40, 16, False, True, None), (2, 7, 7, 64, 8, False, False, "relu"),
                                                              (2, 11, 6, 128, 0, True, True, None)])
def test_bn_act_apply_split_vs_fp64(dtn, dt, N, H, W, C, z_coff, pool, with_lo, act):
    """z pair = act(scale * (y_hi + y_lo) + shift) against fp64 to the pair rounding (z_lo = None: to the 16-bit rounding of the
    hi plane), odd H / W, a channel offset inside a wider buffer; the pooled pair = the maximum of the STORED pair values, split
    again, bit for bit (odd sizes drop the last row / column); zp_lo = None when z_lo is None"""
    from semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(H * W + C)
    v = torch.randn(N, H, W, C, generator=g) * 2
    y_hi, y_lo = pr.split(v, dt)
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    zs = z_coff + C + 8
    z_hi = torch.full((N, H, W, zs), SENT, dtype=dt, device=dev())
    z_lo = torch.full((N, H, W, zs), SENT, dtype=dt, device=dev())
    zp = torch.full((N, H // 2, W // 2, 2 * C + 8), SENT, dtype=dt, device=dev())
    ops.bn_act_apply_split(y_hi.to(dev()), y_lo.to(dev()), sc.to(dev()), sh.to(dev()), ACT[act], z_hi, z_lo if with_lo else None, zs, z_coff,
                           zp if pool else None, zp[..., C:] if (pool and with_lo) else None, 2 * C + 8)
    torch.cuda.synchronize()
    ref = _bn_ref(y_hi.double() + y_lo.double(), sc, sh, act)
    sl = slice(z_coff, z_coff + C)
    zh, zl = z_hi[..., sl].cpu(), z_lo[..., sl].cpu()
    if with_lo:
        check_pair(zh, zl, ref, dt, "bn_act_apply_split")
        stored = zh.float() + zl.float()
    else:
        half_ulp = 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8
        assert bool(((zh.double() - ref).abs() <= half_ulp * 1.001 * ref.abs() + 1e-7).all())
        assert bool((z_lo == SENT).all())
        stored = zh.float()
    for z in (z_hi, z_lo):
        assert bool((z[..., :z_coff] == SENT).all()) and bool((z[..., z_coff + C:] == SENT).all())
    if pool:
        m = stored[:, :H // 2 * 2, :W // 2 * 2].reshape(N, H // 2, 2, W // 2, 2, C).amax(dim=(2, 4))
        mh, ml = pr.split(m, dt)
        assert torch.equal(bits(zp[..., :C].cpu()), bits(mh))
        if with_lo:
            assert torch.equal(bits(zp[..., C:2 * C].cpu()), bits(ml))
            assert bool((zp[..., 2 * C:] == SENT).all())
        else:
            assert bool((zp[..., C:] == SENT).all())
    else:
        assert bool((zp == SENT).all())


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("N,H,W,ncls", [(2, 18, 22, 2), (3, 45, 53, 1), (1, 33, 64, 4)])
def test_head1x1_split_vs_fp64(dtn, dt, N, H, W, ncls):
    """head1x1_fwd_split (OutConv on a pair) and head1x1_bn_fwd_split (BatchNorm + ReLU on the load path): fp32 logits against fp64
    to 1e-6 * scale + 1e-6 (64 terms of fp32 accumulation).  (test_head1x1_on_conv_output_with_bn_relu pins the 16-bit form.)"""
    from semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(ncls + H)
    v = torch.randn(N, H, W, 64, generator=g)
    x_hi, x_lo = pr.split(v, dt)
    w = (torch.rand(ncls, 64, generator=g) * 2 - 1) / 8
    b = torch.randn(ncls, generator=g) * 0.1
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3
    val = x_hi.double() + x_lo.double()
    for bn in (False, True):
        logits = torch.full((N, ncls, H, W), float("nan"), dtype=torch.float32, device=dev())
        if bn:
            ops.head1x1_bn_fwd_split(x_hi.to(dev()), x_lo.to(dev()), sc.to(dev()), sh.to(dev()), ACT["relu"], w.to(dev()), b.to(dev()), logits)
            src = _bn_ref(val, sc, sh, "relu")
        else:
            ops.head1x1_fwd_split(x_hi.to(dev()), x_lo.to(dev()), w.to(dev()), b.to(dev()), logits)
            src = val
        torch.cuda.synchronize()
        ref = (src @ w.double().t() + b.double()).permute(0, 3, 1, 2)
        scale = float(ref.abs().max())
        err = float((logits.double().cpu() - ref).abs().max())
        print(f"head1x1 bn={bn} ncls={ncls}: err {err:.3e} scale {scale:.3f}")
        assert err < 1e-6 * scale + 1e-6, (bn, err, scale)


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("Cin,Cout", [(1, 64), (3, 64), (3, 32)])
def test_first_conv_pair_vs_fp64(dtn, dt, Cin, Cout):
    """conv_smallcin_fwd_split (fp32 image and weights -> conv-output pair + BatchNorm partial rows) for 1 and 3 channels on a ragged
    image, and stem_fwd_bn_pair (1 channel: conv + BatchNorm + ReLU in one pass into a [hi | lo] buffer), against fp64 to pair_tol.
    (test_smallcin_split_cout32_thread_per_pixel_form and test_stem_without_conv_output_in_memory pin both at 2e-5 / 2e-4 .. 3e-4
    relative to fp32 / their own coefficients.)"""
    import torch.nn.functional as F
    from semantic_segmentation_amd import ops
    N, H, W = 2, 45, 53
    g = torch.Generator().manual_seed(Cin * 100 + Cout)
    x = torch.rand(N, Cin, H, W, generator=g)
    w = (torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) / (9 * Cin) ** 0.5
    y_hi = torch.full((N, H, W, Cout), SENT, dtype=dt, device=dev())
    y_lo = torch.full((N, H, W, Cout), SENT, dtype=dt, device=dev())
    nt = ops.conv_smallcin_mtiles(N, H, W)
    part = torch.zeros(ops.bn_partials_numel(nt, Cout), dtype=torch.float32, device=dev())
    ops.conv_smallcin_fwd_split(x.to(dev()), w.to(dev()), y_hi, y_lo, part, 3, 1)
    torch.cuda.synchronize()
    ref = F.conv2d(x.double(), w.double(), padding=1).permute(0, 2, 3, 1)
    got = check_pair(y_hi, y_lo, ref, dt, f"conv_smallcin_fwd_split {Cin}->{Cout}")
    check_stat_rows(part, nt, Cout, got)
    if Cin == 1 and Cout == 64:
        sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3
        zpair = torch.full((N, H, W, 128), float("nan"), dtype=dt, device=dev())
        ops.stem_fwd_bn_pair(x.to(dev()), w.to(dev()), sc.to(dev()), sh.to(dev()), ACT["relu"], zpair)
        torch.cuda.synchronize()
        check_pair(zpair[..., :64], zpair[..., 64:], _bn_ref(ref, sc, sh, "relu"), dt, "stem_fwd_bn_pair")


def test_bn_act_apply_split_pool3d_rejects_misaligned_planes():
    """the fused BatchNorm + ReLU + MaxPool3d pass stores 16-byte channel groups: a plane that does not start on a 16-byte boundary
    is an argument error, not a launch"""
    from semantic_segmentation_amd import ops
    NB, D, H, W, C = 1, 2, 4, 4, 64
    dt = torch.float16
    y = torch.zeros(2, NB * D, H, W, C, dtype=dt, device=dev())
    sc, sh = torch.ones(C, device=dev()), torch.zeros(C, device=dev())
    z = torch.zeros(NB * D, H, W, 2 * C + 16, dtype=dt, device=dev())
    zp = torch.zeros(NB * D // 2, H // 2, W // 2, 2 * C + 16, dtype=dt, device=dev())
    ops.bn_act_apply_split_pool3d(y[0], y[1], sc, sh, 1, z, z[..., C:], 2 * C + 16, 0, zp, zp[..., C:], 2 * C + 16, NB, D, H, W)
    for bad in ("z_hi", "z_lo", "zp_hi", "zp_lo"):
        a = dict(z_hi=z, z_lo=z[..., C:], zp_hi=zp, zp_lo=zp[..., C:])
        a[bad] = a[bad][..., 4:]                                     # 8 bytes off
        with pytest.raises(RuntimeError, match="16-byte"):
            ops.bn_act_apply_split_pool3d(y[0], y[1], sc, sh, 1, a["z_hi"], a["z_lo"], 2 * C + 16, 0, a["zp_hi"], a["zp_lo"], 2 * C + 16,
                                          NB, D, H, W)
    torch.cuda.synchronize()
