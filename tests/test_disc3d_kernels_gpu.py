"""The kernels of the 3-D Pix2Pix discriminators at ZERO tolerance on integer operands (tests/disc3d_reference.py), f16 and bf16: the
image-side conv of csrc/ends_img.hip, the one-channel head of csrc/ends3d.hip, and the k4 middle convs on the generic engine through
the 3-D geometry builders (64 depth-strided taps in one launch).  Equal after one correct rounding of a 16-bit store; two runs
bit-equal; the refusals return before any launch (GPU only)."""
import pytest
import torch

from tests import disc3d_reference as d3
from tests import exact_reference as er

pytestmark = pytest.mark.gpu

SENT = 7.0
ACT_NONE, ACT_RELU, ACT_LEAKY02 = 0, 1, 2
GS_EINVAL, GS_EUNSUPPORTED = -1, -3


def dev():
    return torch.device("cuda:0")


def sl(t, dt=None):
    """[N,C,D,H,W] -> the device's [N*D,H,W,C]"""
    t = d3.slices(t)
    return (t if dt is None else t.to(dt)).to(dev())


def full(shape, dtype):
    return torch.full(tuple(shape), SENT, dtype=dtype, device=dev())


@pytest.mark.parametrize("dtn,dt", er.DTS)
@pytest.mark.parametrize("case", d3.IMG_CASES, ids=d3.img_id)
def test_image_side_forward_exact(case, dtn, dt):
    """plain conv, and conv + bias + LeakyReLU(0.2): every output element is the one correctly rounded value"""
    from semantic_segmentation_amd import ops
    Cin, Cout, k, N, vol = case
    s, p = d3.GEOM[k]
    OD, OH, OW = d3.img_out(case)
    for vset in ("S", "P"):
        c = d3.img_build(case, vset)
        what = f"img3d fwd {d3.img_id(case)} {vset} {dtn}"
        x, w, b = c["x"].to(dev()), c["w"].to(dev()), c["b"].to(dev())
        y = full((N * OD, OH, OW, Cout), dt)
        ops.conv3d_img_fwd(x, w, None, y, k, s, p, ACT_NONE)
        er.assert_exact(y.cpu(), er.expect16(d3.slices(c["y"]), dt), what)
        y2 = full((N * OD, OH, OW, Cout), dt)
        ops.conv3d_img_fwd(x, w, b, y2, k, s, p, ACT_LEAKY02)
        ref = d3.slices(c["y"] + c["b"].double().view(1, -1, 1, 1, 1))
        er.assert_leaky_exact(y2.cpu(), ref, what + " + bias + leaky")
        y3 = full((N * OD, OH, OW, Cout), dt)
        ops.conv3d_img_fwd(x, w, b, y3, k, s, p, ACT_LEAKY02)
        assert torch.equal(y2.view(torch.int16), y3.view(torch.int16)), "two forward runs differ"


@pytest.mark.parametrize("dtn,dt", er.DTS)
@pytest.mark.parametrize("case", d3.IMG_CASES, ids=d3.img_id)
def test_image_side_gradients_exact(case, dtn, dt):
    """weight gradient (one block; several slabs; blocks that walk several patches: the 40 x 18 x 70 case) and data gradient (one and
    two 64-channel chunks, every register form) with gscale = 1/4; the layer's bias gradient (gs_colsum over dy, as the engine runs
    it); two runs bit-equal"""
    from semantic_segmentation_amd import ops
    Cin, Cout, k, N, vol = case
    s, p = d3.GEOM[k]
    OD, OH, OW = d3.img_out(case)
    c = d3.img_build(case, "S")
    x, w = c["x"].to(dev()), c["w"].to(dev())
    dy = sl(c["dy"], dt)
    what = f"{d3.img_id(case)} {dtn}"
    runs = []
    for _ in range(2):
        g = full((Cout, Cin, k, k, k), torch.float32)
        ops.conv3d_img_wgrad(x, dy, g, k, s, p, d3.GSCALE)
        runs.append(g)
    er.assert_exact(runs[0].cpu(), er.expect32(c["dw"], d3.GSCALE), "img3d wgrad " + what)
    assert torch.equal(runs[0], runs[1]), "two weight-gradient runs differ"
    runs = []
    for _ in range(2):
        dx = full((N, Cin) + tuple(vol), torch.float32)
        ops.conv3d_img_dgrad(dy, w, dx, k, s, p, d3.GSCALE)
        runs.append(dx)
    er.assert_exact(runs[0].cpu(), er.expect32(c["dx"], d3.GSCALE), "img3d dgrad " + what)
    assert torch.equal(runs[0], runs[1]), "two data-gradient runs differ"
    ws = torch.empty(1024 * Cout, dtype=torch.float32, device=dev())
    db = full((Cout,), torch.float32)
    ops.colsum(dy, Cout, 0, N * OD, OH, OW, 0, 0, OH, OW, Cout, d3.GSCALE, ws, db)
    er.assert_exact(db.cpu(), er.expect32(d3.db_right(c["dy"].double()), d3.GSCALE), "bias gradient " + what)


@pytest.mark.parametrize("dtn,dt", er.DTS)
@pytest.mark.parametrize("case", d3.HEAD_CASES, ids=d3.head_id)
def test_head_exact(case, dtn, dt):
    """logits with and without bias; dz, dw, db (accumulated into a known start value, gscale = 1/4); two runs bit-equal"""
    from semantic_segmentation_amd import ops
    Cin, k, vol = case
    N, p = d3.HEAD_N, d3.HEAD_PAD[k]
    OD, OH, OW = d3.head_out(case)
    for vset in ("S", "P"):
        r = d3.head_build(case, vset)
        what = f"head3d {d3.head_id(case)} {vset} {dtn}"
        xd = sl(r["x"], dt)
        wdev, bdev, dl = r["w"].to(dev()), r["b"].to(dev()), r["dy"].to(dev())
        y = full((N, 1, OD, OH, OW), torch.float32)
        ops.conv3d_head_fwd(xd, wdev, None, y, k, p)
        er.assert_exact(y.cpu(), er.expect32(r["y"]), what + " logits")
        yb = full((N, 1, OD, OH, OW), torch.float32)
        ops.conv3d_head_fwd(xd, wdev, bdev, yb, k, p)
        er.assert_exact(yb.cpu(), er.expect32(r["y"] + r["b"].double().view(1, 1, 1, 1, 1)), what + " logits + bias")
        runs = []
        for _ in range(2):
            dz = full((N * vol[0], vol[1], vol[2], Cin), dt)
            g = torch.full((1, Cin, k, k, k), 2.0, device=dev())
            db = torch.full((1,), -3.0, device=dev())
            ops.conv3d_head_bwd(xd, wdev, dl, dz, g, db, k, p, d3.GSCALE)
            runs.append((dz, g, db))
        dz, g, db = runs[0]
        er.assert_exact(dz.cpu(), er.expect16(d3.slices(r["dx"]), dt), what + " dz")
        er.assert_exact(g.cpu(), er.expect32(r["dw"] * d3.GSCALE + 2.0), what + " dw (accumulated onto 2)")
        er.assert_exact(db.cpu(), er.expect32(r["db"] * d3.GSCALE - 3.0), what + " db (accumulated onto -3)")
        for a, b in zip(runs[0], runs[1]):
            assert torch.equal(a.view(torch.int16) if a.dtype == dt else a, b.view(torch.int16) if b.dtype == dt else b), "two runs differ"
        # the halves alone: dz without the weight gradient, the weight gradient without dz
        dz2 = full(dz.shape, dt)
        ops.conv3d_head_bwd(None, wdev, dl, dz2, None, None, k, p, d3.GSCALE)
        assert torch.equal(dz2.view(torch.int16), dz.view(torch.int16))
        g2, db2 = torch.full_like(g, 2.0), torch.full_like(db, -3.0)
        ops.conv3d_head_bwd(xd, wdev, dl, None, g2, db2, k, p, d3.GSCALE)
        assert torch.equal(g2, g) and torch.equal(db2, db)


@pytest.mark.parametrize("dtn,dt", er.DTS)
@pytest.mark.parametrize("case", d3.ENGINE_CASES, ids=d3.engine_id)
def test_generic_engine_at_64_depth_taps_exact(case, dtn, dt):
    """Conv3d k4 / pad 1, stride 2 and 1, through gs_conv_igemm with ops.geom_conv3d: forward with bias + LeakyReLU and BatchNorm tile
    partials; the data gradient (stride 1: one 64-tap launch; stride 2: the eight sub-voxel classes of eight taps, launched singly and as the
    two gs_conv_igemm_batch launches of four the engine makes);
    the deterministic weight gradient straight into [Cout][Cin][4][4][4].  The 5-D weight goes through pack_weight as its
    [Cout][Cin][16][4] view: slot (kz*4 + ky)*4 + kx."""
    from semantic_segmentation_amd import ops
    Cin, Cout, s, vol = case
    N, (D, H, W) = d3.ENGINE_N, vol
    OD, OH, OW = d3.engine_out(case)
    geom = ops.geom_conv3d(N, D, H, W, Cin, Cout, 4, s, 1)
    for vset in ("S", "P"):
        r = d3.engine_build(case, vset)
        what = f"engine3d {d3.engine_id(case)} {vset} {dtn}"
        wf = torch.empty(64, Cout, Cin, dtype=dt, device=dev())
        wd = torch.empty(64, Cin, Cout, dtype=dt, device=dev())
        ops.pack_weight(ops.conv3d_weight_view(r["w"].to(dev())), wf, wd, False)
        er.assert_exact(wf.float().cpu(), d3.pack_slots(r["w"], False), what + " pack [slot][co][ci]")
        er.assert_exact(wd.float().cpu(), d3.pack_slots(r["w"], True), what + " pack [slot][ci][co]")
        xd, dyd = sl(r["x"], dt), sl(r["dy"], dt)
        y = full((N * OD, OH, OW, Cout), dt)
        ops.conv_igemm(geom, xd, wf, y)
        er.assert_exact(y.cpu(), er.expect16(d3.slices(r["y"]), dt), what + " forward")
        nt = ops.conv_igemm_mtiles(geom)
        part = torch.full((ops.bn_partials_numel(nt, Cout),), float("nan"), device=dev())
        y2 = full((N * OD, OH, OW, Cout), dt)
        ops.conv_igemm(geom, xd, wf, y2, r["b"].to(dev()), part, ACT_LEAKY02)
        er.assert_leaky_exact(y2.cpu(), d3.slices(r["y"] + r["b"].double().view(1, -1, 1, 1, 1)), what + " forward + bias + leaky")
        want_dx = er.expect16(d3.slices(r["dx"]), dt)
        dx = full((N * D, H, W, Cin), dt)
        if s == 1:
            ops.conv_igemm(ops.geom_conv3d_dgrad_s1(N, D, H, W, Cin, Cout, 4, 1), dyd, wd, dx)
        else:
            for cls in range(8):
                g = ops.geom_conv3d_s2_dgrad_class(N, D, H, W, Cin, Cout, 4, 1, cls >> 2, (cls >> 1) & 1, cls & 1)
                assert g.ntaps == 8
                ops.conv_igemm(g, dyd, wd, dx)
        er.assert_exact(dx.cpu(), want_dx, what + " data gradient")
        if s == 2:                                          # as the engine launches them: two gs_conv_igemm_batch calls of four classes
            gds = [ops.geom_conv3d_s2_dgrad_class(N, D, H, W, Cin, Cout, 4, 1, cls >> 2, (cls >> 1) & 1, cls & 1) for cls in range(8)]
            dxb = full((N * D, H, W, Cin), dt)
            ops.conv_igemm_batch(gds[:4], dyd, [wd] * 4, dxb)
            ops.conv_igemm_batch(gds[4:], dyd, [wd] * 4, dxb)
            er.assert_exact(dxb.cpu(), want_dx, what + " data gradient, two batched launches")
        outs = []
        for _ in range(2):
            ws = torch.full((max(ops.conv_wgrad_ws_floats(geom), 1),), float("nan"), device=dev())
            g_ = torch.full((Cout, Cin, 4, 4, 4), float("nan"), device=dev())
            ops.conv_wgrad_det(geom, xd, dyd, ws, g_, Cout, Cin, 64, d3.GSCALE)
            outs.append(g_)
        er.assert_exact(outs[0].cpu(), er.expect32(r["dw"], d3.GSCALE), what + " weight gradient (deterministic)")
        assert torch.equal(outs[0], outs[1]), "two weight-gradient runs differ"


def test_batchnorm_partials_of_a_3d_launch_sum_to_the_channel_sums():
    """the tile partials gs_conv_igemm writes for a 3-D geometry, finalised with count N*OD*OH*OW, give the exact batch mean"""
    from semantic_segmentation_amd import ops
    case = (8, 16, 2, (4, 6, 10))
    Cin, Cout, s, (D, H, W) = case
    N = d3.ENGINE_N
    OD, OH, OW = d3.engine_out(case)
    r = d3.engine_build(case, "S")
    dt = torch.float16
    geom = ops.geom_conv3d(N, D, H, W, Cin, Cout, 4, s, 1)
    wf = torch.empty(64, Cout, Cin, dtype=dt, device=dev())
    ops.pack_weight(ops.conv3d_weight_view(r["w"].to(dev())), wf, None, False)
    nt = ops.conv_igemm_mtiles(geom)
    part = torch.zeros(ops.bn_partials_numel(nt, Cout), device=dev())
    y = full((N * OD, OH, OW, Cout), dt)
    ops.conv_igemm(geom, sl(r["x"], dt), wf, y, None, part)
    count = N * OD * OH * OW
    z = [torch.zeros(Cout, device=dev()) for _ in range(4)]
    ones, zeros = torch.ones(Cout, device=dev()), torch.zeros(Cout, device=dev())
    ops.bn_finalize(part, nt, Cout, count, ones, zeros, None, None, 0.1, 1e-5, z[0], z[1], z[2], z[3])
    mean64 = r["y"].double().mean((0, 2, 3, 4))
    assert float((z[2].double().cpu() - mean64).abs().max()) <= 2.0 ** -20 * float(mean64.abs().max() + 1)


def _raw(name, *args):
    from semantic_segmentation_amd import _lib
    return getattr(_lib.load(), name)(*args)


def test_refusals_return_before_any_launch():
    """GS_EINVAL: null or misaligned pointer, bad dtype, volumes that do not match; GS_EUNSUPPORTED: Cin outside 1..16, Cout not a
    multiple of 8 / above 128, another geometry; the head: Cin not a multiple of 8 / above 1024.  The outputs keep their sentinel."""
    N, Cin, D, H, W, Cout = 1, 2, 8, 8, 8, 64
    x = torch.ones(N, 17, D, H, W, device=dev())
    w = torch.ones(136, 17, 4, 4, 4, device=dev())
    y = full((N * 8 * 8 * 8 * 136 + 8,), torch.float16)
    dx = full((N * 17 * D * H * W,), torch.float32)
    g = full((136 * 17 * 64,), torch.float32)
    ws = torch.empty(1 << 20, device=dev())
    st = torch.cuda.current_stream().cuda_stream
    X, Wp, Y, DX, G, WS = x.data_ptr(), w.data_ptr(), y.data_ptr(), dx.data_ptr(), g.data_ptr(), ws.data_ptr()

    def fwd(x=X, w=Wp, y=Y, cin=Cin, cout=Cout, k=4, s=2, p=1, od=4, oh=4, ow=4, dt=0, act=ACT_LEAKY02):
        return _raw("gs_conv3d_img_fwd", x, w, None, y, N, cin, D, H, W, cout, od, oh, ow, k, s, p, act, dt, st)

    def wgrad(x=X, dy=Y, g=G, ws=WS, cin=Cin, cout=Cout, k=4, s=2, p=1, od=4, oh=4, ow=4, dt=0):
        return _raw("gs_conv3d_img_wgrad", x, dy, g, ws, N, cin, D, H, W, cout, od, oh, ow, k, s, p, 1.0, dt, st)

    def dgrad(dy=Y, w=Wp, dx=DX, cin=Cin, cout=Cout, k=4, s=2, p=1, od=4, oh=4, ow=4, dt=0):
        return _raw("gs_conv3d_img_dgrad", dy, w, dx, N, cin, D, H, W, cout, od, oh, ow, k, s, p, 1.0, dt, st)

    for f, ptrs in ((fwd, ("x", "w", "y")), (wgrad, ("x", "dy", "g", "ws")), (dgrad, ("dy", "w", "dx"))):
        for name in ptrs:
            assert f(**{name: None}) == GS_EINVAL, (f.__name__, name, "null")
        assert f(dt=7) == GS_EINVAL, (f.__name__, "dtype")
        assert f(od=5) == GS_EINVAL and f(oh=5) == GS_EINVAL and f(ow=3) == GS_EINVAL, (f.__name__, "volume mismatch")
        for cin in (17, 0):
            assert f(cin=cin) == GS_EUNSUPPORTED, (f.__name__, cin)
        for cout in (12, 136, 0):
            assert f(cout=cout) == GS_EUNSUPPORTED, (f.__name__, cout)
        for (k, s, p, o) in ((3, 1, 1, 8), (4, 1, 1, 7), (4, 2, 0, 3), (1, 2, 0, 4), (2, 2, 0, 4)):
            assert f(k=k, s=s, p=p, od=o, oh=o, ow=o) == GS_EUNSUPPORTED, (f.__name__, k, s, p)
    assert fwd(y=Y + 2) == GS_EINVAL and fwd(x=X + 1) == GS_EINVAL and fwd(w=Wp + 2) == GS_EINVAL
    assert wgrad(dy=Y + 8) == GS_EINVAL and wgrad(g=G + 1) == GS_EINVAL and wgrad(ws=WS + 2) == GS_EINVAL
    assert dgrad(dy=Y + 4) == GS_EINVAL and dgrad(dx=DX + 3) == GS_EINVAL
    assert fwd(act=ACT_RELU) == GS_EUNSUPPORTED

    L = full((N * 7 * 7 * 7,), torch.float32)
    LP = L.data_ptr()

    def hfwd(x=Y, w=Wp, y=LP, cin=64, k=4, p=1, od=7, dt=0):
        return _raw("gs_conv3d_head_fwd", x, w, None, y, N, D, H, W, cin, od, 7, 7, k, p, dt, st)

    def hbwd(x=Y, w=Wp, dl=LP, dz=Y, g=G, db=DX, ws=WS, cin=64, k=4, p=1, od=7, dt=0):
        return _raw("gs_conv3d_head_bwd", x, w, dl, dz, g, db, ws, N, D, H, W, cin, od, 7, 7, k, p, 1.0, dt, st)

    for f in (hfwd, hbwd):
        assert f(w=None) == GS_EINVAL and f(dt=3) == GS_EINVAL and f(od=8) == GS_EINVAL, f.__name__
        for cin in (0, 4, 12, 1032):
            assert f(cin=cin) == GS_EUNSUPPORTED, (f.__name__, cin)
        for (k, p) in ((3, 1), (4, 0), (1, 1), (2, 0)):
            assert f(k=k, p=p) == GS_EUNSUPPORTED, (f.__name__, k, p)
    assert hfwd(x=None) == GS_EINVAL and hfwd(y=None) == GS_EINVAL and hfwd(x=Y + 4) == GS_EINVAL
    assert hbwd(dl=None) == GS_EINVAL and hbwd(g=None) == GS_EINVAL and hbwd(ws=None) == GS_EINVAL and hbwd(dz=Y + 2) == GS_EINVAL
    assert hbwd(x=None) == GS_EINVAL and hbwd(dz=None, g=None, db=None) == GS_EINVAL
    torch.cuda.synchronize()
    assert bool((y == SENT).all()) and bool((dx == SENT).all()) and bool((g == SENT).all()) and bool((L == SENT).all())
    from semantic_segmentation_amd import ops
    with pytest.raises(NotImplementedError, match="1..16"):
        ops.conv3d_img_fwd(torch.ones(1, 17, 8, 8, 8, device=dev()), torch.ones(64, 17, 4, 4, 4, device=dev()), None,
                           torch.empty(4, 4, 4, 64, dtype=torch.float16, device=dev()), 4, 2, 1)
    with pytest.raises(ValueError, match=r"\[N,Cin,D,H,W\]"):
        ops.conv3d_img_fwd(torch.ones(1, 2, 8, 8, device=dev()), torch.ones(64, 2, 4, 4, 4, device=dev()), None,
                           torch.empty(4, 4, 4, 64, dtype=torch.float16, device=dev()), 4, 2, 1)


@pytest.mark.parametrize("dtn,dt", er.DTS)
@pytest.mark.parametrize("case", [(5, 8, 1, (2, 3, 70)), (16, 128, 3, (3, 4, 5))], ids=lambda c: f"c{c[0]}-o{c[1]}-n{c[2]}")
def test_k1_volume_equals_k1_image_with_depth_in_rows(case, dtn, dt):
    """a k1 conv is pointwise and its kernel is rank-free: on random normal operands (summation order shows) conv3d_img_fwd / _wgrad /
    _dgrad on [N,Cin,D,H,W] give the bits of conv_imgwide_fwd / _wgrad / _dgrad on the same memory viewed as [N,Cin,D*H,W]"""
    from semantic_segmentation_amd import ops
    Cin, Cout, N, (D, H, W) = case
    g = torch.Generator().manual_seed(31 * Cin + Cout)
    x = torch.randn(N, Cin, D, H, W, generator=g).to(dev())
    w = torch.randn(Cout, Cin, 1, 1, 1, generator=g).to(dev())
    b = torch.randn(Cout, generator=g).to(dev())
    dy = torch.randn(N * D, H, W, Cout, generator=g).to(dt).to(dev())
    x2, w2, dy2 = x.view(N, Cin, D * H, W), w.view(Cout, Cin, 1, 1), dy.view(N, D * H, W, Cout)
    y3, y2 = full((N * D, H, W, Cout), dt), full((N, D * H, W, Cout), dt)
    ops.conv3d_img_fwd(x, w, b, y3, 1, 1, 0, ACT_LEAKY02)
    ops.conv_imgwide_fwd(x2, w2, b, y2, 1, 1, 0, ACT_LEAKY02)
    assert torch.equal(y3.view(torch.int16).flatten(), y2.view(torch.int16).flatten()), f"k1 forward {dtn}"
    g3, g2 = full(w.shape, torch.float32), full(w2.shape, torch.float32)
    ops.conv3d_img_wgrad(x, dy, g3, 1, 1, 0, d3.GSCALE)
    ops.conv_imgwide_wgrad(x2, dy2, g2, 1, 1, 0, d3.GSCALE)
    assert torch.equal(g3.view(torch.int32).flatten(), g2.view(torch.int32).flatten()), f"k1 weight gradient {dtn}"
    dx3, dx2 = full(x.shape, torch.float32), full(x2.shape, torch.float32)
    ops.conv3d_img_dgrad(dy, w, dx3, 1, 1, 0, d3.GSCALE)
    ops.conv_imgwide_dgrad(dy2, w2, dx2, 1, 1, 0, d3.GSCALE)
    assert torch.equal(dx3.view(torch.int32).flatten(), dx2.view(torch.int32).flatten()), f"k1 data gradient {dtn}"
    assert bool(torch.isfinite(g3).all()) and bool((g3 != SENT).all()) and bool((dx3 != SENT).all()), "outputs were not written"
