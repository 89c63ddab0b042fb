"""gs_conv_imgwide_fwd / _wgrad / _dgrad (csrc/ends_img.hip: the image-side conv of 5..16 channels) at ZERO tolerance on integer
operands (tests/disc_wide_reference.py), f16 and bf16; two runs bit-equal; the refusals return before any launch (GPU only)."""
import pytest
import torch

from tests import disc_wide_reference as dw
from tests import exact_reference as er

pytestmark = pytest.mark.gpu

SENT = 7.0
ACT_NONE, ACT_RELU, ACT_LEAKY02 = 0, 1, 2
GS_EINVAL, GS_EUNSUPPORTED = -1, -3


def dev():
    return torch.device("cuda:0")


def nhwc(t, dt=None):
    t = er.channels_last(t)
    return (t if dt is None else t.to(dt)).to(dev())


@pytest.mark.parametrize("dtn,dt", er.DTS)
@pytest.mark.parametrize("case", dw.CASES, ids=dw.case_id)
def test_forward_exact(case, dtn, dt):
    """plain conv, and conv + bias + LeakyReLU(0.2): every output element is the one correctly rounded value"""
    from semantic_segmentation_amd import ops
    Cin, Cout, k, N, H, W = case
    s, p = dw.GEOM[k]
    OH, OW = dw.out_hw(case)
    for vset in ("S", "P"):
        c = dw.build(case, vset)
        x, w, b = c["x"].to(dev()), c["w"].to(dev()), c["b"].to(dev())
        y = torch.full((N, OH, OW, Cout), SENT, dtype=dt, device=dev())
        ops.conv_imgwide_fwd(x, w, None, y, k, s, p, ACT_NONE)
        er.assert_exact(y.cpu(), er.expect16(er.channels_last(c["y"]), dt), f"imgwide fwd {dw.case_id(case)} {vset} {dtn}")
        y2 = torch.full((N, OH, OW, Cout), SENT, dtype=dt, device=dev())
        ops.conv_imgwide_fwd(x, w, b, y2, k, s, p, ACT_LEAKY02)
        ref = er.channels_last(c["y"] + c["b"].double().view(1, -1, 1, 1))
        er.assert_leaky_exact(y2.cpu(), ref, f"imgwide fwd + bias + leaky {dw.case_id(case)} {vset} {dtn}")
        y3 = torch.full((N, OH, OW, Cout), SENT, dtype=dt, device=dev())
        ops.conv_imgwide_fwd(x, w, b, y3, k, s, p, ACT_LEAKY02)
        assert torch.equal(y2.view(torch.int16), y3.view(torch.int16)), "two forward runs differ"


@pytest.mark.parametrize("dtn,dt", er.DTS)
@pytest.mark.parametrize("case", dw.CASES, ids=dw.case_id)
def test_gradients_exact(case, dtn, dt):
    """weight gradient (one block: the N = 1 case; several slabs; blocks that walk several patches: the long cases) and data gradient
    with gscale = 1/4; the bias gradient of the layer (gs_colsum over dy, as the engines run it); two runs bit-equal"""
    from semantic_segmentation_amd import ops
    Cin, Cout, k, N, H, W = case
    s, p = dw.GEOM[k]
    OH, OW = dw.out_hw(case)
    c = dw.build(case, "S")
    x, w = c["x"].to(dev()), c["w"].to(dev())
    dy = nhwc(c["dy"], dt)
    what = f"{dw.case_id(case)} {dtn}"
    runs = []
    for _ in range(2):
        g = torch.full((Cout, Cin, k, k), SENT, dtype=torch.float32, device=dev())
        ops.conv_imgwide_wgrad(x, dy, g, k, s, p, dw.GSCALE)
        runs.append(g)
    er.assert_exact(runs[0].cpu(), er.expect32(c["dw"], dw.GSCALE), "imgwide wgrad " + what)
    assert torch.equal(runs[0], runs[1]), "two weight-gradient runs differ"
    runs = []
    for _ in range(2):
        dx = torch.full((N, Cin, H, W), SENT, dtype=torch.float32, device=dev())
        ops.conv_imgwide_dgrad(dy, w, dx, k, s, p, dw.GSCALE)
        runs.append(dx)
    er.assert_exact(runs[0].cpu(), er.expect32(c["dx"], dw.GSCALE), "imgwide dgrad " + what)
    assert torch.equal(runs[0], runs[1]), "two data-gradient runs differ"
    ws = torch.empty(1024 * Cout, dtype=torch.float32, device=dev())
    db = torch.full((Cout,), SENT, dtype=torch.float32, device=dev())
    ops.colsum(dy, Cout, 0, N, OH, OW, 0, 0, OH, OW, Cout, dw.GSCALE, ws, db)
    er.assert_exact(db.cpu(), er.expect32(dw.db_right(c["dy"].double()), dw.GSCALE), "bias gradient " + what)


def _raw(name, *args):
    from semantic_segmentation_amd import _lib
    return getattr(_lib.load(), name)(*args)


def test_refusals_return_before_any_launch():
    """GS_EINVAL: null or misaligned pointer, bad dtype; GS_EUNSUPPORTED: Cin outside 5..16, Cout not a multiple of 8 / above 128,
    another geometry.  The output buffers keep their sentinel."""
    N, Cin, H, W, Cout = 1, 6, 8, 8, 64
    x = torch.ones(N, Cin, H, W, device=dev())
    w = torch.ones(136, 17, 4, 4, device=dev())
    y = torch.full((N * 8 * 8 * 136 + 8,), SENT, dtype=torch.float16, device=dev())
    dx = torch.full((N * 17 * H * W,), SENT, device=dev())
    g = torch.full((136 * 17 * 16,), SENT, device=dev())
    ws = torch.empty(1 << 16, device=dev())
    st = torch.cuda.current_stream().cuda_stream
    X, Wp, Y, DX, G, WS = x.data_ptr(), w.data_ptr(), y.data_ptr(), dx.data_ptr(), g.data_ptr(), ws.data_ptr()

    def fwd(x=X, w=Wp, y=Y, cin=Cin, cout=Cout, k=4, s=2, p=1, oh=4, ow=4, dt=0, act=ACT_LEAKY02):
        return _raw("gs_conv_imgwide_fwd", x, w, None, y, N, cin, H, W, cout, oh, ow, k, s, p, act, dt, st)

    def wgrad(x=X, dy=Y, g=G, ws=WS, cin=Cin, cout=Cout, k=4, s=2, p=1, oh=4, ow=4, dt=0):
        return _raw("gs_conv_imgwide_wgrad", x, dy, g, ws, N, cin, H, W, cout, oh, ow, k, s, p, 1.0, dt, st)

    def dgrad(dy=Y, w=Wp, dx=DX, cin=Cin, cout=Cout, k=4, s=2, p=1, oh=4, ow=4, dt=0):
        return _raw("gs_conv_imgwide_dgrad", dy, w, dx, N, cin, H, W, cout, oh, ow, k, s, p, 1.0, dt, st)

    for f, ptrs in ((fwd, ("x", "w", "y")), (wgrad, ("x", "dy", "g", "ws")), (dgrad, ("dy", "w", "dx"))):
        for name in ptrs:
            assert f(**{name: None}) == GS_EINVAL, (f.__name__, name, "null")
        assert f(dt=7) == GS_EINVAL, (f.__name__, "dtype")
        assert f(oh=5) == GS_EINVAL, (f.__name__, "plane mismatch")
        for cin in (4, 17, 0):
            assert f(cin=cin) == GS_EUNSUPPORTED, (f.__name__, cin)
        for cout in (12, 136, 0):
            assert f(cout=cout) == GS_EUNSUPPORTED, (f.__name__, cout)
        for (k, s, p, o) in ((3, 1, 1, 8), (4, 1, 1, 7), (4, 2, 0, 3), (1, 2, 0, 4), (2, 2, 0, 4)):
            assert f(k=k, s=s, p=p, oh=o, ow=o) == GS_EUNSUPPORTED, (f.__name__, k, s, p)
    assert fwd(y=Y + 2) == GS_EINVAL and fwd(x=X + 1) == GS_EINVAL and fwd(w=Wp + 2) == GS_EINVAL
    assert wgrad(dy=Y + 8) == GS_EINVAL and wgrad(g=G + 1) == GS_EINVAL and wgrad(ws=WS + 2) == GS_EINVAL
    assert dgrad(dy=Y + 4) == GS_EINVAL and dgrad(dx=DX + 3) == GS_EINVAL
    assert fwd(act=ACT_RELU) == GS_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == SENT).all()) and bool((dx == SENT).all()) and bool((g == SENT).all())
    from semantic_segmentation_amd import ops
    with pytest.raises(NotImplementedError, match="5..16"):
        ops.conv_imgwide_fwd(torch.ones(1, 4, 8, 8, device=dev()), torch.ones(64, 4, 4, 4, device=dev()), None,
                             torch.empty(1, 4, 4, 64, dtype=torch.float16, device=dev()), 4, 2, 1)


# the small-Cout head at input channel counts that are no 8 * 2^j (ndf 96: the PatchGAN's 384-channel head with k 4, PixelDiscriminator's
# 192-channel one with k 1; 24: fewer chunks than any power-of-two group above 16): (Cin, Cout, k, p), N, H, W = 2, 11, 9
HEAD_CASES = [(384, 1, 4, 1), (192, 1, 1, 0), (24, 2, 1, 0), (40, 1, 4, 1)]


@pytest.mark.parametrize("dtn,dt", er.DTS)
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "cin%d_cout%d_k%d_p%d" % c)
def test_smallcout_head_exact_at_any_multiple_of_8(case, dtn, dt):
    """gs_conv_smallcout_fwd / _bwd on exact_reference.smallcout_build's operands: logits, dx, dw, db at zero tolerance"""
    from semantic_segmentation_amd import ops
    Cin, Cout, k, p = case
    N, H, W = 2, 11, 9
    r = er.smallcout_build(case, "S")
    what = f"smallcout cin{Cin} k{k} {dtn}"
    OH, OW = r["y"].shape[2], r["y"].shape[3]
    xd = nhwc(r["x"], dt)
    wdev, bdev = r["w"].to(dev()), r["b"].to(dev())
    y = torch.full((N, Cout, OH, OW), SENT, device=dev())
    ops.conv_smallcout_fwd(xd, wdev, bdev, y, k, 1, p)
    er.assert_exact(y.cpu(), er.expect32(r["y"].double() + r["b"].double().view(1, -1, 1, 1)), what + " logits")
    dx = torch.full((N, H, W, Cin), SENT, dtype=dt, device=dev())
    g = torch.zeros((Cout, Cin, k, k), device=dev())
    db = torch.zeros((Cout,), device=dev())
    ops.conv_smallcout_bwd(xd, wdev, r["dy"].to(dev()), dx, g, db, k, 1, p, 0.5)
    er.assert_exact(dx.cpu(), er.expect16(er.channels_last(r["dx"]), dt), what + " dx")
    er.assert_exact(g.cpu(), er.expect32(r["dw"], 0.5), what + " dw")
    er.assert_exact(db.cpu(), er.expect32(r["db"], 0.5), what + " db")
