"""The image-side tail of the 3-D Pix2Pix generator (csrc/gen3d.hip: gs_conv3d_tail_fwd / _bwd_ws_floats / _bwd) at ZERO tolerance
on integer operands (tests/gen3d_reference.py), f16 and bf16: the fp32 image equal to the fp64 statement, dx equal after one correct
16-bit rounding, dw / db exact (a sparse dout keeps every fp32 sum exact in any order), two runs bit-equal, dx and dw / db separable.
With act = tanh: |t - tanh64(pre)| <= 2^-20 on operands whose pre-activation is an exact fp32 number, and the gradients through the
kernel's own t within the project's bound of the statement.  The refusals return before any launch (GPU only)."""
import ctypes

import pytest
import torch

from tests import cell3d_reference as c3
from tests import exact_reference as er
from tests import gen3d_reference as g3
from tests.backward_replay import compare

pytestmark = pytest.mark.gpu

SENT = 7.0
GS_EINVAL, GS_EUNSUPPORTED = -1, -3
ACT_NONE, ACT_TANH = 0, 3


def dev():
    return torch.device("cuda:0")


def full(shape, dtype):
    return torch.full(tuple(shape), SENT, dtype=dtype, device=dev())


def same_bits(a, b):
    return torch.equal(a.view(torch.int16) if a.element_size() == 2 else a, b.view(torch.int16) if b.element_size() == 2 else b)


@pytest.mark.parametrize("dtn,dt", er.DTS)
@pytest.mark.parametrize("case", g3.TAIL_CASES, ids=g3.tail_id)
def test_tail_exact(case, dtn, dt):
    from semantic_segmentation_amd import ops
    Cin, Cout, N, (D, H, W) = case
    r = g3.tail_build(case)
    what = f"tail3d {g3.tail_id(case)} {dtn}"
    x16 = c3.slices(r["x"]).to(dt).to(dev())
    w, b, dout = r["w"].to(dev()), r["b"].to(dev()), r["dout"].to(dev())
    out = full((N, Cout, D, H, W), torch.float32)
    ops.conv3d_tail_fwd(x16, w, b, out, ACT_NONE)
    er.assert_exact(out.cpu(), er.expect32(r["t"]), what + " forward + bias")
    out2 = full(out.shape, torch.float32)
    ops.conv3d_tail_fwd(x16, w, b, out2, ACT_NONE)
    assert torch.equal(out, out2), "two forward runs differ"
    nob = full(out.shape, torch.float32)
    ops.conv3d_tail_fwd(x16, w, None, nob, ACT_NONE)
    er.assert_exact(nob.cpu(), er.expect32(r["t"] - r["b"].double().view(1, -1, 1, 1, 1)), what + " forward without bias")
    runs = []
    for _ in range(2):
        dx, dw, db = full(x16.shape, dt), full(w.shape, torch.float32), full((Cout,), torch.float32)
        ops.conv3d_tail_bwd(x16, w, None, dout, dx, dw, db, ACT_NONE, g3.TAIL_GSCALE)
        runs.append((dx, dw, db))
    dx, dw, db = runs[0]
    tag = what + f" (dout density {r['density']})"
    er.assert_exact(dx.cpu(), er.expect16(c3.slices(r["dx"]), dt), tag + " data gradient")
    er.assert_exact(dw.cpu(), er.expect32(r["dw"]), tag + " weight gradient")
    er.assert_exact(db.cpu(), er.expect32(r["db"]), tag + " bias gradient")
    for a, bb in zip(runs[0], runs[1]):
        assert same_bits(a, bb), "two backward runs differ"
    # the parts on their own: dx without dw / db (x is then not read), dw / db without dx
    dx1 = full(x16.shape, dt)
    ops.conv3d_tail_bwd(None, w, None, dout, dx1, None, None, ACT_NONE, g3.TAIL_GSCALE)
    assert same_bits(dx1, dx)
    dw1, db1 = full(w.shape, torch.float32), full((Cout,), torch.float32)
    ops.conv3d_tail_bwd(x16, w, None, dout, None, dw1, db1, ACT_NONE, g3.TAIL_GSCALE)
    assert torch.equal(dw1, dw) and torch.equal(db1, db)


@pytest.mark.parametrize("dtn,dt", er.DTS)
@pytest.mark.parametrize("case", [g3.TAIL_CASES[2], g3.TAIL_CASES[3]], ids=g3.tail_id)
def test_tail_tanh(case, dtn, dt):
    from semantic_segmentation_amd import ops
    Cin, Cout, N, (D, H, W) = case
    x, w, b, dout = g3.tail_tanh_inputs(case)
    S = 1024.0
    x16 = c3.slices(x).to(dt).to(dev())
    assert torch.equal(x16.float().cpu(), c3.slices(x))                # integers: nothing is lost in the 16-bit store
    t = full((N, Cout, D, H, W), torch.float32)
    ops.conv3d_tail_fwd(x16, w.to(dev()), b.to(dev()), t, ACT_TANH)
    r64 = g3.tail_statement(x, w, b, dout, gscale=S, t_given=t.cpu())
    pre = g3.tail_statement(x, w, b, act="none")["t"]
    assert torch.equal(pre.float().double(), pre), "the pre-activation of this case must be an fp32 number"
    d = float((t.cpu().double() - r64["t"]).abs().max())
    print(f"tail3d tanh {g3.tail_id(case)} {dtn}: max |t - tanh64(pre)| = {d:.3e} (bound {2.0 ** -20:.3e}), pre in "
          f"{float(pre.min()):.2f} .. {float(pre.max()):.2f}")
    assert d <= 2.0 ** -20
    runs = []
    for _ in range(2):
        dx, dw, db = full(x16.shape, dt), full(w.shape, torch.float32), full((Cout,), torch.float32)
        ops.conv3d_tail_bwd(x16, w.to(dev()), t, dout.to(dev()), dx, dw, db, ACT_TANH, S)
        runs.append((dx, dw, db))
    for a, bb in zip(runs[0], runs[1]):
        assert same_bits(a, bb), "two backward runs differ"
    # du through dx / dw / db, at the kernel's own t: the statement in fp64 and with dx stored in 16 bits
    r16 = g3.tail_statement(x, w, b, dout, gscale=S, t_given=t.cpu(), store=dt)
    got = dict(dx=c3.volume(runs[0][0].float().cpu(), N), dw=runs[0][1].cpu(), db=runs[0][2].cpu())
    keys = ("dx", "dw", "db")
    rep, bad = compare(got, {k: r64[k] for k in keys}, {k: r16[k] for k in keys}, {k: 0.0 for k in keys})
    for k in keys:
        print(f"  {k}: err {rep[k]['err']:.3e} e16 {rep[k]['e16']:.3e} ratio {rep[k]['ratio']:.2f} rows {rep[k]['row_worst']:.2f}")
    assert not bad, (bad, rep)


def test_refusals_launch_nothing():
    from semantic_segmentation_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    N, D, H, W = 1, 2, 3, 4
    x = full((N * D, H, W, 64 + 8), torch.float16)
    w = full((4 * 72 * 27,), torch.float32)
    img = full((N, 5, D, H, W), torch.float32)
    dx = full(x.shape, torch.float16)
    ws = full((1 << 16,), torch.float32)

    def fwd(xp=x.data_ptr(), wp=w.data_ptr(), op=img.data_ptr(), cin=8, cout=1, act=ACT_TANH, dtype=0, n=N):
        return lib.gs_conv3d_tail_fwd(P(xp), P(wp), None, P(op), n, D, H, W, cin, cout, act, dtype, None)

    def bwd(xp=x.data_ptr(), wp=w.data_ptr(), tp=img.data_ptr(), dp=img.data_ptr(), dxp=dx.data_ptr(), dwp=w.data_ptr(),
            dbp=w.data_ptr(), wsp=ws.data_ptr(), cin=8, cout=1, act=ACT_TANH, dtype=0):
        return lib.gs_conv3d_tail_bwd(P(xp), P(wp), P(tp), P(dp), P(dxp), P(dwp), P(dbp), P(wsp), N, D, H, W, cin, cout, act, 1.0,
                                      dtype, None)

    unsupported = [fwd(cin=12), fwd(cin=72), fwd(cout=5), fwd(cout=0), fwd(act=1), bwd(cin=12), bwd(cin=72), bwd(cout=5), bwd(act=2)]
    assert all(rc == GS_EUNSUPPORTED for rc in unsupported), unsupported
    assert b"multiple of 8 up to 64" in lib.gs_last_error()
    invalid = [fwd(xp=None), fwd(wp=None), fwd(op=None), fwd(xp=x.data_ptr() + 2), fwd(dtype=5), fwd(n=0),
               bwd(wp=None), bwd(dp=None), bwd(tp=None), bwd(xp=None), bwd(wsp=None), bwd(dbp=None), bwd(dxp=None, dwp=None, dbp=None),
               bwd(dxp=dx.data_ptr() + 2)]
    torch.cuda.synchronize()
    assert all(rc == GS_EINVAL for rc in invalid), invalid
    for t in (x, w, img, dx, ws):
        assert bool((t == SENT).all()), "a refused call wrote something"
    assert lib.gs_conv3d_tail_bwd_ws_floats(0, 1, 1, 1, 8, 1) == 0
    assert lib.gs_conv3d_tail_bwd_ws_floats(N, D, H, W, 8, 2) >= 2 * 8 * 27 + 2


def test_symbols_exported():
    from semantic_segmentation_amd import _lib, ops
    lib = _lib.load()
    for name in ("gs_conv3d_tail_fwd", "gs_conv3d_tail_bwd_ws_floats", "gs_conv3d_tail_bwd"):
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None
    assert callable(ops.conv3d_tail_fwd) and callable(ops.conv3d_tail_bwd)


def test_wrapper_refuses_with_the_limits():
    from semantic_segmentation_amd import ops
    x = full((2, 3, 4, 12), torch.float16)
    out = full((1, 1, 2, 3, 4), torch.float32)
    with pytest.raises(NotImplementedError, match="multiple of 8 up to 64"):
        ops.conv3d_tail_fwd(x, full((1, 12, 3, 3, 3), torch.float32), None, out, ACT_TANH)
    with pytest.raises(ValueError):
        ops.conv3d_tail_fwd(x, full((1, 8, 3, 3, 3), torch.float32), None, out, ACT_TANH)
    assert bool((out == SENT).all())
