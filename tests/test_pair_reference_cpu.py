"""CPU tests of tests/pair_reference.py: the fp64 reference the GPU tests of the pair kernels compare against is (a) reproduced by
fp32 arithmetic and (b) by pair rounding to well inside pair_tol, while (c) a missing segment or a shifted x_lo window moves it
by far more than pair_tol -- so tests/test_pair_kernels_gpu.py can fail, and only for the right reason."""
import pytest
import torch
import torch.nn.functional as F

from tests import pair_reference as pr

CASES = ([("conv2d", c) for c in pr.CONV2D_CASES] + [("conv3d", c) for c in pr.CONV3D_CASES] +
         [("upconv", c) for c in pr.UPCONV_CASES])
BUILD = {"conv2d": pr.build_conv2d, "conv3d": pr.build_conv3d, "upconv": pr.build_upconv}


def test_split_and_pack_definitions():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(1000, generator=g)
    for _, dt in pr.DTYPES:
        hi, lo = pr.split(v, dt)
        assert hi.dtype == dt and lo.dtype == dt
        eps = 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8
        assert float((v - hi.float()).abs().max()) <= eps * float(v.abs().max())
        assert float((v - hi.float() - lo.float()).abs().max()) <= eps * eps * float(v.abs().max()) * 1.01
        w = torch.randn(6, 5, 3, 3, generator=g)
        pk = pr.expected_pack(w, [(0, 0, 5), (1, 2, 3), (2, 0, 2), (0, 1, 2)], False, dt)
        wh, wl = pr.split(w, dt)
        assert pk.shape == (9, 6, 12)
        assert torch.equal(pk[4, :, :5], wh[:, :, 1, 1]) and torch.equal(pk[7, :, 5:8], wl[:, 2:5, 2, 1])
        assert float(pk[:, :, 8:10].abs().max()) == 0 and torch.equal(pk[0, :, 10:], wh[:, 1:3, 0, 0])
        wt = torch.randn(5, 6, 2, 2, generator=g)                                    # transposed: [Cin][Cout][ky][kx]
        pt = pr.expected_pack(wt, [(0, 0, 5), (1, 0, 5)], True, dt)
        th, tl = pr.split(wt, dt)
        assert torch.equal(pt[3, :, :5], th[:, :, 1, 1].t()) and torch.equal(pt[2, :, 5:], tl[:, :, 1, 0].t())
    assert pr.k_channels(8, 6).tolist() == [0, 1, 2, 3, 4, 5, 0, 1]
    assert pr.k_channels(8, 6, 4).tolist() == [0, 1, 2, 3, 4, 5, 4, 5]


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("kind", ["conv2d", "conv3d", "upconv"])
def test_split_layout_is_the_product_without_the_lo_lo_term(kind, dtn, dt):
    """[hi | hi | lo] applied to [x_hi | x_lo | x_hi] = conv(x_hi + x_lo, w_hi + w_lo) - conv(x_lo, w_lo), in all three forms"""
    g = torch.Generator().manual_seed(4)
    cin, cout = 16, 8
    segs = [(0, 0, cin), (0, 0, cin), (1, 0, cin)]
    if kind == "conv2d":
        v, w = pr.make_values(g, 2, 7, 9, cin), pr.make_weight(g, cout, cin, 3, 3)
        conv = lambda a, b: F.conv2d(a.permute(0, 3, 1, 2), b, padding=1).permute(0, 2, 3, 1)
        kw, taps, tr = {}, 9, False
    elif kind == "conv3d":
        v, w = pr.make_values(g, 2, 3, 5, 6, cin), pr.make_weight(g, cout, cin, 3, 3, 3)
        conv = lambda a, b: F.conv3d(a.permute(0, 4, 1, 2, 3), b, padding=1).permute(0, 2, 3, 4, 1)
        kw, taps, tr = {}, 27, False
    else:
        v, w = pr.make_values(g, 2, 4, 5, cin), pr.make_weight(g, cout, cin, 2, 2, transposed=True)
        conv = lambda a, b: F.pad(F.conv_transpose2d(a.permute(0, 3, 1, 2), b, stride=2), [1, 0, 0, 1]).permute(0, 2, 3, 1)
        kw, taps, tr = dict(out_hw=(9, 11), off=(0, 1)), 4, True
    xh, xl = (t.double() for t in pr.split(v, dt))
    wh, wl = (t.double() for t in pr.split(w, dt))
    got = pr.pair_conv_ref(pr.make_window(v, dt, 0, cin, 2 * cin), pr.expected_pack(w, segs, tr, dt), taps, **kw)
    want = conv(xh + xl, wh + wl) - conv(xl, wl)
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())
    if kind == "upconv":
        own = pr.upconv_owned(4, 5, 9, 11, 0, 1)
        assert float(got[:, ~own].abs().max()) == 0.0 and float(got[:, own].abs().min()) > 0.0


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("kind,case", CASES, ids=[f"{k}-{c[0]}" for k, c in CASES])
def test_reference_resolves_pair_tol(kind, case, dtn, dt):
    """for every case of the GPU tests: fp32 evaluation and pair rounding stay within pair_tol / 2 of the fp64 reference; zeroing a
    segment or rolling the x_lo window by 8 channels moves it by at least 20 * pair_tol"""
    c = BUILD[kind](case, dt)
    ref = pr.case_ref(c, dt)
    scale = float(ref.abs().max())
    tol = pr.pair_tol(dt, scale)
    assert torch.isfinite(ref).all() and scale > 0.3
    # (a) the same sum in fp32
    r32 = pr.case_ref(c, dt, dtype=torch.float32)
    assert float((r32.double() - ref).abs().max()) < 0.5 * tol, (float((r32.double() - ref).abs().max()), tol)
    # (b) the fp64 value rounded to a pair
    hi, lo = pr.split(ref.float(), dt)
    assert float((hi.double() + lo.double() - ref).abs().max()) < 0.5 * tol
    # (c) every non-zero segment matters.  The sum in front of the activation is linear in the segments: the reference without
    # segment j is act(pre - the segment's own contribution)
    lin = dict(bias=None, act=None)
    act = torch.relu if c["act"] == "relu" else (lambda t: t)
    pre = pr.case_ref(c, dt, act=None) if c["act"] is not None else ref
    ranges = pr.seg_ranges(c["segs"])
    for j, (kind_, k0, k1) in enumerate(ranges):
        if kind_ == 2:
            continue
        part = pr.case_ref(c, dt, ksel=torch.arange(k0, k1), **lin)
        delta = float((act(pre - part) - ref).abs().max())
        assert delta > 20 * tol, (j, c["segs"][j], delta, tol)
    # ... and so does the place the x_lo segment reads: the lo channels of the window rolled by 8
    if len(ranges) > 1 and ranges[1][0] == 0:
        _, k0, k1 = ranges[1]
        kc = pr.k_channels(c["K"], c["wrap"], c["wrap_to"])[k0:k1]
        win = c["win"].clone()
        win[..., kc] = torch.roll(c["win"][..., kc], 8, dims=-1)
        ksel = torch.arange(k0, k1)
        moved = pr.case_ref(c, dt, ksel=ksel, win=win, **lin) - pr.case_ref(c, dt, ksel=ksel, **lin)
        delta = float((act(pre + moved) - ref).abs().max())
        assert delta > 20 * tol, ("x_lo window rolled", delta, tol)
    # a zero segment contributes nothing, whatever finite values sit under it
    pads = pr.pad_only_channels(c["segs"], c["K"], c["wrap"], c["wrap_to"])
    if pads:
        win = c["win"].clone()
        win[..., pads] = -3.0
        assert torch.equal(pr.case_ref(c, dt, win=win), ref)


def test_case_lists_cover_the_edges():
    """what the GPU tests rely on the lists to contain"""
    f16 = torch.float16
    pads = {c[0] for c in pr.CONV3D_CASES
            if pr.pad_only_channels(*(lambda b: (b["segs"], b["K"], b["wrap"], b["wrap_to"]))(pr.build_conv3d(c, f16)))}
    assert {"tail_x", "tail_xw_mid"} <= pads
    assert {c[2] for c in pr.CONV3D_CASES} == {1, 2, 3, 4} and any(c[1] > 1 for c in pr.CONV3D_CASES)
    assert any(pr.build_conv3d(c, f16)["wrap_to"] == 128 and c[6] == 128 and c[7] == 64 for c in pr.CONV3D_CASES)
    assert any(c[5] == 32 and pr.build_conv3d(c, f16)["K"] == 128 for c in pr.CONV3D_CASES)
    c2 = pr.CONV2D_CASES
    assert {c[7] for c in c2} == {"1", "x", "w", "xw", "xw-"} and {c[6] for c in c2} == {64, 72, 192}
    assert {c[8] for c in c2} == {-1, 0, 4, 8, 44} and any(c[3] < 24 for c in c2) and any(c[5] == c[4] // 2 for c in c2)
    assert all(c[9] % 8 == 0 and c[10] % 8 == 0 for c in c2) and any(c[11] for c in c2) and any(c[12] == "relu" for c in c2)
    assert {c[7] for c in pr.UPCONV_CASES} >= {(0, 0), (0, 1), (1, 0)}
    assert all(pr.case_ref(pr.build_conv2d(c, f16), f16).numel() <= 500_000 for c in c2)


def test_segs3d_lays_zero_segments_over_written_lo_channels_only():
    """unet3d_engine.segs3d: a zero (kind 2) segment multiplies the input channels under it, and 0 * NaN = NaN; the pair forward
    writes the first lo_len lo channels of a buffer from torch.empty and nothing behind them.  So every layout segs3d returns
    walks [0, cin + lo_len) at most and stays inside the 2 * cin channels of the buffer; what would need more raises
    NotImplementedError (the "auto" mode then runs the 16-bit engine)."""
    from semantic_segmentation_amd.unet3d.unet3d_engine import segs3d
    n_ok = n_refused = 0
    for cin in range(8, 400, 8):
        for lo0, ll in [(0, None)] + [(cin - r, r) for r in range(8, cin, 8)]:
            for mode in ("1", "x", "w", "xw", "xw-"):
                try:
                    segs, K, wrap = segs3d(mode, cin, lo0, ll)
                except NotImplementedError:
                    n_refused += 1
                    continue
                n_ok += 1
                valid = cin + (cin if ll is None else ll)
                wrap_to = lo0 if mode == "xw-" else 0
                kc = pr.k_channels(K, wrap, wrap_to)
                assert int(kc.max()) < valid <= 2 * cin, (mode, cin, lo0, ll, segs)
                for (kind, ci0, ln), (_, k0, k1) in zip(segs, pr.seg_ranges(segs)):      # weights meet the channels they belong to
                    if kind == 2:
                        continue
                    ch = kc[k0:k1]
                    hi_plane = ch < cin
                    want = torch.arange(ci0, ci0 + ln)
                    got = torch.where(hi_plane, ch, ch - cin + lo0)
                    assert torch.equal(got, want), (mode, cin, lo0, ll, segs)
    assert n_ok > 1000 and n_refused > 0
    # "x" on a concat buffer [up_h res_h | res_l -] / on a plain pair whose walk would need a pad behind the lo channels
    for args in (("x", 136, 96, 40), ("xw", 128, 88, 40), ("xw", 80, 0, None), ("x", 40, 0, None)):
        with pytest.raises(NotImplementedError):
            segs3d(*args)
    for name, (segs, K, wrap) in pr.CONV3D_LAYOUTS.items():                              # ... which the kernel tests keep exercising
        assert pr.pad_only_channels(segs, K, wrap)
