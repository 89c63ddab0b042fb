"""The fragment-order lo plane of the pair-forward conv (include/gsseg.h) and its readers.

Everything here is a bit-for-bit comparison: the fragment-order launch against the dense launch of the same operands (override
gs_pair_lo_set_layout(0)), and each reader on a fragment-order lo plane against the same reader on the dense plane of the same values.
The layout map is rebuilt in plain torch from the documented formula.  Small shapes pin the 8-wave form (conv3x3_set_kernel_form(8))
or cap the persistent grid, because the automatic plan gives tensors this small to the 4-wave form, which keeps the dense plane.

The persistent grid: gs_set_persistent_grid accepts 0 or 8..1024 (tests/test_exact_kernels_gpu.py holds it to refusing 1..3), so
"every block runs eight items" is reached at the lower limit of 8 blocks with 64 items (N=2, H=64, W=128, two cout tiles); the
16-item shape N=2, H=32, W=64 runs under the same cap with two items per block (first item, hand-over, last item).  GPU only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [("f16", torch.float16), ("bf16", torch.bfloat16)]
SENT = 7.0


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


_IDX = {}


def frag_index(N, H, W, C):
    """[N,H,W,C] int64: the element of the fragment-order plane that holds (n, y, x, c) -- the documented map:
    byte offset (((((item*8 + w)*2 + i)*2 + j)*2 + g)*64 + l)*16, dword q, 16-bit half e with
    item = ((n*H/16 + ty)*W/32 + tx)*C/64 + ct, y = 16 ty + 2 w + i, x = 32 tx + 16 g + 8 (q >> 1) + 4 h + 2 (q & 1) + e,
    c = 64 ct + 32 j + l31, l = 32 h + l31."""
    key = (N, H, W, C)
    if key not in _IDX:
        n = torch.arange(N).view(N, 1, 1, 1)
        y = torch.arange(H).view(1, H, 1, 1)
        x = torch.arange(W).view(1, 1, W, 1)
        c = torch.arange(C).view(1, 1, 1, C)
        ty, w, i = y // 16, (y % 16) // 2, y % 2
        tx, xr = x // 32, x % 32
        g, q1, h, q0, e = xr // 16, (xr % 16) // 8, (xr % 8) // 4, (xr % 4) // 2, xr % 2
        ct, j, l31 = c // 64, (c % 64) // 32, c % 32
        item = ((n * (H // 16) + ty) * (W // 32) + tx) * (C // 64) + ct
        byte = (((((item * 8 + w) * 2 + i) * 2 + j) * 2 + g) * 64 + 32 * h + l31) * 16
        _IDX[key] = (byte // 2 + 2 * (2 * q1 + q0) + e).expand(N, H, W, C).contiguous()
        assert _IDX[key].flatten().sort().values.equal(torch.arange(N * H * W * C))      # a permutation of the plane
    return _IDX[key]


def to_dense(frag):
    return frag.flatten()[frag_index(*frag.shape).to(frag.device)]


def to_frag(dense):
    out = torch.empty_like(dense).flatten()
    out[frag_index(*dense.shape).to(dense.device).flatten()] = dense.flatten()
    return out.view(dense.shape)


class pinned:
    """kernel form / persistent grid / lo layout override for the duration of a block"""

    def __init__(self, form=-1, grid=0):
        self.form, self.grid = form, grid

    def __enter__(self):
        from semantic_segmentation_amd import ops
        ops.conv3x3_set_kernel_form(self.form)
        ops.set_persistent_grid(self.grid)

    def __exit__(self, *exc):
        from semantic_segmentation_amd import ops
        ops.pair_lo_set_layout(-1)
        ops.set_persistent_grid(0)
        ops.conv3x3_set_kernel_form(-1)


def conv_operands(N, H, W, K, wrap, cout, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, H, W, wrap, generator=g) * 0.7).to(dt).to(dev())
    pack = (torch.randn(9, cout, K, generator=g) * 0.05).to(dt).to(dev())
    return x, pack


def run_conv(ops, x, pack, N, H, W, K, wrap, cout, lo_layout):
    rows = max(ops.conv3x3_stat_rows(N, H, W, K, cout, pair=True), ops.conv3x3_mtiles(N, H, W, cout))
    part = torch.zeros(ops.bn_partials_numel(rows, cout), dtype=torch.float32, device=dev())
    y_hi = torch.full((N, H, W, cout), SENT, dtype=x.dtype, device=dev())
    y_lo = torch.full((N, H, W, cout), SENT, dtype=x.dtype, device=dev())
    ops.conv3x3_segs(x, pack, y_hi, y_lo, N, H, W, K, wrap, wrap, cout, in_stride=wrap, bn_partials=part, lo_layout=lo_layout)
    torch.cuda.synchronize()
    return y_hi, y_lo, part


# (name, N, H, W, K, wrap, Cout, pinned form, grid cap)
LAYOUT_CASES = [
    ("one_item", 1, 16, 32, 64, 64, 64, 8, 0),
    ("many_items_2tiles_xw_grid8", 2, 32, 64, 192, 128, 128, -1, 8),
    ("eight_items_per_block_xw", 2, 64, 128, 192, 128, 128, -1, 8),
    ("decoder_entry_engine_wrap", 1, 16, 64, 320, 192, 64, 8, 0),        # unet_engine._segs("xw", 128, lo_len=64): K 320, wrap 192
    ("decoder_entry_wrap256", 1, 16, 64, 320, 256, 64, 8, 0),
    # 256 blocks with ONE item each (the automatic plan, full grid): every tile leaves through the flush behind the block's last item,
    # with no MFMA between its passes -- where a store whose data registers were rewritten too early lost values from run to run
    ("one_item_per_block_full_grid", 2, 256, 256, 64, 64, 64, -1, 0),
]


@pytest.mark.parametrize("dtn,dt", DTYPES)
@pytest.mark.parametrize("case", LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_fragment_lo_is_the_dense_lo_permuted(case, dtn, dt):
    from semantic_segmentation_amd import ops
    name, N, H, W, K, wrap, cout, form, grid = case
    x, pack = conv_operands(N, H, W, K, wrap, cout, dt, 5)
    with pinned(form, grid):
        if name == "eight_items_per_block_xw":
            assert N * (H // 16) * (W // 32) * (cout // 64) == 8 * ops.get_persistent_grid()
        ops.pair_lo_set_layout(0)
        assert ops.conv3x3_pair_lo_layout(N, H, W, K, cout) == ops.LO_DENSE
        d_hi, d_lo, d_part = run_conv(ops, x, pack, N, H, W, K, wrap, cout, ops.LO_DENSE)
        ops.pair_lo_set_layout(-1)
        assert ops.conv3x3_pair_lo_layout(N, H, W, K, cout) == ops.LO_FRAGMENT
        f_hi, f_lo, f_part = run_conv(ops, x, pack, N, H, W, K, wrap, cout, ops.LO_FRAGMENT)
        for _ in range(3 if name == "one_item_per_block_full_grid" else 0):          # the same bits on every run
            r_hi, r_lo, r_part = run_conv(ops, x, pack, N, H, W, K, wrap, cout, ops.LO_FRAGMENT)
            assert torch.equal(bits(r_hi), bits(f_hi)) and torch.equal(bits(r_lo), bits(f_lo)) and torch.equal(r_part, f_part)
    assert float(d_lo.float().abs().max()) > 0 and not bool((d_lo == SENT).any())
    assert torch.equal(bits(f_hi), bits(d_hi))
    assert torch.equal(f_part, d_part)
    assert torch.equal(bits(to_dense(f_lo)), bits(d_lo))


@pytest.mark.parametrize("dtn,dt", DTYPES)
def test_ineligible_launch_keeps_the_dense_plane_and_refuses_fragment_order(dtn, dt):
    from semantic_segmentation_amd import _lib, ops
    N, H, W, K, cout = 1, 24, 40, 64, 64
    x, pack = conv_operands(N, H, W, K, K, cout, dt, 6)
    with pinned(8, 0):
        assert ops.conv3x3_pair_lo_layout(N, H, W, K, cout) == ops.LO_DENSE
        a_hi, a_lo, a_part = run_conv(ops, x, pack, N, H, W, K, K, cout, ops.LO_DENSE)
        # the parent path: gs_conv3x3_precise itself
        rows = max(ops.conv3x3_stat_rows(N, H, W, K, cout, pair=True), ops.conv3x3_mtiles(N, H, W, cout))
        b_part = torch.zeros(ops.bn_partials_numel(rows, cout), dtype=torch.float32, device=dev())
        b_hi, b_lo = torch.full_like(a_hi, SENT), torch.full_like(a_lo, SENT)
        dy, dx = ops._tap_arrays(ops.TAPS3_FWD)
        _lib.call("gs_conv3x3_precise", ops._p(x), ops._p(pack), ops._p(b_hi), ops._p(b_lo), None, ops._p(b_part), N, H, W, K, K, 0, K,
                  cout, cout, 0, dy, dx, 0, ops.dt_code(x), ops._stream())
        torch.cuda.synchronize()
        assert torch.equal(bits(a_hi), bits(b_hi)) and torch.equal(bits(a_lo), bits(b_lo)) and torch.equal(a_part, b_part)
        c_hi, c_lo = torch.full_like(a_hi, SENT), torch.full_like(a_lo, SENT)
        c_part = torch.zeros_like(b_part)
        with pytest.raises(RuntimeError):
            ops.conv3x3_segs(x, pack, c_hi, c_lo, N, H, W, K, K, K, cout, in_stride=K, bn_partials=c_part, lo_layout=ops.LO_FRAGMENT)
        torch.cuda.synchronize()
        assert bool((c_hi == SENT).all()) and bool((c_lo == SENT).all()) and not bool(c_part.any())      # nothing was launched
        # an eligible shape without statistics / with a bias is refused as well
        y = torch.full((1, 16, 32, 64), SENT, dtype=dt, device=dev())
        xe, pe = conv_operands(1, 16, 32, 64, 64, 64, dt, 7)
        assert ops.conv3x3_pair_lo_layout(1, 16, 32, 64, 64) == ops.LO_FRAGMENT
        with pytest.raises(RuntimeError):
            ops.conv3x3_segs(xe, pe, y, y.clone(), 1, 16, 32, 64, 64, 64, 64, in_stride=64, lo_layout=ops.LO_FRAGMENT)
    with pytest.raises(RuntimeError):
        ops.pair_lo_set_layout(1)


# ------------------------------------------------------------------------------------------------ readers
def pair_planes(N, H, W, C, dt, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(N, H, W, C, generator=g) * 2.0
    hi = v.to(dt)
    lo = (v - hi.float()).to(dt)
    scale = (torch.rand(C, generator=g) + 0.5).to(dev())
    shift = (torch.randn(C, generator=g) * 0.3).to(dev())
    return hi.to(dev()), lo.to(dev()), scale, shift


@pytest.mark.parametrize("dtn,dt", DTYPES)
@pytest.mark.parametrize("C", [64, 128, 512])
def test_apply_reads_fragment_lo_as_dense_lo(C, dtn, dt):
    """bn_act_apply_split: plain with / without z_lo, into a concat destination (z_stride = 4C), with the pooled pair (with and
    without its lo plane); both traversal orders"""
    from semantic_segmentation_amd import ops
    N, H, W = 2, 16, 64
    hi, lo, scale, shift = pair_planes(N, H, W, C, dt, 20 + C)
    lo_f = to_frag(lo)
    assert not torch.equal(bits(lo_f), bits(lo))

    def run(lo_plane, layout, want_lo, concat, pool, pool_lo):
        zs = 4 * C if concat else 2 * C
        z = torch.full((N, H, W, zs), float("nan"), dtype=dt, device=dev())          # (unwritten channels keep their NaN bits)
        zp = torch.full((N, H // 2, W // 2, 2 * C), float("nan"), dtype=dt, device=dev()) if pool else None
        ops.bn_act_apply_split(hi, lo_plane, scale, shift, 1, z, z[..., zs // 2:] if want_lo else None, zs, 0,
                               zp, zp[..., C:] if (pool and pool_lo) else None, 2 * C if pool else 0, lo_layout=layout)
        torch.cuda.synchronize()
        return z, zp

    try:
        for trav in (0, 1):
            ops.bn_set_traversal(trav)
            for want_lo, concat, pool, pool_lo in ((True, False, False, False), (False, False, False, False), (True, True, False, False),
                                                   (True, True, True, True), (False, False, True, False), (True, False, True, False)):
                zd, zpd = run(lo, ops.LO_DENSE, want_lo, concat, pool, pool_lo)
                zf, zpf = run(lo_f, ops.LO_FRAGMENT, want_lo, concat, pool, pool_lo)
                what = (trav, want_lo, concat, pool, pool_lo)
                assert not bool(torch.isnan(zd[..., :C]).any()), what
                assert torch.equal(bits(zf), bits(zd)), what
                if pool:
                    assert not bool(torch.isnan(zpd[..., :C]).any()), what
                    assert torch.equal(bits(zpf), bits(zpd)), what
    finally:
        ops.bn_set_traversal(-1)
    with pytest.raises(RuntimeError):                     # 24 rows: no fragment-order plane of this shape exists
        z = torch.empty(1, 24, 32, 2 * C, dtype=dt, device=dev())
        ops.bn_act_apply_split(hi[:1, :12].reshape(1, 24, 32, C).contiguous(), lo[:1, :12].reshape(1, 24, 32, C).contiguous(), scale, shift, 1,
                               z, None, 2 * C, 0, lo_layout=ops.LO_FRAGMENT)


@pytest.mark.parametrize("dtn,dt", DTYPES)
@pytest.mark.parametrize("ncls", [1, 2, 4])
def test_heads_read_fragment_lo_as_dense_lo(ncls, dtn, dt):
    from semantic_segmentation_amd import ops
    N, H, W, C = 2, 16, 64, 64
    hi, lo, scale, shift = pair_planes(N, H, W, C, dt, 40 + ncls)
    lo_f = to_frag(lo)
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(ncls, 64, generator=g) * 0.2).to(dev())
    b = torch.randn(ncls, generator=g).to(dev())
    try:
        for trav in (0, 1):
            ops.bn_set_traversal(trav)
            out = []
            for plane, layout in ((lo, ops.LO_DENSE), (lo_f, ops.LO_FRAGMENT)):
                logits = torch.full((N, ncls, H, W), float("nan"), dtype=torch.float32, device=dev())
                lab = torch.full((N, H, W), 255, dtype=torch.uint8, device=dev())
                ops.head1x1_bn_fwd_split(hi, plane, scale, shift, 1, w, b, logits, lo_layout=layout)
                ops.head1x1_labels(hi, plane, w, b, lab, scale, shift, 1, lo_layout=layout)
                torch.cuda.synchronize()
                out.append((logits, lab))
            assert not bool(torch.isnan(out[0][0]).any()) and int(out[0][1].max()) < max(ncls, 2)
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    finally:
        ops.bn_set_traversal(-1)


# ------------------------------------------------------------------------------------------------ network
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_network_is_bit_identical_and_takes_the_fragment_path(dtype, monkeypatch):
    """UNet(1, 2, precise="mixed"), batch 2, 128 x 128, forward + backward: dense everywhere against automatic.  The persistent grid
    is capped at its lower limit (8 blocks), where the plan gives levels 0-2 of a batch this small to the 8-wave form."""
    from oracle import oracle
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd.losses import seg_loss
    from semantic_segmentation_amd.unet import UNet
    sd = oracle.unet_state_dict(1, 2, seed=13)
    x, mask = oracle.synthetic_batch(2, 128, seed=21)
    asked = []
    real = ops.conv3x3_pair_lo_layout

    def counting(N, H, W, K, Cout):
        r = real(N, H, W, K, Cout)
        asked.append((H, r))
        return r

    monkeypatch.setattr(ops, "conv3x3_pair_lo_layout", counting)
    res = []
    with pinned(-1, 8):
        for mode in (0, -1):
            ops.pair_lo_set_layout(mode)
            del asked[:]
            net = UNet(1, 2, compute_dtype=dtype, precise="mixed")
            net.load_state_dict(sd, strict=True)
            net = net.cuda().train()
            logits = net(x.cuda())
            seg_loss(logits, mask.cuda()).backward()
            torch.cuda.synchronize()
            res.append((logits.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}, list(asked)))
    (l0, g0, a0), (l1, g1, a1) = res
    assert a0 and all(r == ops.LO_DENSE for _, r in a0)
    for level in (128, 64, 32):                              # levels 0-2 really ran fragment-order launches
        assert sum(1 for h, r in a1 if h == level and r == ops.LO_FRAGMENT) >= 2, (level, a1)
    assert all(r == ops.LO_DENSE for h, r in a1 if h < 32)
    assert torch.equal(l0, l1)
    assert len(g0) == 64 and g0.keys() == g1.keys()
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
