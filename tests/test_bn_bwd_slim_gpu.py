"""The slim BatchNorm backward kernels (ops.bn_bwd_set_form, csrc/bn.hip SLIM) against the normal ones: two pixels per lane in
flight instead of four, everything else the same, so reduce partials and apply output must be equal bit for bit.

Shape N=3, H=9, W=11: 297 pixels in five tiles of 64, the last one ragged (41 pixels: no multiple of the pixels in flight of
either form).  C = 48 gives six chunk lanes, so 256 % 6 threads only join the barriers; C = 8 keeps one pixel per lane and tile
pass; C = 128 has sixteen lanes per pixel and several passes per tile."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, H, W = 3, 9, 11


def _inputs(dt, C, concat):
    from semantic_segmentation_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 + C + (7 if concat else 0))
    y = torch.randn(N, H, W, C, generator=g).to(dt).to(dev)
    sa, ca = (2 * C, C) if concat else (C, 0)
    dzbuf = torch.randn(N, H, W, sa, generator=g).to(dt).to(dev)      # concat: the other half holds values that must not be read
    coef = torch.stack([1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g),
                        0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)]).to(dev).contiguous()
    c12 = (0.01 * torch.randn(2, C, generator=g)).to(dev).contiguous()
    npart = ops.bn_partials_numel(ops.bn_bwd_tiles(N, H, W), C)
    return y, dzbuf, sa, ca, coef, c12, npart


def _run(form, y, dzbuf, sa, ca, coef, c12, npart):
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd._lib import ACT_RELU
    C = y.shape[3]
    part = torch.zeros(npart, dtype=torch.float32, device=y.device)
    dy = torch.zeros_like(y)
    with ops.bn_bwd_form(form):
        ops.bn_act_bwd_reduce(y, dzbuf, sa, ca, None, coef[0], coef[1], coef[2], coef[3], ACT_RELU, part)
        ops.bn_act_bwd_apply(y, dzbuf, sa, ca, None, coef[0], coef[1], coef[2], coef[3], c12[0], c12[1], ACT_RELU, True, dy)
    torch.cuda.synchronize()
    return part, dy


@pytest.mark.parametrize("rev", [0, 6], ids=["fwd", "rev"])
@pytest.mark.parametrize("concat", [False, True], ids=["dense", "concat"])
@pytest.mark.parametrize("C", [8, 48, 64, 128])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_slim_equals_normal(dt, C, concat, rev):
    from semantic_segmentation_amd import ops
    args = _inputs(dt, C, concat)
    ops.bn_set_traversal(rev)
    try:
        part_n, dy_n = _run(ops.BN_BWD_NORMAL, *args)
        part_s, dy_s = _run(ops.BN_BWD_SLIM, *args)
    finally:
        ops.bn_set_traversal(-1)
    ntiles = ops.bn_bwd_tiles_used(N, H, W, False)
    assert ntiles == 5
    assert torch.isfinite(part_n).all() and part_n[:ntiles * 2 * C].abs().sum() > 0 and dy_n.float().abs().sum() > 0
    assert torch.equal(part_s, part_n)
    assert torch.equal(dy_s, dy_n)


def test_traversal_does_not_change_results():
    """the tail-first order only permutes which block takes which tile"""
    from semantic_segmentation_amd import ops
    args = _inputs(torch.float16, 64, False)
    outs = []
    for rev in (0, 6):
        ops.bn_set_traversal(rev)
        try:
            outs.append(_run(ops.BN_BWD_SLIM, *args))
        finally:
            ops.bn_set_traversal(-1)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_form_argument_is_checked():
    from semantic_segmentation_amd import ops
    with pytest.raises(RuntimeError):
        ops.bn_bwd_set_form(2)
    ops.bn_bwd_set_form(ops.BN_BWD_NORMAL)
