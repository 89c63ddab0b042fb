"""The co-resident BatchNorm backward (ops.bn_bwd_set_form(1), csrc/bn.hip SLIM: per-channel coefficients in LDS, four pixels
per lane in flight) against the normal form, which the exact tests pin: reduce partials and apply output equal bit for bit.

Shape N=3, H=9, W=11 as in test_bn_bwd_slim_gpu.py: 297 pixels in five tiles of 64, the last one ragged (41 pixels: no multiple
of two, four or eight pixels in flight).  The channel counts that test does not reach: C = 24 gives three chunk lanes, so
256 % 3 threads only join the barriers; C = 512 fills one wave per pixel; C = 1024 has 128 lanes per pixel, two unit lanes and
is the largest C whose coefficients the block keeps in LDS; C = 1032 and 2048 take the fallback to the normal kernel.  Each
case runs both traversal orders, and apply with and without the BatchNorm terms.

The engine takes the form from the hand-over of a 128-cout weight gradient until the next join: the last test holds a whole
UNet backward to the one-stream gradients and counts the launches that took it."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

N, H, W = 3, 9, 11


def _inputs(dt, C, concat):
    from semantic_segmentation_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2000 + C + (7 if concat else 0))
    y = torch.randn(N, H, W, C, generator=g).to(dt).to(dev)
    sa, ca = (2 * C, C) if concat else (C, 0)
    dzbuf = torch.randn(N, H, W, sa, generator=g).to(dt).to(dev)      # concat: the other half holds values that must not be read
    coef = torch.stack([1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g),
                        0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)]).to(dev).contiguous()
    c12 = (0.01 * torch.randn(2, C, generator=g)).to(dev).contiguous()
    npart = ops.bn_partials_numel(ops.bn_bwd_tiles(N, H, W), C)
    return y, dzbuf, sa, ca, coef, c12, npart


def _run(form, act, y, dzbuf, sa, ca, coef, c12, npart):
    """reduce partials, apply output with the BatchNorm terms, apply output without them"""
    from semantic_segmentation_amd import ops
    part = torch.zeros(npart, dtype=torch.float32, device=y.device)
    dy_bn, dy_act = torch.zeros_like(y), torch.zeros_like(y)
    with ops.bn_bwd_form(form):
        ops.bn_act_bwd_reduce(y, dzbuf, sa, ca, None, coef[0], coef[1], coef[2], coef[3], act, part)
        ops.bn_act_bwd_apply(y, dzbuf, sa, ca, None, coef[0], coef[1], coef[2], coef[3], c12[0], c12[1], act, True, dy_bn)
        ops.bn_act_bwd_apply(y, dzbuf, sa, ca, None, coef[0], coef[1], coef[2], coef[3], c12[0], c12[1], act, False, dy_act)
    torch.cuda.synchronize()
    return part, dy_bn, dy_act


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "identity"])
@pytest.mark.parametrize("concat", [False, True], ids=["dense", "concat"])
@pytest.mark.parametrize("C", [24, 512, 1024, 1032, 2048])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_coresident_equals_normal(dt, C, concat, relu):
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd._lib import ACT_NONE, ACT_RELU
    args = _inputs(dt, C, concat)
    act = ACT_RELU if relu else ACT_NONE
    ntiles = ops.bn_bwd_tiles_used(N, H, W, False)
    assert ntiles == 5
    for rev in (0, 6):
        ops.bn_set_traversal(rev)
        try:
            ref = _run(ops.BN_BWD_NORMAL, act, *args)
            got = _run(ops.BN_BWD_SLIM, act, *args)
        finally:
            ops.bn_set_traversal(-1)
        part_n, dy_bn_n, dy_act_n = ref
        assert torch.isfinite(part_n).all() and part_n[:ntiles * 2 * C].abs().sum() > 0
        for t in (dy_bn_n, dy_act_n):
            assert torch.isfinite(t.float()).all() and t.float().abs().sum() > 0
        assert not torch.equal(dy_bn_n, dy_act_n)                     # the BatchNorm terms were applied
        for name, a, b in zip(("reduce partials", "apply, bn", "apply, no bn"), got, ref):
            assert torch.equal(a, b), f"{name}, traversal {rev}"


def test_unet_backward_takes_the_form_and_equals_one_stream(monkeypatch):
    """UNet(1, 2) at batch 2, 64 x 64: the gate's two-stream backward against the one-stream one, every parameter gradient.

    The plain launches of levels 1-4 from the first 128-cout hand-over (up3.conv.3) on take the form, whatever was handed to
    the side stream after that weight gradient: up3.conv.0, up2 and up1 (.3 and .0), down4 (.3 and .0) and the .0 stages of
    down3, down2 and down1 -- ten stages, a reduce and an apply each.  The pooled .3 stages, the head stage, level 0 and the
    one-stream backward take none."""
    from oracle import oracle
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd.losses import seg_loss
    from semantic_segmentation_amd.unet import UNet, unet_engine
    dev = torch.device("cuda:0")
    net = UNet(1, 2).to(dev)
    net.load_state_dict(oracle.unet_state_dict(1, 2, seed=7), strict=True)
    net.train()
    x, mask = oracle.synthetic_batch(2, 64, seed=3)
    x, mask = x.to(dev), mask.to(dev)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    taken = []
    form_ctx = ops.bn_bwd_form

    @contextlib.contextmanager
    def counting_form(form):
        taken.append(form)
        with form_ctx(form):
            yield

    monkeypatch.setattr(ops, "bn_bwd_form", counting_form)

    def step(side):
        monkeypatch.setattr(unet_engine, "WGRAD_SIDE_STREAM", side)
        net.load_state_dict(sd)                      # the same BatchNorm running statistics for both runs
        for p in net.parameters():
            p.grad = None
        del taken[:]
        loss = seg_loss(net(x), mask)
        loss.backward()
        torch.cuda.synchronize()
        return ({n: p.grad.clone() for n, p in net.named_parameters()}, net.engine.last_backward_streams,
                taken.count(ops.BN_BWD_SLIM))

    g2, n2, slim2 = step(True)
    g1, n1, slim1 = step(False)
    assert (n2, n1) == (2, 1)
    assert (slim2, slim1) == (20, 0)
    assert len(g1) == 64 and g1.keys() == g2.keys()
    for name in g1:
        assert torch.isfinite(g1[name]).all() and g1[name].abs().sum() > 0, name
        assert torch.equal(g2[name], g1[name]), name
