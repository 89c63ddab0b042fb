"""Networks with 5..64 classes end to end (GPU only, `-m gpu`): UNet3D in the default (pair) and the fast (16-bit) mode against the
fp32 oracle, more than 64 classes refused by name, `evaluate()` on a nine-class UNet, and the 2-D head's backward as ONE call of
the wide kernel.  The reference takes any class count (unet/unet_model.py:8-24, GenSeg-3D/UNet3D/unet3d.py:89-126)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu
REPORT = {}
LIMITS3D_DEFAULT = dict(max=1e-3, mean=1.2e-4)              # tests/test_unet3d_gpu.py LIMITS["default"], restated
LIMITS3D_FAST = dict(max=3.6e-3, mean=6.6e-4)               # tests/test_unet3d_gpu.py LIMITS["fast"], restated


def _dump():
    """the measured figures as parity_wide_heads.json under $GSSEG_REPORT_DIR, when that is set (each test prints its own as well)"""
    out = os.environ.get("GSSEG_REPORT_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "parity_wide_heads.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def _wrap_pair(eng):
    ran = []
    inner = eng.forward_pair
    eng.forward_pair = lambda *a, **k: (ran.append(1), inner(*a, **k))[1]
    return ran


_REF3D = {}


def ref3d(cin, ncls):
    """the oracle's train-mode step on one 16^3 volume, the mask random classes in [0, ncls); computed once per net"""
    if (cin, ncls) not in _REF3D:
        sd = oracle.unet3d_state_dict(cin, ncls, seed=23 + cin)
        g = torch.Generator().manual_seed(cin)
        x = torch.randn(1, cin, 16, 16, 16, generator=g)
        mask = torch.randint(0, ncls, (1, 16, 16, 16), generator=g)
        ref_p = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in sd.items()}
        ref_logits = oracle.unet3d_forward(ref_p, x, train=True)
        n, c, dd, hh, ww = ref_logits.shape
        ref_loss = oracle.seg_loss(ref_logits.reshape(n, c, dd * hh, ww), mask.reshape(n, dd * hh, ww))
        ref_loss.backward()
        _REF3D[(cin, ncls)] = dict(sd=sd, x=x, mask=mask, logits=ref_logits.detach(), loss=float(ref_loss.detach()),
                                   grads={k: v.grad for k, v in ref_p.items() if v.requires_grad})
    return _REF3D[(cin, ncls)]


def run3d(cin, ncls, **kw):
    from semantic_segmentation_amd.losses import seg_loss
    from semantic_segmentation_amd.unet3d import UNet3D
    r = ref3d(cin, ncls)
    net = UNet3D(cin, ncls, **kw)
    net.load_state_dict(r["sd"], strict=True)
    net = net.cuda().train()
    ran = _wrap_pair(net.engine)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        logits = net(r["x"].cuda())
    assert not [str(w.message) for w in rec if "16-bit engine" in str(w.message)], "a covered configuration warned"
    n, c, dd, hh, ww = r["logits"].shape
    assert tuple(logits.shape) == (n, c, dd, hh, ww)
    loss = seg_loss(logits.reshape(n, c, dd * hh, ww), r["mask"].cuda().reshape(n, dd * hh, ww))
    loss.backward()
    torch.cuda.synchronize()
    d = (logits.detach().cpu() - r["logits"]).abs()
    errs = {}
    for k, p in net.named_parameters():
        g = r["grads"][k]
        assert p.grad.shape == g.shape, k
        if k.endswith("conv1.bias") or k.endswith("conv2.bias"):
            continue                                # a bias in front of a batch-statistics BatchNorm: true gradient 0
        errs[k] = float((p.grad.cpu() - g).norm() / (g.norm() + 1e-12))
    assert "s_block1.conv3.weight" in errs and "s_block1.conv3.bias" in errs
    out = {"pair": bool(ran), "logit_max_abs": float(d.max()), "logit_mean_abs": float(d.mean()),
           "loss_abs_err": abs(float(loss) - r["loss"]), "grad_rel_err_median": float(np.median(list(errs.values()))),
           "grad_rel_err_worst": max(errs.values()), "worst_key": max(errs, key=errs.get),
           "head_weight_grad_rel_err": errs["s_block1.conv3.weight"], "head_bias_grad_rel_err": errs["s_block1.conv3.bias"]}
    return out, errs


@pytest.mark.parametrize("cin,ncls", [(1, 6), (2, 9)])
def test_default_unet3d_with_wide_head_meets_1e3(cin, ncls):
    """`UNet3D(C, ncls)` with more than four classes as built by default: forward_pair ran, no fallback warning, logits within the
    default mode's limits, the loss within 1e-3, every gradient of the reference's shape, per-tensor relative L2 median < 0.15 and
    worst < 0.3 (the head's own conv3.weight / conv3.bias included) -- written as test_default_unet3d_multi_channel_meets_1e3 is."""
    out, errs = run3d(cin, ncls)
    REPORT[f"default3d_{cin}_{ncls}"] = out
    _dump()
    print(out)
    assert out["pair"], "the default UNet3D did not run the pair forward"
    assert out["logit_max_abs"] < LIMITS3D_DEFAULT["max"] and out["logit_mean_abs"] < LIMITS3D_DEFAULT["mean"], out
    assert out["loss_abs_err"] < 1e-3, out
    assert out["grad_rel_err_median"] < 0.15 and out["grad_rel_err_worst"] < 0.3, errs


def test_fast_unet3d_with_wide_head():
    """UNet3D(1, 6, precise=False): the 16-bit engine with the single-plane wide head forward; logits within LIMITS["fast"] of
    tests/test_unet3d_gpu.py, the gradient bounds of the default mode's test"""
    out, errs = run3d(1, 6, precise=False)
    REPORT["fast3d_1_6"] = out
    _dump()
    print(out)
    assert not out["pair"]
    assert out["logit_max_abs"] < LIMITS3D_FAST["max"] and out["logit_mean_abs"] < LIMITS3D_FAST["mean"], out
    assert out["loss_abs_err"] < 1e-3, out
    assert out["grad_rel_err_median"] < 0.15 and out["grad_rel_err_worst"] < 0.3, errs


@pytest.mark.parametrize("kw", [{}, {"precise": False}], ids=["default", "fast"])
def test_unet3d_refuses_more_than_64_classes(kw):
    from semantic_segmentation_amd.unet3d import UNet3D
    net = UNet3D(1, 65, **kw).cuda().train()
    x = torch.randn(1, 1, 16, 16, 16, device="cuda")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with pytest.raises(NotImplementedError, match="up to 64"):
            net(x)
    assert not [str(w.message) for w in rec if "16-bit engine" in str(w.message)]


# ------------------------------------------------------------------------------------------------ 2-D
def _unet_3_9():
    from semantic_segmentation_amd.unet import UNet
    sd = oracle.unet_state_dict(3, 9, seed=41)
    net = UNet(3, 9)
    net.load_state_dict(sd, strict=True)
    return net.cuda().train(), sd


def test_evaluate_on_a_nine_class_unet():
    """unet.evaluate.evaluate over a two-batch list loader at 2 x 3 x 48 x 64: a 0-d tensor within 1e-6 of the mean of
    oracle.evaluate_dice on the network's OWN eval-mode logits per batch (the metric alone, not the network's logit error); the
    net is left in train mode"""
    from semantic_segmentation_amd.unet.evaluate import evaluate
    net, _ = _unet_3_9()
    g = torch.Generator().manual_seed(12)
    loader = [{"image": torch.randn(2, 3, 48, 64, generator=g), "mask": torch.randint(0, 9, (2, 1, 48, 64), generator=g)}
              for _ in range(2)]
    with torch.no_grad():
        net(loader[0]["image"].cuda())                        # one train-mode pass moves the running statistics off (0, 1)
    score = evaluate(net, loader, torch.device("cuda:0"))
    assert isinstance(score, torch.Tensor) and score.dim() == 0
    assert net.training
    net.eval()
    with torch.no_grad():
        want = [float(oracle.evaluate_dice(net(b["image"].cuda()).float().cpu(), b["mask"])) for b in loader]
    net.train()
    print("evaluate UNet(3, 9):", float(score), want)
    assert abs(float(score) - float(np.mean(want))) < 1e-6, (float(score), want)


def test_unet_wide_head_backward_is_one_launch():
    """UNet(3, 9) train step at 2 x 3 x 48 x 64: the head's backward calls ops.head1x1_wide_bwd once and ops.conv_smallcout_bwd not at
    all; the head's gradients agree with the oracle within the bounds of test_default_unet_with_wide_ends_meets_1e3"""
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd.losses import seg_loss
    net, sd = _unet_3_9()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 3, 48, 64, generator=g)
    mask = torch.randint(0, 9, (2, 1, 48, 64), generator=g)
    params = {k: v.detach().clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    ref_loss = oracle.seg_loss(oracle.unet_forward(params, x, True, {}), mask)
    keys = ("outc.conv.weight", "outc.conv.bias")
    ref = dict(zip(keys, torch.autograd.grad(ref_loss, [params[k] for k in keys])))
    calls = {"old": 0, "new": 0}
    old, new = ops.conv_smallcout_bwd, ops.head1x1_wide_bwd
    ops.conv_smallcout_bwd = lambda *a, **k: (calls.__setitem__("old", calls["old"] + 1), old(*a, **k))[1]
    ops.head1x1_wide_bwd = lambda *a, **k: (calls.__setitem__("new", calls["new"] + 1), new(*a, **k))[1]
    try:
        loss = seg_loss(net(x.cuda()), mask.cuda())
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.conv_smallcout_bwd, ops.head1x1_wide_bwd = old, new
    assert calls == {"old": 0, "new": 1}, calls
    assert abs(float(loss) - float(ref_loss)) < 2e-5
    got = dict(net.named_parameters())
    rel = {k: float((got[k].grad.cpu().double() - ref[k].double()).norm() / ref[k].double().norm()) for k in keys}
    REPORT["unet_3_9_head_grads"] = rel
    _dump()
    print(rel)
    assert max(rel.values()) < 0.27, rel
