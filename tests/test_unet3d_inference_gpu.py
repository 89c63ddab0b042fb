"""UNet3D inference (`-m gpu`): the folded-BatchNorm eval forward of the pair engine against the fp32 oracle and against the two-pass
form, the weight-pack cache, and UNet3D.predict (labels from the head, no logits tensor) against the predicate on the same network's
logits, byte for byte."""
import json
import os

import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu
REPORT = {}

# (in_channels, classes, level_channels, NB, (D, H, W)).  Two samples and three unequal dimensions: a depth / batch mix-up in the flattened
# [NB*D] grid or in the pooling cannot cancel; 9 classes: the wide head; [128, 128, 256]: 64-multiples other than the default widths
CONFIGS = {"c2_nb2": (1, 2, None, 2, (16, 16, 24)), "c9_in2": (2, 9, None, 1, (16, 16, 16)),
           "wide_levels": (1, 2, [128, 128, 256], 1, (16, 16, 16))}
EV = 1e-5            # the project's bound on the eval forward: test_unet3d_gpu.LIMITS["default"]["ev"], times max(1, |ref|.max())
# |folded - two-pass| / max(1, |ref|.max()), asserted at 1.5 x the value measured on the first run on the MI355X.
# Measured: c2_nb2 2.92e-6, c9_in2 2.90e-6, wide_levels 2.59e-6 -- the size of either form's own distance from the oracle (2.4e-6 ..
# 3.5e-6): two roundings of the same fp32 values, below the 1e-5 the forward itself is held to.
FOLD_VS_TWO_PASS = {"c2_nb2": 4.4e-6, "c9_in2": 4.4e-6, "wide_levels": 3.9e-6}


def _report_dir():
    """the directory tests/test_unet3d_gpu.py writes its parity report to: asked of that module's _dump (its open() is intercepted,
    nothing of its report is written), so that this file's report lands beside it"""
    from unittest import mock
    from tests import test_unet3d_gpu as base
    with mock.patch("builtins.open", mock.mock_open()) as opened:
        base._dump()
    return os.path.dirname(opened.call_args[0][0])


def _dump():
    with open(os.path.join(_report_dir(), "parity_unet3d_inference.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def _build(cfg, precise=None, seed=71):
    from semantic_segmentation_amd.unet3d import UNet3D
    cin, ncls, levels, NB, dims = CONFIGS[cfg] if isinstance(cfg, str) else cfg
    kw = {} if levels is None else dict(level_channels=levels)
    sd = oracle.unet3d_state_dict(cin, ncls, seed=seed, **kw)
    net = UNet3D(cin, ncls, precise=precise, **kw)
    net.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(NB, cin, *dims, generator=g)
    mask = torch.randint(0, max(ncls, 2), (NB, *dims), generator=g)
    return net.cuda(), x.cuda(), (mask.float() if ncls == 1 else mask).cuda()


def _train_step(net, x, mask, lr=0.05):
    """one SGD step in train mode: the running statistics leave their initial values, every parameter's version is bumped"""
    from semantic_segmentation_amd.losses import seg_loss
    net.train()
    net.zero_grad(set_to_none=True)
    logits = net(x)
    n, c, d, h, w = logits.shape
    seg_loss(logits.reshape(n, c, d * h, w), mask.reshape(n, d * h, w)).backward()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(p.grad, alpha=-lr)
    net.eval()


def _oracle_eval(net, x):
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    with torch.no_grad():
        return oracle.unet3d_forward(sd, x.cpu(), train=False)


def _eval(net, x, fold=True):
    from semantic_segmentation_amd.unet import unet_engine
    keep = unet_engine.FOLD_BN_INFERENCE
    unet_engine.FOLD_BN_INFERENCE = fold
    try:
        with torch.no_grad():
            out = net(x)
        torch.cuda.synchronize()
        return out
    finally:
        unet_engine.FOLD_BN_INFERENCE = keep


def _folded_packs(net):
    return {k: v for k, v in net.engine._packs.items() if k.endswith("|fsegs")}


class _PackCounter:
    """counts the pack launches of semantic_segmentation_amd.ops while active"""
    NAMES = ("pack_weight", "pack_weight_multi", "pack_weight_segs", "pack_weight_q8", "pack_weight_split")

    def __enter__(self):
        from semantic_segmentation_amd import ops
        self.ops, self.calls, self.saved = ops, [], {n: getattr(ops, n) for n in self.NAMES}
        for n, fn in self.saved.items():
            setattr(ops, n, (lambda n_, fn_: lambda *a, **k: (self.calls.append(n_), fn_(*a, **k))[1])(n, fn))
        return self

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(self.ops, n, fn)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_folded_eval_forward_vs_oracle_and_two_pass(cfg):
    net, x, mask = _build(cfg)
    assert net.engine.plan is not None
    _train_step(net, x, mask)
    assert float(net.a_block2.bn1.running_mean.abs().max()) > 0            # not the initial statistics
    ref = _oracle_eval(net, x)
    scale = max(1.0, float(ref.abs().max()))
    folded = _eval(net, x, fold=True)
    packs = _folded_packs(net)
    # the engine holds a folded pack for every conv stage but the first, and no plain segment pack was built for this forward
    assert set(packs) == {s + "|fsegs" for s in net.engine._pair_layout(x.shape[-1])[0]} and len(packs) == 13
    two_pass = _eval(net, x, fold=False)
    assert tuple(folded.shape) == tuple(ref.shape) and folded.dtype == torch.float32
    e_f = float((folded.cpu() - ref).abs().max()) / scale
    e_t = float((two_pass.cpu() - ref).abs().max()) / scale
    e_ft = float((folded - two_pass).abs().max()) / scale
    REPORT[cfg] = {"folded_vs_oracle": e_f, "two_pass_vs_oracle": e_t, "folded_vs_two_pass": e_ft, "logit_scale": scale}
    _dump()
    print(f"{cfg}: folded vs oracle {e_f:.3e}, two-pass vs oracle {e_t:.3e}, folded vs two-pass {e_ft:.3e} (of the logit scale {scale:.3f})")
    assert e_f < EV, REPORT[cfg]
    assert e_ft < FOLD_VS_TWO_PASS[cfg], REPORT[cfg]
    # the packs follow the statistics: one more training step, and the next eval forward meets the oracle on the NEW state
    _train_step(net, x, mask)
    ref2 = _oracle_eval(net, x)
    assert float((ref2 - ref).abs().max()) > 100 * EV * scale               # the state did change
    folded2 = _eval(net, x, fold=True)
    e_f2 = float((folded2.cpu() - ref2).abs().max()) / max(1.0, float(ref2.abs().max()))
    REPORT[cfg]["folded_vs_oracle_after_second_step"] = e_f2
    _dump()
    assert e_f2 < EV, REPORT[cfg]
    assert all(v[0] != packs[k][0] for k, v in _folded_packs(net).items()), "a folded pack kept its key across a training step"


def test_pack_cache_reuse_and_invalidation():
    net, x, mask = _build("c9_in2", seed=83)
    _train_step(net, x, mask)
    eng = net.engine
    with _PackCounter() as first:
        a = _eval(net, x)
    assert first.calls, "the first eval forward packs"
    held = {k: tuple(t.data_ptr() for t in v[1:] if torch.is_tensor(t)) for k, v in eng._packs.items()}
    assert any(k.endswith("|fsegs") for k in held) and any(k.endswith("|up") for k in held)
    with _PackCounter() as second:
        b = _eval(net, x)
    assert second.calls == [], second.calls                                # the second builds no pack
    assert {k: tuple(t.data_ptr() for t in v[1:] if torch.is_tensor(t)) for k, v in eng._packs.items()} == held
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))           # bit-identical logits
    # an in-place update bumps the version: the next forward folds the new weight
    with torch.no_grad():
        net.s_block2.conv1.weight.mul_(1.5)
    with _PackCounter() as third:
        c = _eval(net, x)
    assert third.calls == ["pack_weight_segs"], third.calls                # the one stale pack, one launch
    ref = _oracle_eval(net, x)
    assert float((ref - a.cpu()).abs().max()) > 10 * EV * max(1.0, float(ref.abs().max()))       # the change is far above the bound
    assert float((c.cpu() - ref).abs().max()) < EV * max(1.0, float(ref.abs().max()))
    # a forward that keeps a graph reuses nothing under the default policy: everything is packed again, and nothing of the
    # inference packs survives it
    from semantic_segmentation_amd import engine_common
    assert engine_common.PACK_CACHE and not engine_common.PACK_CACHE_TRAINING
    net.train()
    with _PackCounter() as train:
        out = net(x)
    torch.cuda.synchronize()
    assert out.requires_grad
    assert train.calls == ["pack_weight_segs", "pack_weight_multi", "pack_weight", "pack_weight", "pack_weight"], train.calls
    assert not any(k.endswith("|fsegs") for k in eng._packs)
    assert all(tuple(t.data_ptr() for t in v[1:] if torch.is_tensor(t)) != held.get(k) for k, v in eng._packs.items())


def _want_labels(logits):
    """the predicate on logits [NB, C, D, H, W], on the CPU: arg-max with ties to the lowest index; one class: sigmoid > 0.5"""
    lg = logits.detach().float().cpu()
    if lg.shape[1] == 1:
        return (torch.sigmoid(lg[:, 0]) > 0.5).to(torch.uint8), lg[:, 0].abs() < 1e-6
    mx = lg.max(1, keepdim=True).values
    idx = torch.arange(lg.shape[1]).view(1, -1, 1, 1, 1).expand_as(lg)
    first = torch.where(lg == mx, idx, torch.full_like(idx, lg.shape[1])).min(1).values
    return first.to(torch.uint8), torch.zeros(first.shape, dtype=torch.bool)


PREDICT_CONFIGS = dict(CONFIGS, c1=(1, 1, None, 1, (16, 16, 16)))


@pytest.mark.parametrize("precise", [None, False], ids=["default", "fast"])
@pytest.mark.parametrize("cfg", list(PREDICT_CONFIGS))
def test_predict_equals_the_predicate_on_the_logits(cfg, precise):
    from semantic_segmentation_amd import ops
    net, x, mask = _build(PREDICT_CONFIGS[cfg], precise=precise, seed=97)
    _train_step(net, x, mask)
    NB, _, D, H, W = x.shape
    calls = []
    saved = ops.head1x1_labels, ops.labels_from_logits
    ops.head1x1_labels = lambda *a, **k: (calls.append("head"), saved[0](*a, **k))[1]
    ops.labels_from_logits = lambda *a, **k: (calls.append("logits"), saved[1](*a, **k))[1]
    try:
        for mode in ("eval", "train"):
            net.train(mode == "train")
            state = {k: v.clone() for k, v in net.state_dict().items()}
            with torch.no_grad():
                # the freshly initialised head prefers one class everywhere: centre every class's logits on 0 through the head's bias
                state["s_block1.conv3.bias"] -= net(x).transpose(0, 1).flatten(1).median(1).values
                net.load_state_dict(state, strict=True)
                logits = net(x)
            net.load_state_dict(state, strict=True)                        # train mode: the same running statistics for both calls
            del calls[:]
            lab = net.predict(x)
            torch.cuda.synchronize()
            assert calls == (["head"] if precise is None else ["logits"]), calls
            assert lab.dtype == torch.uint8 and tuple(lab.shape) == (NB, D, H, W) and lab.is_cuda and not lab.requires_grad
            want, free = _want_labels(logits)
            bad = (lab.cpu() != want) & ~free
            assert int(bad.sum()) == 0, (cfg, mode, int(bad.sum()), bad.nonzero()[:5].tolist())
            assert len(want.unique()) > 1, "a constant label map proves nothing"
            if mode == "train":                                            # predict follows self.training, as forward does
                assert not torch.equal(net.a_block2.bn1.running_mean, state["a_block2.bn1.running_mean"])
    finally:
        ops.head1x1_labels, ops.labels_from_logits = saved
    with pytest.raises(RuntimeError):
        net.predict(x.cpu())
