"""UNet.predict (`-m gpu`): the label map equals the predicate of unet/evaluate.py:29-40 applied to the same network's logits, byte
for byte, in every numerics mode; where the pair forward runs, the labels come from the head launch itself (gs_head1x1_labels)."""
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu

NETS = [(1, 1), (1, 2), (3, 9)]                              # (image channels, classes): sigmoid, the 8-lanes head, the wide head
SHAPES = [(2, 32, 32), (1, 37, 29)]                          # odd sizes go through Up's padding
MODES = {"default": None, "precise": True, "fast": False}


def _want_labels(logits):
    lg = logits.detach().float().cpu()
    if lg.shape[1] == 1:
        return (torch.sigmoid(lg[:, 0]) > 0.5).to(torch.uint8), lg[:, 0].abs() < 1e-6
    mx = lg.max(1, keepdim=True).values
    idx = torch.arange(lg.shape[1]).view(1, -1, 1, 1).expand_as(lg)
    first = torch.where(lg == mx, idx, torch.full_like(idx, lg.shape[1])).min(1).values       # ties to the lowest index
    return first.to(torch.uint8), torch.zeros(first.shape, dtype=torch.bool)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cin,ncls", NETS)
def test_unet_predict_equals_the_predicate_on_the_logits(cin, ncls, shape, mode):
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd.unet import UNet
    N, H, W = shape
    net = UNet(cin, ncls, precise=MODES[mode])
    net.load_state_dict(oracle.unet_state_dict(cin, ncls, seed=5 + ncls), strict=True)
    net = net.cuda()
    x = torch.randn(N, cin, H, W, generator=torch.Generator().manual_seed(ncls)).cuda()
    calls = []
    saved = ops.head1x1_labels, ops.labels_from_logits
    ops.head1x1_labels = lambda *a, **k: (calls.append(("head", "scale" if (len(a) > 5 or k.get("scale") is not None) else "plain")),
                                          saved[0](*a, **k))[1]
    ops.labels_from_logits = lambda *a, **k: (calls.append(("logits", "")), saved[1](*a, **k))[1]
    try:
        for train in (False, True):                          # eval (default mode: BatchNorm folded); train: batch statistics
            net.train(train)
            state = {k: v.clone() for k, v in net.state_dict().items()}
            with torch.no_grad():
                # the freshly initialised head may prefer one class everywhere: centre every class's logits on 0 through the head's bias
                state["outc.conv.bias"] -= net(x).transpose(0, 1).flatten(1).median(1).values
                net.load_state_dict(state, strict=True)
                logits = net(x)
            net.load_state_dict(state, strict=True)          # the same running statistics for both calls
            del calls[:]
            lab = net.predict(x)
            torch.cuda.synchronize()
            assert lab.dtype == torch.uint8 and tuple(lab.shape) == (N, H, W) and lab.is_cuda and not lab.requires_grad
            want, free = _want_labels(logits)
            bad = (lab.cpu() != want) & ~free
            assert int(bad.sum()) == 0, (mode, train, int(bad.sum()), bad.nonzero()[:5].tolist())
            assert len(want.unique()) > 1, "a constant label map proves nothing"
            if mode == "fast":
                assert calls == [("logits", "")], calls
            else:
                assert [c[0] for c in calls] == ["head"], calls      # predict called gs_head1x1_labels, once, and nothing else
            if mode == "default":
                # train mode, up to four classes: the last stage's conv pair with BatchNorm + ReLU on the head's load path;
                # eval (folded) and the wide head: the dense z pair
                assert calls[0][1] == ("scale" if (train and ncls <= 4) else "plain"), calls
    finally:
        ops.head1x1_labels, ops.labels_from_logits = saved
    with pytest.raises(RuntimeError):
        net.predict(x.cpu())
