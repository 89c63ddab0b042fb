"""UNet3DEngine.backward held to the fp64 replay of the state its own forward saved (tests/backward_replay.py), as
test_unet_backward_replay_gpu.py does for the 2-D engine.  One allowance: the bias of a conv in front of a batch-statistics
BatchNorm3d has gradient zero up to noise, the engine returns exact zeros, and it is held in absolute terms (compare3d)."""
import warnings

import pytest
import torch

from oracle import oracle
from tests import backward_replay as br

pytestmark = pytest.mark.gpu

DEFAULT = ([64, 128, 256], 512)


# one seed per case, fixed here (as in test_unet_backward_replay_gpu.py)
SEEDS = {"default_f16": 11, "dense16_f16": 11, "default_bf16": 11, "c2k9_16": 12, "narrow_16": 11, "eval_f16": 12,
         "seg_loss_f16": 11}


def C(cid, seed, cin=1, ncls=2, widths=DEFAULT, NB=2, D=8, H=16, W=16, dtype="f16", precise=None, train=True, pair=True,
      real_loss=False):
    return pytest.param(dict(id=cid, seed=SEEDS.get(cid, seed), cin=cin, ncls=ncls, widths=widths, NB=NB, D=D, H=H, W=W, dtype=dtype, precise=precise,
                             train=train, pair=pair, real_loss=real_loss), id=cid)


CASES = [
    C("default_f16", 11), C("dense16_f16", 11, precise=False, pair=False), C("default_bf16", 11, dtype="bf16"),
    C("c2k9_16", 11, cin=2, ncls=9, NB=1, D=16),                      # wide input (padded to 8 channels), 5..64-class head
    C("narrow_16", 11, widths=([32, 128, 256], 512), NB=1, D=16, pair=False),     # no pair layout: "auto" runs the 16-bit engine
    C("eval_f16", 11, NB=1, train=False),
    C("seg_loss_f16", 11, real_loss=True),                            # dlogits of the real loss over the volume
]


def forward_case(c):
    from semantic_segmentation_amd.unet3d import UNet3D
    dev = torch.device("cuda:0")
    sd = oracle.unet3d_state_dict(c["cin"], c["ncls"], seed=c["seed"], level_channels=tuple(c["widths"][0]),
                                  bottleneck_channel=c["widths"][1])
    net = UNet3D(c["cin"], c["ncls"], level_channels=list(c["widths"][0]), bottleneck_channel=c["widths"][1],
                 compute_dtype=c["dtype"], precise=c["precise"])
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    net.train(c["train"])
    g = torch.Generator().manual_seed(c["seed"])
    x = torch.randn((c["NB"], c["cin"], c["D"], c["H"], c["W"]), generator=g).to(dev)
    n = c["NB"] * c["D"] * c["H"] * c["W"]
    dl = ((torch.rand((c["NB"], c["ncls"], c["D"], c["H"], c["W"]), generator=g, dtype=torch.float64) * 2 - 1) / n).float().to(dev)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)               # the narrow widths: "auto" names its fall-back
        logits, ctx = net.engine.forward(x, c["train"], True)
    if c.get("real_loss"):
        from semantic_segmentation_amd.losses import seg_loss
        mask = (torch.rand((c["NB"], c["D"], c["H"], c["W"]), generator=g) > 0.5).long().to(dev)
        lg = logits.detach().clone().requires_grad_(True)
        seg_loss(lg.reshape(c["NB"], c["ncls"], c["D"] * c["H"], c["W"]), mask.reshape(c["NB"], c["D"] * c["H"], c["W"])).backward()
        dl = lg.grad.detach()
    return net, sd, ctx, dl


@pytest.mark.parametrize("c", CASES)
def test_backward3d_is_the_replay(c):
    net, sd, ctx, dl = forward_case(c)
    eng = net.engine
    with torch.no_grad():
        grads = eng.backward(ctx, dl)
    torch.cuda.synchronize()

    # ---- the branch this case is for
    assert bool(ctx.get("pair")) == c["pair"]
    assert all(s.stats == c["train"] for s in ctx["stages"])
    assert any(s.wide for s in ctx["stages"]) == (c["cin"] > 1)
    assert len(ctx["stages"]) == 14 and ctx["ncls"] == c["ncls"]

    state = br.state_from_unet3d_ctx(eng, ctx)
    got = {k: v.detach().cpu() for k, v in grads.items()}
    r64, r16, d_u, n_und, bias_scale = br.replays3d(state, br.d64(dl), eng.tdt)
    assert set(got) == set(r64), set(got) ^ set(r64)
    assert (len(bias_scale) == 14) == c["train"]
    if c["train"]:
        assert all(not got[k].any() for k in bias_scale)             # exact zeros in front of batch statistics
    else:
        assert all(got[name + ".bias"].any() for name in state["stages"])       # real column sums
    rep, bad = br.compare3d(got, r64, r16, d_u, bias_scale, eng.tdt)
    br.record("unet3d/" + c["id"], rep, n_und)
    net.load_state_dict(sd, strict=True)
    for k in r64:
        if k not in bias_scale:
            assert d_u[k] <= max(rep[k]["e16"], br.FLOOR32), f"{k}: d_U {d_u[k]:.3g} above e16 {rep[k]['e16']:.3g}: this case needs another seed"
    assert not bad, {k: rep[k] for k in bad}
