"""networks.PixelDiscriminator (reference models_pix2pix/networks.py:668-697) in fp64 on the CPU, as the plain state that the
discriminator replays of tests/pix2pix_backward_replay.py (BatchNorm) and tests/instnorm_reference.py (InstanceNorm) take: the
network is the PatchGAN's plan with 1 x 1 kernels -- first conv + bias + LeakyReLU, one normed conv + LeakyReLU, head -- so its
hand-derived backward IS replay_discriminator with k = 1, stride 1, pad 0 and the names net.0 / net.2 / net.3 / net.5.

  Under BatchNorm net.2 and net.5 carry no bias (the reference passes bias=use_bias to the last conv as well); under InstanceNorm
  all three do, and net.2's cancels in the norm: the engine does not add it and returns exact zeros for its gradient.

forward_state(..., mutant=) states the wrong forwards the tests must tell from the right one: batch statistics where instance
statistics are due and the reverse, the unbiased variance, the head's bias present under BatchNorm."""
import torch
import torch.nn.functional as F

from golden_util_disc import seeded_pixel_state_dict  # noqa: F401
from tests import instnorm_reference as ir
from tests import pix2pix_backward_replay as pr

MUTANTS = ("swapped_stats", "unbiased_var", "head_bias_under_bn")


def torch_module(input_nc, ndf, norm):
    """the module tree in plain torch (double), for torch.autograd and load_state_dict(strict=True)"""
    inst = norm == "instance"
    nl = torch.nn.InstanceNorm2d(2 * ndf, affine=False, track_running_stats=False) if inst else torch.nn.BatchNorm2d(2 * ndf)

    class Pixel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.net = torch.nn.Sequential(torch.nn.Conv2d(input_nc, ndf, 1), torch.nn.LeakyReLU(0.2, True),
                                           torch.nn.Conv2d(ndf, 2 * ndf, 1, bias=inst), nl, torch.nn.LeakyReLU(0.2, True),
                                           torch.nn.Conv2d(2 * ndf, 1, 1, bias=inst))

        def forward(self, x):
            return self.net(x)
    return Pixel().double()


def forward_state(sd, x, norm, train=True, store=None, mutant=None):
    """(plain state, logits).  store=dt rounds what the engine keeps in 16 bits (z, y, the packed weight, the activations)."""
    assert mutant is None or mutant in MUTANTS
    inst = norm == "instance"
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x = x.double()
    r16, r32 = pr._rounders(store)
    N, _, H, W = x.shape
    w, b = sd["net.0.weight"], sd["net.0.bias"]
    z = r16(F.leaky_relu(F.conv2d(x, w, b), 0.2))
    recs = [dict(kind="first", name="net.0", k=1, s=1, p=0, w=w, b=b, x=x, z=z)]
    w = sd["net.2.weight"]
    if inst:
        b = sd["net.2.bias"]
        yfull = F.conv2d(z, r16(w), b if store is None else None)
        if H * W < 2:
            raise ValueError(f"Expected more than 1 spatial element when training, got input size {list(yfull.shape)}")
        rec = dict(kind="mid", name="net.2", k=1, s=1, p=0, w=w, b=b, inp=z, y=r16(yfull), wd=r16(w))
        if mutant == "swapped_stats":
            rec["mean"], rec["invstd"] = ir._stats(rec["y"], r32, "batch_stats")
        else:
            rec["mean"], rec["invstd"] = ir._stats(rec["y"], r32, mutant if mutant == "unbiased_var" else None)
        cur = r16(ir.in_act_apply64(rec["y"], rec["mean"], rec["invstd"], "leaky"))
    else:
        yfull = F.conv2d(z, r16(w), None)
        rec = dict(kind="mid", name="net.2", k=1, s=1, p=0, w=w, b=None, inp=z, y=r16(yfull), train_stats=bool(train), wd=r16(w),
                   bnname="net.3")
        if mutant in ("swapped_stats", "unbiased_var") and train:
            g, be = sd["net.3.weight"], sd["net.3.bias"]
            if mutant == "swapped_stats":                              # instance statistics where batch statistics are due
                mean, var = yfull.mean((2, 3), keepdim=True), yfull.var((2, 3), unbiased=False, keepdim=True)
            else:
                mean, var = yfull.mean((0, 2, 3), keepdim=True), yfull.var((0, 2, 3), unbiased=True, keepdim=True)
            v = (rec["y"] - mean) * torch.rsqrt(var + pr.BN_EPS) * g.view(1, -1, 1, 1) + be.view(1, -1, 1, 1)
            rec.update(scale=None, shift=None, mean=None, invstd=None)
            cur = r16(F.leaky_relu(v, 0.2))
        else:
            rec.update(pr._bn_coef(sd, "net.3", yfull, train, r32))
            cur = r16(F.leaky_relu(rec["y"] * pr._col(rec["scale"]) + pr._col(rec["shift"]), 0.2))
    recs.append(rec)
    w = sd["net.5.weight"]
    b = sd.get("net.5.bias")
    recs.append(dict(kind="last", name="net.5", k=1, s=1, p=0, w=w, b=b, inp=cur))
    logits = F.conv2d(cur, w, b)
    if mutant == "head_bias_under_bn" and not inst:
        logits = logits + 0.1
    return dict(kind="pix2pix_d_in" if inst else "pix2pix_d", N=N, H=H, W=W, recs=recs), logits


def replays(state, dl, need_dx, store):
    return (ir if state["kind"] == "pix2pix_d_in" else pr).replays(state, dl, need_dx, store)
