"""Seeded state dicts with the key set of the reference's ResnetGenerator (models_pix2pix/networks.py:321-439): `model.1`, `model.4`,
`model.7` (stem and the two stride-2 convs), `model.{10+i}.conv_block.{1,5}` (`.{1,6}` with dropout), the two transposed convs at
`model.{10+n}` / `model.{13+n}` and the head at `model.{17+n}`.  Under BatchNorm every norm carries weight / bias / running_mean /
running_var / num_batches_tracked and only the head has a bias; under InstanceNorm there are no norm keys and every conv has a bias.
Shared by make_golden_resnet.py (imports the reference) and the tests (never do)."""
from typing import Dict

import torch

from golden_util import _normal


def seeded_resnet_state_dict(seed: int, input_nc=1, output_nc=1, ngf=64, n_blocks=9, norm="instance", use_dropout=False,
                             bias_std=0.1, perturb_running=True) -> Dict[str, torch.Tensor]:
    """conv kernels N(0, 0.02) (the 7x7 and 3x3 kernels of a 256-channel block then give outputs of the order of the input),
    biases N(0, bias_std), BatchNorm gamma N(1, 0.1), beta N(0, 0.1), running statistics away from (0, 1): means N(0, 0.05), variances 0.15 .. 0.45,
    the size of a block conv's output, so that eval mode neither dies out nor overflows 16 bits over eighteen convs"""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    inst = norm == "instance"

    def conv(name, shape, bias):
        sd[name + ".weight"] = _normal(g, shape, 0.02)
        if bias:
            sd[name + ".bias"] = _normal(g, (shape[0],), bias_std)

    def norm_keys(name, c):
        if inst:
            return
        sd[name + ".weight"] = _normal(g, (c,), 0.1, 1.0)
        sd[name + ".bias"] = _normal(g, (c,), 0.1)
        sd[name + ".running_mean"] = _normal(g, (c,), 0.05) if perturb_running else torch.zeros(c)
        sd[name + ".running_var"] = (0.5 + torch.rand((c,), generator=g)) * 0.3 if perturb_running else torch.ones(c)
        sd[name + ".num_batches_tracked"] = torch.tensor(3 if perturb_running else 0, dtype=torch.long)

    conv("model.1", (ngf, input_nc, 7, 7), inst)
    norm_keys("model.2", ngf)
    conv("model.4", (2 * ngf, ngf, 3, 3), inst)
    norm_keys("model.5", 2 * ngf)
    conv("model.7", (4 * ngf, 2 * ngf, 3, 3), inst)
    norm_keys("model.8", 4 * ngf)
    j = 6 if use_dropout else 5
    for b in range(n_blocks):
        p = "model.%d.conv_block" % (10 + b)
        conv(p + ".1", (4 * ngf, 4 * ngf, 3, 3), inst)
        norm_keys(p + ".2", 4 * ngf)
        conv(p + ".%d" % j, (4 * ngf, 4 * ngf, 3, 3), inst)
        norm_keys(p + ".%d" % (j + 1), 4 * ngf)
    i = 10 + n_blocks
    for cin, cout in ((4 * ngf, 2 * ngf), (2 * ngf, ngf)):
        sd["model.%d.weight" % i] = _normal(g, (cin, cout, 3, 3), 0.02)          # ConvTranspose2d: [Cin][Cout][3][3]
        if inst:
            sd["model.%d.bias" % i] = _normal(g, (cout,), bias_std)
        norm_keys("model.%d" % (i + 1), cout)
        i += 3
    conv("model.%d" % (i + 1), (output_nc, ngf, 7, 7), True)
    return sd


INPUT_STD = 0.5


# the two fixtures of make_golden_resnet.py.  A: the default generator (9 blocks, ngf 64, InstanceNorm, dropout modules present with
# p = 0) on 8 x 8 block planes of 256 channels.  B: 6 blocks, ngf 16, three channels, BatchNorm, block planes 5 x 7: odd and not
# square, so reflect, replicate, symmetric and wrap-around padding and a transposed plane all give different numbers.
FIXTURES = {
    "pix2pix_resnet_a": dict(cin=1, cout=1, ngf=64, n_blocks=9, norm="instance", use_dropout=True, N=2, H=32, W=32, seed_g=51, seed_x=53),
    "pix2pix_resnet_b": dict(cin=3, cout=3, ngf=16, n_blocks=6, norm="batch", use_dropout=False, N=3, H=20, W=28, seed_g=61, seed_x=63),
}


def fixture_state_dict(f):
    return seeded_resnet_state_dict(f["seed_g"], f["cin"], f["cout"], f["ngf"], f["n_blocks"], f["norm"], f["use_dropout"])


def fixture_inputs(f):
    """(input [N,cin,H,W], real image [N,cout,H,W], dense gradient [N,cout,H,W]) of a fixture, regenerated from its seed (fp32).
    The loss of the fixture is L1(image, real) * 100 + sum(image * dense) / numel: the L1 term alone has a gradient of one size
    everywhere, the dense one gives every pixel its own."""
    g = torch.Generator().manual_seed(f["seed_x"])
    x = INPUT_STD * torch.randn((f["N"], f["cin"], f["H"], f["W"]), generator=g)
    real = torch.rand((f["N"], f["cout"], f["H"], f["W"]), generator=g) * 2 - 1
    dense = torch.randn((f["N"], f["cout"], f["H"], f["W"]), generator=g)
    return x, real, dense


def fixture_loss(image, real, dense):
    return torch.nn.functional.l1_loss(image, real) * 100.0 + (image * dense).sum() / image.numel()
