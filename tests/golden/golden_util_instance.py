"""Seeded state dicts with the key set of the reference's Pix2Pix networks under get_norm_layer('instance')
(models_pix2pix/networks.py:23-38): InstanceNorm2d without parameters or buffers, so no norm keys at all, and `use_bias` True
(:553-617, :620-665): a bias on every down conv, every Cell_upconv primitive and the PatchGAN's middle convs.
Shared by make_golden_instance.py (imports the reference) and the tests (never do)."""
from typing import Dict

import torch

from golden_util import _normal


def seeded_generator_state_dict_instance(seed: int, input_nc=1, output_nc=1, num_downs=8, ngf=64, bias_std=0.1) -> Dict[str, torch.Tensor]:
    """UnetGenerator(input_nc, output_nc, num_downs, ngf, InstanceNorm): conv kernels N(0, 0.02), biases N(0, bias_std)"""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}

    def conv(name, cout, cin):
        sd[name + ".weight"] = _normal(g, (cout, cin, 4, 4), 0.02)
        sd[name + ".bias"] = _normal(g, (cout,), bias_std)

    def cell(name, cin, cout):
        for j, k in enumerate((4, 6, 8)):
            sd[f"{name}._ops._ops.{j}.op.weight"] = _normal(g, (cin, cout, k, k), 0.02)
            sd[f"{name}._ops._ops.{j}.op.bias"] = _normal(g, (cout,), bias_std)

    chans = [(output_nc, ngf), (ngf, ngf * 2), (ngf * 2, ngf * 4), (ngf * 4, ngf * 8)]
    chans += [(ngf * 8, ngf * 8)] * (num_downs - 4)
    prefix = "model"
    for depth, (outer, inner) in enumerate(chans):
        p = prefix + ".model"
        outermost, innermost = depth == 0, depth == num_downs - 1
        if outermost:
            conv(p + ".0", inner, input_nc)
            cell(p + ".3", inner * 2, outer)
            prefix = p + ".1"
        elif innermost:
            conv(p + ".1", inner, outer)
            cell(p + ".3", inner, outer)
        else:
            conv(p + ".1", inner, outer)
            cell(p + ".5", inner * 2, outer)
            prefix = p + ".3"
    return sd


def seeded_discriminator_state_dict_instance(seed: int, input_nc=2, ndf=64, n_layers=3, bias_std=0.1) -> Dict[str, torch.Tensor]:
    """NLayerDiscriminator(input_nc, ndf, n_layers, InstanceNorm): convs at 0, 2, 5, ... 3 * n_layers - 1 and 3 * n_layers + 2"""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    mult = [min(2 ** n, 8) for n in range(n_layers + 1)]
    shapes = [(0, ndf, input_nc)] + [(3 * n - 1, ndf * mult[n], ndf * mult[n - 1]) for n in range(1, n_layers + 1)]
    shapes.append((3 * n_layers + 2, 1, ndf * mult[n_layers]))
    for i, co, ci in shapes:
        sd[f"model.{i}.weight"] = _normal(g, (co, ci, 4, 4), 0.02)
        sd[f"model.{i}.bias"] = _normal(g, (co,), bias_std)
    return sd


INPUT_STD = 0.2


# the two fixtures of make_golden_instance.py: networks, input and seeds
FIXTURES = {
    "pix2pix_instance_a": dict(cin=1, cout=1, D=6, n_layers=3, N=2, H=64, W=64, seed_g=31, seed_d=32, seed_x=33),
    "pix2pix_instance_b": dict(cin=3, cout=3, D=5, n_layers=2, N=3, H=32, W=64, seed_g=41, seed_d=42, seed_x=43),
}


def fixture_inputs(f):
    """(input [N,cin,H,W], real image [N,cout,H,W], arch [D,3]) of a fixture, regenerated from its seed (fp32 values).
    The input has standard deviation INPUT_STD: the planes of the first normed conv then have a variance of a few eps, so that the
    eps of the norm is visible in the image and the logits above their 16-bit error (a dropped eps is one of the stated mutants)."""
    g = torch.Generator().manual_seed(f["seed_x"])
    x = INPUT_STD * torch.randn((f["N"], f["cin"], f["H"], f["W"]), generator=g)
    real = torch.rand((f["N"], f["cout"], f["H"], f["W"]), generator=g) * 2 - 1
    arch = 0.5 * torch.randn((f["D"], 3), generator=g)
    return x, real, arch
