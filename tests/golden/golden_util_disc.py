"""Seeded weights and inputs of the discriminator fixtures tests/golden/pix2pix_disc_{patch,pixel}.npz (made by make_golden_disc.py from
the reference's own classes in double).  Only checksums of the weights are stored: everything here is regenerated from the seeds."""
from typing import Dict

import torch

from golden_util import seeded_discriminator_state_dict

INPUT_STD = 0.5


def seeded_pixel_state_dict(seed, input_nc, ndf, norm, bias_std=0.1) -> Dict[str, torch.Tensor]:
    """the keys of PixelDiscriminator (networks.py:668-697): weights N(0, 1 / sqrt(fan_in)) (logits of order one), biases N(0, bias_std),
    gamma N(1, 0.1), beta N(0, 0.1); BatchNorm running statistics at their initial values.  Under BatchNorm net.2 and net.5 have no
    bias; under InstanceNorm both have one and there is no net.3.*"""
    g = torch.Generator().manual_seed(seed)

    def normal(shape, std, mean=0.0):
        return (torch.randn(shape, generator=g, dtype=torch.float64) * std + mean).float()
    inst = norm == "instance"
    sd = {"net.0.weight": normal((ndf, input_nc, 1, 1), input_nc ** -0.5), "net.0.bias": normal((ndf,), bias_std),
          "net.2.weight": normal((2 * ndf, ndf, 1, 1), ndf ** -0.5)}
    if inst:
        sd["net.2.bias"] = normal((2 * ndf,), bias_std)
    else:
        sd["net.3.weight"], sd["net.3.bias"] = normal((2 * ndf,), 0.1, 1.0), normal((2 * ndf,), 0.1)
        sd["net.3.running_mean"], sd["net.3.running_var"] = torch.zeros(2 * ndf), torch.ones(2 * ndf)
        sd["net.3.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
    sd["net.5.weight"] = normal((1, 2 * ndf, 1, 1), (2 * ndf) ** -0.5)
    if inst:
        sd["net.5.bias"] = normal((1,), bias_std)
    return sd


def perturbed_running(sd, seed):
    """a copy with running statistics that are not the initial 0 / 1 (the eval logits of a fixture)"""
    g = torch.Generator().manual_seed(seed)
    out = dict(sd)
    for k in sd:
        if k.endswith("running_mean"):
            out[k] = torch.randn(sd[k].shape, generator=g) * 0.1
        elif k.endswith("running_var"):
            out[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    return out


# kind patch: NLayerDiscriminator(cin, ndf, n_layers) under BatchNorm; kind pixel: PixelDiscriminator(cin, ndf) under `norm`
FIXTURES = {
    "pix2pix_disc_patch": [dict(tag="d6", kind="patch", cin=6, ndf=64, n_layers=3, norm="batch", N=2, H=32, W=32, seed=51)],
    "pix2pix_disc_pixel": [dict(tag="p2_bn", kind="pixel", cin=2, ndf=64, norm="batch", N=2, H=8, W=8, seed=52),
                           dict(tag="p6_in", kind="pixel", cin=6, ndf=32, norm="instance", N=3, H=5, W=7, seed=53)],
}


def fixture_state_dict(f):
    if f["kind"] == "patch":
        return seeded_discriminator_state_dict(f["seed"], f["cin"], f["ndf"], f["n_layers"], bias_std=0.05)
    return seeded_pixel_state_dict(f["seed"], f["cin"], f["ndf"], f["norm"])


def fixture_input(f):
    return INPUT_STD * torch.randn((f["N"], f["cin"], f["H"], f["W"]), generator=torch.Generator().manual_seed(f["seed"] + 1))


def fixture_dense(shape, f):
    """the fixed dense gradient of the logits: loss = sum(logits * dense)"""
    g = torch.Generator().manual_seed(f["seed"] + 2)
    n = 1
    for s in shape:
        n *= s
    return (torch.rand(tuple(shape), generator=g, dtype=torch.float64) * 2 - 1) / n
