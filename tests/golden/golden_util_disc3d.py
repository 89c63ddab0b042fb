"""Seeded weights and inputs of the 3-D discriminator fixture tests/golden/pix2pix3d_disc.npz (made by make_golden_disc3d.py from the
reference's own GenSeg-3D classes in double).  Only checksums of the weights are stored: everything here is regenerated from the seeds."""
from typing import Dict

import torch

INPUT_STD = 0.5


def _normal(g, shape, std, mean=0.0):
    return (torch.randn(shape, generator=g, dtype=torch.float64) * std + mean).float()


def _norm_keys(sd, g, name, c, bias_std):
    sd[name + ".weight"], sd[name + ".bias"] = _normal(g, (c,), 0.1, 1.0), _normal(g, (c,), bias_std)
    sd[name + ".running_mean"], sd[name + ".running_var"] = torch.zeros(c), torch.ones(c)
    sd[name + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.long)


def seeded_patchgan3d_state_dict(seed, input_nc, ndf, n_layers, norm, bias_std=0.05) -> Dict[str, torch.Tensor]:
    """the keys of the 3-D NLayerDiscriminator (GenSeg-3D/models/networks.py:806-855): Conv3d weights [co, ci, 4, 4, 4] ~ N(0, 1 /
    sqrt(fan_in)) (activations and logits of order one), biases N(0, bias_std), gamma N(1, 0.1), beta N(0, bias_std), BatchNorm3d running
    statistics at their initial values.  Convs at 0, 2, 5, ..., 3 n_layers - 1 (the last of them with stride 1) and the head at
    3 n_layers + 2; a middle conv has a bias only under InstanceNorm3d, where there are no norm keys."""
    g = torch.Generator().manual_seed(seed)
    inst = norm == "instance"
    sd: Dict[str, torch.Tensor] = {}
    sd["model.0.weight"] = _normal(g, (ndf, input_nc, 4, 4, 4), (64 * input_nc) ** -0.5)
    sd["model.0.bias"] = _normal(g, (ndf,), bias_std)
    mult = [min(2 ** n, 8) for n in range(n_layers + 1)]
    for n in range(1, n_layers + 1):
        conv_i, ci, co = 3 * n - 1, ndf * mult[n - 1], ndf * mult[n]
        sd[f"model.{conv_i}.weight"] = _normal(g, (co, ci, 4, 4, 4), (64 * ci) ** -0.5)
        if inst:
            sd[f"model.{conv_i}.bias"] = _normal(g, (co,), bias_std)
        else:
            _norm_keys(sd, g, f"model.{conv_i + 1}", co, bias_std)
    last, cl = 3 * n_layers + 2, ndf * mult[n_layers]
    sd[f"model.{last}.weight"] = _normal(g, (1, cl, 4, 4, 4), (64 * cl) ** -0.5)
    sd[f"model.{last}.bias"] = _normal(g, (1,), bias_std)
    return sd


def seeded_pixel3d_state_dict(seed, input_nc, ndf, norm, bias_std=0.1) -> Dict[str, torch.Tensor]:
    """the keys of the 3-D PixelDiscriminator (GenSeg-3D/models/networks.py:858-886): Conv3d k 1 at net.0 / 2 / 5, the norm at net.3.
    Under BatchNorm3d net.2 and net.5 have no bias; under InstanceNorm3d both have one and there is no net.3.*"""
    g = torch.Generator().manual_seed(seed)
    inst = norm == "instance"
    sd = {"net.0.weight": _normal(g, (ndf, input_nc, 1, 1, 1), input_nc ** -0.5), "net.0.bias": _normal(g, (ndf,), bias_std),
          "net.2.weight": _normal(g, (2 * ndf, ndf, 1, 1, 1), ndf ** -0.5)}
    if inst:
        sd["net.2.bias"] = _normal(g, (2 * ndf,), bias_std)
    else:
        _norm_keys(sd, g, "net.3", 2 * ndf, bias_std)
    sd["net.5.weight"] = _normal(g, (1, 2 * ndf, 1, 1, 1), (2 * ndf) ** -0.5)
    if inst:
        sd["net.5.bias"] = _normal(g, (1,), bias_std)
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


# kind patch: NLayerDiscriminator(cin, ndf, n_layers); kind pixel: PixelDiscriminator(cin, ndf); both under the 3-D `norm`
FIXTURES = {
    "pix2pix3d_disc": [dict(tag="d2_bn", kind="patch", cin=2, ndf=64, n_layers=3, norm="batch", N=2, D=24, H=32, W=40, seed=61),
                       dict(tag="d2_in", kind="patch", cin=2, ndf=16, n_layers=2, norm="instance", N=1, D=12, H=16, W=20, seed=62),
                       dict(tag="p2_bn", kind="pixel", cin=2, ndf=64, norm="batch", N=2, D=3, H=4, W=5, seed=63)],
}


def state_dict_of(kind, seed, cin, ndf, n_layers, norm):
    if kind == "patch":
        return seeded_patchgan3d_state_dict(seed, cin, ndf, n_layers, norm)
    return seeded_pixel3d_state_dict(seed, cin, ndf, norm)


def fixture_state_dict(f):
    return state_dict_of(f["kind"], f["seed"], f["cin"], f["ndf"], f.get("n_layers"), f["norm"])


def fixture_input(f):
    """fp32 values (stored as fp32 in the fixture: a 2 x 2 x 24 x 32 x 40 volume in double would be a megabyte)"""
    return INPUT_STD * torch.randn((f["N"], f["cin"], f["D"], f["H"], f["W"]), generator=torch.Generator().manual_seed(f["seed"] + 1))


def fixture_dense(shape, f):
    """the fixed dense gradient of the logits: loss = sum(logits * dense)"""
    g = torch.Generator().manual_seed(f["seed"] + 2)
    n = 1
    for s in shape:
        n *= s
    return (torch.rand(tuple(shape), generator=g, dtype=torch.float64) * 2 - 1) / n
