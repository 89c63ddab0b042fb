"""Seeded weights and inputs of the 3-D generator fixture tests/golden/pix2pix3d_gen.npz (made by make_golden_gen3d.py from the
reference's own GenSeg-3D classes in double), and the key layout of the reference's UnetGenerator(upsampling='linear') state dict.
Only checksums of the weights are stored: everything here is regenerated from the seeds."""
from typing import Dict, List, Tuple

import torch

KS = (4, 6, 8)
BN_LEAVES = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")

# UnetGenerator(input_nc, output_nc, num_downs, ngf, norm, use_dropout) on N volumes of D x H x W; mode train / eval
FIXTURES = {
    "pix2pix3d_gen": [
        dict(tag="bn5_train", input_nc=1, output_nc=1, num_downs=5, ngf=16, norm="batch", use_dropout=False, train=True,
             N=2, D=32, H=32, W=32, seed=91, stride=2),
        dict(tag="bn5_eval", input_nc=1, output_nc=1, num_downs=5, ngf=16, norm="batch", use_dropout=False, train=False,
             N=2, D=32, H=32, W=32, seed=91, stride=2),
        dict(tag="in5_rgb", input_nc=2, output_nc=3, num_downs=5, ngf=16, norm="instance", use_dropout=False, train=True,
             N=1, D=32, H=64, W=32, seed=92, stride=2),
        dict(tag="bn6_drop_eval", input_nc=1, output_nc=1, num_downs=6, ngf=16, norm="batch", use_dropout=True, train=False,
             N=1, D=64, H=64, W=64, seed=93, stride=4),
    ],
}


def channels(f) -> List[int]:
    """c[k]: channels after k cells"""
    ngf = f["ngf"]
    return [f["input_nc"], ngf, 2 * ngf, 4 * ngf] + [8 * ngf] * (f["num_downs"] - 3)


def block_prefix(d: int) -> str:
    """state-dict prefix of the Sequential of the block at depth d (0 = outermost)"""
    return "model.model." + ("1.model." if d >= 1 else "") + "3.model." * max(d - 1, 0)


def block_layout(f, d: int) -> dict:
    """indices in the block's Sequential: cell, downnorm, upconv, upnorm, dropout (None: absent); and the up-conv's channels"""
    nd, c = f["num_downs"], channels(f)
    outer = f["output_nc"] if d == 0 else c[d]
    if d == 0:
        return dict(cell=0, downnorm=None, upconv=4, upnorm=None, drop=None, up_in=2 * c[1] // 4, up_out=outer)
    if d == nd - 1:
        return dict(cell=1, downnorm=None, upconv=4, upnorm=5, drop=None, up_in=c[nd] // 4, up_out=outer)
    drop = 8 if f["use_dropout"] and 4 <= d <= nd - 2 else None
    return dict(cell=1, downnorm=2, upconv=6, upnorm=7, drop=drop, up_in=2 * c[d + 1] // 4, up_out=outer)


def key_shapes(f) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of every entry of the reference's state dict, in registration order"""
    nd, c = f["num_downs"], channels(f)
    inst = f["norm"] == "instance"

    def norm_keys(pre, ch):
        return [] if inst else [(pre + "." + leaf, () if leaf == "num_batches_tracked" else (ch,)) for leaf in BN_LEAVES]

    def walk(d):
        p, lay = block_prefix(d), block_layout(f, d)
        out = []
        for j, k in enumerate(KS):
            out.append((f"{p}{lay['cell']}._ops._ops.{j}.op.weight", (c[d + 1], c[d], k, k, k)))
            if inst:
                out.append((f"{p}{lay['cell']}._ops._ops.{j}.op.bias", (c[d + 1],)))
        if lay["downnorm"] is not None:
            out += norm_keys(f"{p}{lay['downnorm']}", c[d + 1])
        if d + 1 < nd:
            out += walk(d + 1)
        out.append((f"{p}{lay['upconv']}.weight", (lay["up_out"], lay["up_in"], 3, 3, 3)))
        out.append((f"{p}{lay['upconv']}.bias", (lay["up_out"],)))
        if lay["upnorm"] is not None:
            out += norm_keys(f"{p}{lay['upnorm']}", lay["up_out"])
        return out
    return walk(0)


def fixture_state_dict(f) -> Dict[str, torch.Tensor]:
    """conv weights ~ N(0, 1 / sqrt(fan_in)) (activations of order one at every level), biases N(0, 0.1), BatchNorm gamma N(1, 0.1),
    beta N(0, 0.1), running mean N(0, 0.2), running variance U(0.5, 1.5): a trained network's, so that nothing cancels by chance"""
    g = torch.Generator().manual_seed(f["seed"])
    sd: Dict[str, torch.Tensor] = {}
    for key, shape in key_shapes(f):
        leaf = key.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            sd[key] = torch.tensor(3, dtype=torch.long)
        elif len(shape) == 5:
            fan = shape[1] * shape[2] ** 3
            sd[key] = (torch.randn(shape, generator=g, dtype=torch.float64) * fan ** -0.5).float()
        elif leaf == "running_var":
            sd[key] = (torch.rand(shape, generator=g, dtype=torch.float64) + 0.5).float()
        elif leaf == "running_mean":
            sd[key] = (torch.randn(shape, generator=g, dtype=torch.float64) * 0.2).float()
        elif leaf == "weight":
            sd[key] = (1.0 + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)).float()
        else:
            sd[key] = (torch.randn(shape, generator=g, dtype=torch.float64) * 0.1).float()
    return sd


def fixture_input(f):
    return 0.5 * torch.randn((f["N"], f["input_nc"], f["D"], f["H"], f["W"]), generator=torch.Generator().manual_seed(f["seed"] + 1))


def fixture_arch(f):
    """conv_arch [6, 3] in double, rows of order one: a non-uniform architecture"""
    return torch.randn((6, 3), generator=torch.Generator().manual_seed(f["seed"] + 3), dtype=torch.float64)


def fixture_dense(f):
    """the fixed dense gradient of the image: loss = sum(y * dense)"""
    shape = (f["N"], f["output_nc"], f["D"], f["H"], f["W"])
    n = 1
    for s in shape:
        n *= s
    return (torch.rand(shape, generator=torch.Generator().manual_seed(f["seed"] + 2), dtype=torch.float64) * 2 - 1) / n


def lattice(y, f):
    """what the fixture stores of the image (the whole of it would not fit the size limit of a committed file): every `stride`-th
    voxel per axis; the whole image is held through its checksum and through the gradients, which depend on all of it"""
    s = f["stride"]
    return y[:, :, ::s, ::s, ::s]
