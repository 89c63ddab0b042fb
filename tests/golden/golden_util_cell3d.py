"""Seeded weights and inputs of the 3-D cell fixture tests/golden/pix2pix3d_cells.npz (made by make_golden_cell3d.py from the reference's
own GenSeg-3D classes in double).  Only checksums of the weights are stored: everything here is regenerated from the seeds."""
from typing import Dict

import torch

KS = (4, 6, 8)
PREFIX = {"cell": "_ops._ops.%d.", "mixed": "_ops.%d.", "conv_421": "", "conv_622": "", "conv_823": ""}

# kind cell: Cell_conv(cin, cout, bias, layer) reading conv_arch; mixed: MixedOp_conv(cin, cout, bias) with softmax(arch[layer]) passed
# in; conv_*: one primitive on its own; up: LinearAdditiveUpsample(2, 4, threed=True).  Non-cubic volumes; odd sizes; both image sides.
FIXTURES = {
    "pix2pix3d_cells": [dict(tag="cell_img1", kind="cell", cin=1, cout=16, bias=True, N=2, D=8, H=12, W=10, layer=4, seed=81),
                        dict(tag="cell_c16", kind="cell", cin=16, cout=24, bias=True, N=2, D=6, H=4, W=8, layer=2, seed=82),
                        dict(tag="mixed_c8_odd", kind="mixed", cin=8, cout=16, bias=False, N=1, D=5, H=7, W=6, layer=0, seed=83),
                        dict(tag="k6_img3", kind="conv_622", cin=3, cout=8, bias=True, N=1, D=6, H=4, W=6, layer=0, seed=84),
                        dict(tag="k4_c8_deep", kind="conv_421", cin=8, cout=8, bias=True, N=2, D=2, H=2, W=2, layer=0, seed=86),
                        dict(tag="up_c32", kind="up", cin=32, N=2, D=2, H=3, W=4, seed=85),
                        dict(tag="up_c64_odd", kind="up", cin=64, N=1, D=3, H=2, W=5, seed=87)],
}


def _normal(g, shape, std):
    return (torch.randn(shape, generator=g, dtype=torch.float64) * std).float()


def fixture_state_dict(f) -> Dict[str, torch.Tensor]:
    """the keys of the reference module of the fixture's kind: Conv3d weights [co, ci, k, k, k] ~ N(0, 1 / sqrt(fan_in)), biases N(0, 0.1)"""
    g = torch.Generator().manual_seed(f["seed"])
    sd: Dict[str, torch.Tensor] = {}
    if f["kind"] == "up":
        return sd
    ks = KS if f["kind"] in ("cell", "mixed") else (int(f["kind"][5]),)
    for j, k in enumerate(ks):
        pre = PREFIX[f["kind"]] % j if "%d" in PREFIX[f["kind"]] else ""
        sd[pre + "op.weight"] = _normal(g, (f["cout"], f["cin"], k, k, k), (f["cin"] * k ** 3) ** -0.5)
        if f["bias"]:
            sd[pre + "op.bias"] = _normal(g, (f["cout"],), 0.1)
    return sd


def fixture_input(f):
    return 0.5 * torch.randn((f["N"], f["cin"], f["D"], f["H"], f["W"]), generator=torch.Generator().manual_seed(f["seed"] + 1))


def fixture_arch(f):
    """conv_arch [6, 3] in double, rows of order one (mixing weights well apart from 1/3)"""
    return torch.randn((6, 3), generator=torch.Generator().manual_seed(f["seed"] + 3), dtype=torch.float64)


def fixture_dense(shape, f):
    """the fixed dense gradient of the output: loss = sum(y * dense)"""
    g = torch.Generator().manual_seed(f["seed"] + 2)
    n = 1
    for s in shape:
        n *= s
    return (torch.rand(tuple(shape), generator=g, dtype=torch.float64) * 2 - 1) / n
