"""Fixture of the 3-D discriminators from the ORIGINAL reference classes (read-only checkout, its GenSeg-3D directory, CPU), run in
DOUBLE: tests/golden/pix2pix3d_disc.npz -- NLayerDiscriminator(2, 64, 3) under BatchNorm3d, NLayerDiscriminator(2, 16, 2) under
InstanceNorm3d and PixelDiscriminator(2, 64) under BatchNorm3d.  As make_golden_disc.py: weights are regenerated from the seed by
golden_util_disc3d.py (only checksums are stored) and loaded with load_state_dict(strict=True), which also proves that the key sets
and 5-D shapes are the reference's.  Per network: the input (fp32), the train-mode logits, the eval-mode logits (BatchNorm3d: with
perturbed running statistics), and summaries of the gradients of sum(logits * dense) in train mode, dx included.

Usage:  python tests/golden/make_golden_disc3d.py"""
import os
import sys

sys.dont_write_bytecode = True          # the reference checkout is read-only: no __pycache__ there

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = os.environ.get("GENSEG_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "GenSeg-3D"))

from golden_util import grad_summary, tensor_checksum  # noqa: E402
from golden_util_disc3d import FIXTURES, fixture_dense, fixture_input, fixture_state_dict, perturbed_running  # noqa: E402

torch.set_num_threads(8)


def build(f, sd):
    from models import networks
    norm = networks.get_norm_layer(f["norm"], threed=True)
    if f["kind"] == "patch":
        net = networks.NLayerDiscriminator(f["cin"], f["ndf"], f["n_layers"], norm_layer=norm)
    else:
        net = networks.PixelDiscriminator(f["cin"], f["ndf"], norm_layer=norm)
    net.load_state_dict(sd, strict=True)
    return net.double()


def make(name, parts):
    out = {}
    for f in parts:
        t = f["tag"] + "/"
        sd = fixture_state_dict(f)
        x32 = fixture_input(f)
        x = x32.double().requires_grad_(True)
        net = build(f, sd).train()
        logits = net(x)
        dense = fixture_dense(logits.shape, f)
        (logits * dense).sum().backward()
        out[t + "input"], out[t + "logits"], out[t + "dense"] = x32.numpy(), logits.detach().numpy(), dense.numpy()
        out[t + "gsum/dx"] = grad_summary(x.grad)
        for k, p in net.named_parameters():
            out[t + "gsum/" + k] = grad_summary(p.grad)
        with torch.no_grad():
            out[t + "logits_eval"] = build(f, perturbed_running(sd, f["seed"] + 3)).eval()(x.detach()).numpy()
        for k, v in sd.items():
            out[t + "wsum/" + k] = tensor_checksum(v)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for name, parts in FIXTURES.items():
        make(name, parts)
