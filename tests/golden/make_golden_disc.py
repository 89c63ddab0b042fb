"""Fixtures of the discriminators from the ORIGINAL reference classes (read-only checkout, CPU), run in DOUBLE:
tests/golden/pix2pix_disc_patch.npz (NLayerDiscriminator(6, 64, 3) under BatchNorm) and pix2pix_disc_pixel.npz (PixelDiscriminator
under BatchNorm with 2 input channels and under InstanceNorm with 6).  As make_golden_resnet.py: weights are regenerated from the seed
by golden_util_disc.py (only checksums are stored) and loaded with load_state_dict(strict=True), which also proves that the key sets
are the reference's.  Per network: the input, the train-mode logits, the eval-mode logits (BatchNorm: with perturbed running
statistics), and summaries of the gradients of sum(logits * dense) in train mode, dx included.

Usage:  python tests/golden/make_golden_disc.py"""
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
sys.path.insert(0, REF)

from golden_util import grad_summary, tensor_checksum  # noqa: E402
from golden_util_disc import FIXTURES, fixture_dense, fixture_input, fixture_state_dict, perturbed_running  # noqa: E402

torch.set_num_threads(8)


def build(f, sd):
    from models_pix2pix import networks
    norm = networks.get_norm_layer(f["norm"])
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
        x = fixture_input(f).double().requires_grad_(True)
        net = build(f, sd).train()
        logits = net(x)
        dense = fixture_dense(logits.shape, f)
        (logits * dense).sum().backward()
        out[t + "input"], out[t + "logits"], out[t + "dense"] = x.detach().numpy(), logits.detach().numpy(), dense.numpy()
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
