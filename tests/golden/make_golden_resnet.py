"""Fixtures of the ResNet generator (`--netG resnet_9blocks` / `resnet_6blocks`) from the ORIGINAL reference module (read-only
checkout, CPU), run in DOUBLE: tests/golden/pix2pix_resnet_{a,b}.npz.  As make_golden_instance.py: weights are regenerated from the
seed by golden_util_resnet.py (only checksums are stored) and loaded with load_state_dict(strict=True), which also proves that the
key set is the reference's.  Fixture A carries the Dropout modules with p set to 0, so its train image needs no mask; the eval image
is stored on its own (BatchNorm: running statistics).  Gradients are those of golden_util_resnet.fixture_loss.

Usage:  python tests/golden/make_golden_resnet.py"""
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
from golden_util_resnet import FIXTURES, fixture_inputs, fixture_loss, fixture_state_dict  # noqa: E402

torch.set_num_threads(8)


def make(name, f):
    from models_pix2pix import networks
    sd = fixture_state_dict(f)

    def gen():
        G = networks.ResnetGenerator(f["cin"], f["cout"], f["ngf"], norm_layer=networks.get_norm_layer(f["norm"]),
                                     use_dropout=f["use_dropout"], n_blocks=f["n_blocks"])
        G.load_state_dict(sd, strict=True)
        for m in G.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        return G.double()

    x, real, dense = fixture_inputs(f)
    x = x.double().requires_grad_(True)
    out = {"input": x.detach().numpy(), "real": real.numpy(), "dense": dense.numpy()}
    G = gen().train()
    image = G(x)
    loss = fixture_loss(image, real.double(), dense.double())
    loss.backward()
    out["image"] = image.detach().numpy()
    out["loss"] = loss.item()
    out["gsum/dx"] = grad_summary(x.grad)
    for k, p in G.named_parameters():
        out["gsum/" + k] = grad_summary(p.grad)
    with torch.no_grad():
        out["image_eval"] = gen().eval()(x.detach()).numpy()
    for k, v in sd.items():
        out["wsum/" + k] = tensor_checksum(v)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", loss.item(), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for name, f in FIXTURES.items():
        make(name, f)
