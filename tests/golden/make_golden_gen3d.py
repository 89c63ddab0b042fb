"""Fixture of the 3-D Pix2Pix generator from the ORIGINAL reference classes (read-only checkout, its GenSeg-3D directory, CPU), run in
DOUBLE: tests/golden/pix2pix3d_gen.npz -- UnetGenerator(..., upsampling='linear') under BatchNorm3d (train and eval) and
InstanceNorm3d, and with dropout blocks in eval mode.  As make_golden_cell3d.py: weights, input, conv_arch and the dense gradient are
regenerated from the seed by golden_util_gen3d.py (only checksums are stored) and loaded with load_state_dict(strict=True), which also
proves that the key sets and 5-D shapes are the reference's.  Per part: conv_arch, the image on a lattice (golden_util_gen3d.lattice:
the whole of it would not fit the size limit) with its checksum and summary, the keys and shapes, and the gradients of sum(y * dense):
dx and the weights as summaries, the biases / norm parameters and the conv_arch gradient in full.

Usage:  python tests/golden/make_golden_gen3d.py"""
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
from golden_util_gen3d import FIXTURES, fixture_arch, fixture_dense, fixture_input, fixture_state_dict, lattice  # noqa: E402

torch.set_num_threads(8)


def make(name, parts):
    from models import networks
    out = {}
    for f in parts:
        t = f["tag"] + "/"
        x = fixture_input(f).double().requires_grad_(True)
        sd = fixture_state_dict(f)
        arch = fixture_arch(f).requires_grad_(True)
        net = networks.UnetGenerator(f["input_nc"], f["output_nc"], f["num_downs"], f["ngf"],
                                     norm_layer=networks.get_norm_layer(f["norm"], threed=True), upsampling="linear",
                                     use_dropout=f["use_dropout"])
        net.load_state_dict(sd, strict=True)
        net = net.double()
        net.train(f["train"])
        out[t + "keys"] = np.array(list(net.state_dict().keys()))
        out[t + "shapes"] = np.array([list(v.shape) + [0] * (5 - v.dim()) for v in net.state_dict().values()])
        for k, v in sd.items():
            if v.is_floating_point():
                out[t + "wsum/" + k] = tensor_checksum(v)
        networks.conv_arch = arch                          # Cell_conv.forward reads the module global
        y = net(x)
        dense = fixture_dense(f)
        (y * dense).sum().backward()
        out[t + "y_lattice"] = lattice(y.detach(), f).numpy()
        out[t + "ysum"], out[t + "gsum/y"] = tensor_checksum(y), grad_summary(y)
        out[t + "gsum/dx"] = grad_summary(x.grad)
        for k, p in net.named_parameters():
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            out[t + ("gsum/" if p.dim() > 1 else "grad/") + k] = grad_summary(g) if p.dim() > 1 else g.numpy()
        out[t + "arch"] = arch.detach().numpy()
        out[t + "grad/arch"] = (arch.grad if arch.grad is not None else torch.zeros_like(arch)).numpy()
        print(f["tag"], len(net.state_dict()), "keys, image", tuple(y.shape))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for name, parts in FIXTURES.items():
        make(name, parts)
