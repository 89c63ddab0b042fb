"""Fixture of the two 3-D generator operators from the ORIGINAL reference classes (read-only checkout, its GenSeg-3D directory, CPU), run
in DOUBLE: tests/golden/pix2pix3d_cells.npz -- Cell_conv (reading its module's conv_arch), MixedOp_conv, conv_421 / conv_622 on their
own and LinearAdditiveUpsample(2, 4, threed=True).  As make_golden_disc3d.py: weights are regenerated from the seed by
golden_util_cell3d.py (only checksums are stored) and loaded with load_state_dict(strict=True), which also proves that the key sets and
5-D shapes are the reference's.  Per part: the input (fp32), conv_arch, the output, the dense gradient, and the gradients of
sum(y * dense): dx and the weights as summaries, the biases and the conv_arch gradient in full; per module its state-dict keys and shapes.

Usage:  python tests/golden/make_golden_cell3d.py"""
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
from golden_util_cell3d import FIXTURES, fixture_arch, fixture_dense, fixture_input, fixture_state_dict  # noqa: E402

torch.set_num_threads(8)


def make(name, parts):
    from architecture_pix2pix import operations
    from models import networks
    out = {}
    for f in parts:
        t = f["tag"] + "/"
        x32 = fixture_input(f)
        x = x32.double().requires_grad_(True)
        out[t + "input"] = x32.numpy()
        if f["kind"] == "up":
            net, arch = networks.LinearAdditiveUpsample(2, 4, True), None
            y = net(x)
        else:
            sd = fixture_state_dict(f)
            arch = fixture_arch(f).requires_grad_(True)
            if f["kind"] == "cell":
                net = networks.Cell_conv(f["cin"], f["cout"], f["bias"], f["layer"])
            elif f["kind"] == "mixed":
                net = networks.MixedOp_conv(f["cin"], f["cout"], f["bias"])
            else:
                net = operations.OPS[f["kind"]](f["cin"], f["cout"], f["bias"])
            net.load_state_dict(sd, strict=True)
            net = net.double()
            out[t + "keys"] = np.array(list(net.state_dict().keys()))
            out[t + "shapes"] = np.array([list(v.shape) + [0] * (5 - v.dim()) for v in net.state_dict().values()])
            for k, v in sd.items():
                out[t + "wsum/" + k] = tensor_checksum(v)
            if f["kind"] == "cell":
                networks.conv_arch = arch                      # Cell_conv.forward reads the module global
                y = net(x)
            elif f["kind"] == "mixed":
                y = net(x, torch.softmax(arch[f["layer"]], -1))
            else:
                y = net(x)
        dense = fixture_dense(y.shape, f)
        (y * dense).sum().backward()
        out[t + "y"], out[t + "dense"] = y.detach().numpy(), dense.numpy()
        out[t + "gsum/dx"] = grad_summary(x.grad)
        for k, p in net.named_parameters():
            out[t + ("gsum/" if p.dim() > 1 else "grad/") + k] = grad_summary(p.grad) if p.dim() > 1 else p.grad.numpy()
        if arch is not None:
            out[t + "arch"] = arch.detach().numpy()
            out[t + "grad/arch"] = (arch.grad if arch.grad is not None else torch.zeros_like(arch)).numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for name, parts in FIXTURES.items():
        make(name, parts)
