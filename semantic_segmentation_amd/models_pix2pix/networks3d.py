"""The reference's 3-D Pix2Pix module classes that run on the HIP path so far (GenSeg-3D/models/networks.py, a different file from
the 2-D models_pix2pix/networks.py: its `conv_arch` has 6 rows and `arch_parameters()` returns `[conv_arch]` only, so it has globals
of its own here): the mixed down-conv cell (`MixedOp_conv`, `Cell_conv`, :570-601) and `LinearAdditiveUpsample` (:50-81).  They take
and return fp32 NCDHW tensors, support first-order autograd, and raise on a CPU tensor; construction and load_state_dict work on the
CPU.  The generator that is assembled from them (`define_G(..., threed=True)`, `create_model('pix2pix3d')`) is not here yet."""
import torch
import torch.nn as nn

from ..architecture_pix2pix.genotypes import PRIMITIVES_conv
from ..architecture_pix2pix.operations import OPS

num_ops_conv = len(PRIMITIVES_conv)
conv_arch = (1e-3 * torch.randn(6, num_ops_conv)).requires_grad_(True)


def arch_parameters():
    """The tensor the cells read NOW (see networks.conv_arch_parameters: the reference's import-time list goes stale as soon as a
    script rebinds `conv_arch`)."""
    return [conv_arch, ]


class MixedOp_conv(nn.Module):
    def __init__(self, C_in, C_out, bias):
        super().__init__()
        self._ops = nn.ModuleList()
        for primitive in PRIMITIVES_conv:
            self._ops.append(OPS[primitive](C_in, C_out, bias))

    def forward(self, x, weights):
        from .cell3d_engine import mixed_conv3d
        return mixed_conv3d(x, weights, list(self._ops))


class Cell_conv(nn.Module):
    def __init__(self, C_in, C_out, bias, layer_index):
        super().__init__()
        self._layer_index = layer_index
        self._ops = MixedOp_conv(C_in, C_out, bias)

    def forward(self, input):
        weight = nn.functional.softmax(conv_arch[self._layer_index, :].to(input.device), dim=-1)     # the module global, read per call
        return self._ops(input, weight)


class LinearAdditiveUpsample(nn.Module):
    """Trilinear x2 upsample (align_corners=False) followed by the sum of each `n_splits` consecutive channels (Wojna et al.)."""

    def __init__(self, scale_factor, n_splits, threed):
        super().__init__()
        self.scale_factor = scale_factor
        self.n_splits = n_splits
        self.threed = threed
        self.mode = 'trilinear' if threed else 'bilinear'

    def forward(self, input_tensor):
        from .cell3d_engine import linear_additive_upsample
        return linear_additive_upsample(input_tensor, self.scale_factor, self.n_splits, self.threed)
