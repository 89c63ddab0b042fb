"""The reference's 3-D Pix2Pix generator classes on the HIP path (GenSeg-3D/models/networks.py, a different file from the 2-D
models_pix2pix/networks.py: its `conv_arch` has 6 rows and `arch_parameters()` returns `[conv_arch]` only, so it has globals of its
own here): the mixed down-conv cell (`MixedOp_conv`, `Cell_conv`, :570-601), `LinearAdditiveUpsample` (:50-81), and the generator
assembled from them, `LinearUpsampleUnetSkipConnectionBlock` / `UnetGenerator` (:604-728; `networks.define_G(..., threed=True,
upsampling='linear')` builds it).  They take and return fp32 NCDHW tensors, support first-order autograd, and raise on a CPU tensor;
construction and load_state_dict work on the CPU.  The stand-alone cells run their own launches; `UnetGenerator.forward` runs the
whole-network plan of generator3d_engine.py.  The model class around G and D (`create_model('pix2pix3d')`) is not here yet."""
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


class LinearUpsampleUnetSkipConnectionBlock(nn.Module):
    """GenSeg-3D/models/networks.py:654-728 for a 3-D norm layer: the reference's Sequential layout (outermost: cell 0, submodule 1,
    up-conv 4; middle: cell 1, norm 2, submodule 3, up-conv 6, norm 7, [dropout 8]; innermost: cell 1, up-conv 4, norm 5), hence its
    state-dict keys.  The up-conv always carries a bias, also under BatchNorm3d."""

    def __init__(self, outer_nc, inner_nc, input_nc=None, submodule=None, outermost=False, innermost=False,
                 norm_layer=nn.BatchNorm3d, use_dropout=False, n_splits=4, layer_index=-1):
        super().__init__()
        from .networks import add_bias, is_threed_layer
        self.outermost, self.innermost = outermost, innermost
        threed = is_threed_layer(norm_layer)
        if not threed or n_splits != 4:
            raise NotImplementedError("LinearUpsampleUnetSkipConnectionBlock on the HIP path: a 3-D norm layer "
                                      "(get_norm_layer('batch' | 'instance', threed=True)) and n_splits == 4")
        use_bias = add_bias(norm_layer, threed)
        upsample = LinearAdditiveUpsample(scale_factor=2, n_splits=n_splits, threed=threed)
        if input_nc is None:
            input_nc = outer_nc
        downconv = Cell_conv(input_nc, inner_nc, bias=use_bias, layer_index=layer_index)
        downrelu = nn.LeakyReLU(0.2, True)
        downnorm = norm_layer(inner_nc)
        uprelu = nn.ReLU(True)
        upnorm = norm_layer(outer_nc)
        if outermost:
            upconv = nn.Conv3d((inner_nc * 2) // n_splits, outer_nc, kernel_size=3, stride=1, padding=1)
            model = [downconv] + [submodule] + [uprelu, upsample, upconv, nn.Tanh()]
        elif innermost:
            upconv = nn.Conv3d(inner_nc // n_splits, outer_nc, kernel_size=3, stride=1, padding=1)
            model = [downrelu, downconv] + [uprelu, upsample, upconv, upnorm]
        else:
            upconv = nn.Conv3d((inner_nc * 2) // n_splits, outer_nc, kernel_size=3, stride=1, padding=1)
            model = [downrelu, downconv, downnorm] + [submodule] + [uprelu, upsample, upconv, upnorm]
            if use_dropout:
                model = model + [nn.Dropout(0.5)]
        self.model = nn.Sequential(*model)

    def forward(self, x):
        raise RuntimeError("LinearUpsampleUnetSkipConnectionBlock runs inside UnetGenerator.forward (HIP engine)")


class UnetGenerator(nn.Module):
    """GenSeg-3D/models/networks.py:604-651 with upsampling='linear': `num_downs` blocks, innermost first, `layer_index` 0 at the
    innermost; channels input_nc -> ngf -> 2 ngf -> 4 ngf -> 8 ngf -> 8 ngf ...  (The reference's other value, 'deconvolution',
    raises a TypeError there: UnetSkipConnectionBlock takes no layer_index.)"""

    def __init__(self, input_nc, output_nc, num_downs, ngf=64, norm_layer=nn.BatchNorm3d, upsampling='linear', use_dropout=False,
                 compute_dtype=None):
        super().__init__()
        from .generator3d_engine import Generator3DEngine, check_supported
        check_supported(input_nc, output_nc, num_downs, ngf, norm_layer, upsampling)
        blk = LinearUpsampleUnetSkipConnectionBlock
        layer_index = 0
        unet_block = blk(ngf * 8, ngf * 8, input_nc=None, submodule=None, norm_layer=norm_layer, innermost=True, layer_index=layer_index)
        layer_index += 1
        for i in range(num_downs - 5):
            unet_block = blk(ngf * 8, ngf * 8, input_nc=None, submodule=unet_block, norm_layer=norm_layer, use_dropout=use_dropout,
                             layer_index=layer_index)
            layer_index += 1
        for mult in (4, 2, 1):
            unet_block = blk(ngf * mult, ngf * mult * 2, input_nc=None, submodule=unet_block, norm_layer=norm_layer,
                             layer_index=layer_index)
            layer_index += 1
        self.model = blk(output_nc, ngf, input_nc=input_nc, submodule=unet_block, outermost=True, norm_layer=norm_layer,
                         layer_index=layer_index)
        object.__setattr__(self, "_engine", Generator3DEngine(self, compute_dtype))

    @property
    def engine(self):
        return self._engine

    def forward(self, input, dropout_masks=None):
        """`dropout_masks`: optional list of uint8 keep-masks ([N*D,H,W,C], the device layout) for the dropout blocks, innermost
        first; default draws them with torch.rand on the device (train mode) -- not the ATen Philox stream."""
        return self._engine.run(input, dropout_masks)
