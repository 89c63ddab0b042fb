"""Pix2Pix networks of GenSeg on the MI355X HIP engine (reference: models_pix2pix/networks.py).

Same public names, module tree and state-dict keys as the reference for the parts reached by
`--model pix2pix` defaults: `UnetGenerator` (+ `UnetSkipConnectionBlock`, `Cell_upconv`, `MixedOp_upconv`),
`ResnetGenerator` (+ `ResnetBlock`), `NLayerDiscriminator`, `PixelDiscriminator`, `GANLoss`, `get_norm_layer`, `init_weights`, `init_net`, `define_G`, `define_D`, and the
architecture tensors `upconv_arch` / `conv_arch` / `arch_parameters()` (module globals, :443,:477-484).
The leaf torch modules only hold parameters; `UnetGenerator.forward` and `NLayerDiscriminator.forward`
run whole-network plans on the HIP kernels (pix2pix_engine.py: the U-Net generator and the steps all plans share; resnet_engine.py;
discriminator_engine.py: the discriminators on images and on volumes).  No ATen / CPU fallback."""
import functools

import torch
import torch.nn as nn
from torch.nn import init

from ..architecture_pix2pix.genotypes import PRIMITIVES_conv, PRIMITIVES_upconv
from ..architecture_pix2pix.operations import OPS
from ..losses import MODE_BCE_CONST, MODE_MEAN, MODE_MSE_CONST, mean_loss


class Identity(nn.Module):
    def forward(self, x):
        return x


def get_norm_layer(norm_type='instance', threed=False):
    """networks.py:23-41.  'batch' (the pix2pix default, pix2pix_model.py:34) and 'instance' (the default of --norm,
    options/base_options.py:36) run on the HIP engine.  threed (GenSeg-3D/models/networks.py:109-131): the BatchNorm3d /
    InstanceNorm3d partials, from which the discriminators build their 3-D form."""
    if norm_type == 'batch':
        return functools.partial(nn.BatchNorm3d if threed else nn.BatchNorm2d, affine=True, track_running_stats=True)
    if norm_type == 'instance':
        return functools.partial(nn.InstanceNorm3d if threed else nn.InstanceNorm2d, affine=False, track_running_stats=False)
    if norm_type == 'none':
        return lambda x: Identity()
    raise NotImplementedError('normalization layer [%s] is not found' % norm_type)


def init_weights(net, init_type='normal', init_gain=0.02):
    """networks.py:73-104 (same distributions; applied to the parameter-holding leaf modules)."""
    def init_func(m):
        classname = m.__class__.__name__
        if hasattr(m, 'weight') and (classname.find('Conv') != -1 or classname.find('Linear') != -1):
            if init_type == 'normal':
                init.normal_(m.weight.data, 0.0, init_gain)
            elif init_type == 'xavier':
                init.xavier_normal_(m.weight.data, gain=init_gain)
            elif init_type == 'kaiming':
                init.kaiming_normal_(m.weight.data, a=0, mode='fan_in')
            elif init_type == 'orthogonal':
                init.orthogonal_(m.weight.data, gain=init_gain)
            else:
                raise NotImplementedError('initialization method [%s] is not implemented' % init_type)
            if hasattr(m, 'bias') and m.bias is not None:
                init.constant_(m.bias.data, 0.0)
        elif classname.find('BatchNorm2d') != -1 or classname.find('BatchNorm3d') != -1:
            init.normal_(m.weight.data, 1.0, init_gain)
            init.constant_(m.bias.data, 0.0)
    net.apply(init_func)


def init_net(net, init_type='normal', init_gain=0.02, gpu_ids=[]):
    """networks.py:107-122.  Multi-GPU is one process per GPU (parallel.py), never nn.DataParallel."""
    if len(gpu_ids) > 1:
        raise NotImplementedError("use one process per GPU (semantic_segmentation_amd.parallel), not nn.DataParallel")
    if len(gpu_ids) == 1:
        assert torch.cuda.is_available()
        net.to(gpu_ids[0])
    init_weights(net, init_type, init_gain=init_gain)
    return net


def define_G(input_nc, output_nc, ngf, netG, norm='batch', use_dropout=False, init_type='normal', init_gain=0.02,
             gpu_ids=[], upsampling='deconvolution', threed=False):
    """upsampling / threed (GenSeg-3D/models/networks.py:216-262): threed=True with upsampling='linear' builds the 3-D
    linear-upsample U-Net (networks3d.UnetGenerator); there 'unet_128' means 6 downs (7 for images, as ever)."""
    if threed:
        if upsampling != 'linear' or netG not in ('unet_128', 'unet_256'):
            raise NotImplementedError("3-D generators on the MI355X hot path: netG 'unet_128' with upsampling='linear' (got netG=%r, "
                                      "upsampling=%r; the reference's 3-D 'deconvolution' blocks fail to construct)" % (netG, upsampling))
        if netG == 'unet_256':
            raise NotImplementedError("3-D 'unet_256' asks for 8 downs, but the reference's conv_arch has 6 rows (a seventh cell raises "
                                      "IndexError there): use 'unet_128' (6 downs) with upsampling='linear'")
        from .networks3d import UnetGenerator as UnetGenerator3d
        net = UnetGenerator3d(input_nc, output_nc, 6, ngf, norm_layer=get_norm_layer(norm_type=norm, threed=True),
                              upsampling=upsampling, use_dropout=use_dropout)
        return init_net(net, init_type, init_gain, gpu_ids)
    if upsampling != 'deconvolution':
        raise NotImplementedError("2-D generators on the MI355X hot path use upsampling='deconvolution' (got %r); upsampling='linear' "
                                  "is the 3-D U-Net: threed=True" % upsampling)
    norm_layer = get_norm_layer(norm_type=norm)
    if netG == 'unet_128':
        net = UnetGenerator(input_nc, output_nc, 7, ngf, norm_layer=norm_layer, use_dropout=use_dropout)
    elif netG == 'unet_256':
        net = UnetGenerator(input_nc, output_nc, 8, ngf, norm_layer=norm_layer, use_dropout=use_dropout)
    elif netG == 'resnet_9blocks':
        net = ResnetGenerator(input_nc, output_nc, ngf, norm_layer=norm_layer, use_dropout=use_dropout, n_blocks=9)
    elif netG == 'resnet_6blocks':
        net = ResnetGenerator(input_nc, output_nc, ngf, norm_layer=norm_layer, use_dropout=use_dropout, n_blocks=6)
    else:
        raise NotImplementedError('Generator model name [%s] is not on the MI355X hot path' % netG)
    return init_net(net, init_type, init_gain, gpu_ids)


def define_D(input_nc, ndf, netD, n_layers_D=3, norm='batch', init_type='normal', init_gain=0.02, gpu_ids=[], threed=False):
    """threed (GenSeg-3D/models/networks.py:265-311): the discriminators on volumes [N,C,D,H,W] (Conv3d leaves, 3-D norms)"""
    norm_layer = get_norm_layer(norm_type=norm, threed=threed)
    if netD == 'basic':
        net = NLayerDiscriminator(input_nc, ndf, n_layers=3, norm_layer=norm_layer)
    elif netD == 'n_layers':
        net = NLayerDiscriminator(input_nc, ndf, n_layers_D, norm_layer=norm_layer)
    elif netD == 'pixel':
        net = PixelDiscriminator(input_nc, ndf, norm_layer=norm_layer)
    else:
        raise NotImplementedError('Discriminator model name [%s] is not on the MI355X hot path' % netD)
    return init_net(net, init_type, init_gain, gpu_ids)


class GANLoss(nn.Module):
    """networks.py:215-281: vanilla = BCEWithLogits vs a constant label, lsgan = MSE, wgangp = -+mean; the
    label is never materialised (the reduction kernel takes it as a scalar)."""

    def __init__(self, gan_mode, target_real_label=1.0, target_fake_label=0.0):
        super(GANLoss, self).__init__()
        self.register_buffer('real_label', torch.tensor(target_real_label))
        self.register_buffer('fake_label', torch.tensor(target_fake_label))
        self.gan_mode = gan_mode
        if gan_mode not in ('lsgan', 'vanilla', 'wgangp'):
            raise NotImplementedError('gan mode %s not implemented' % gan_mode)
        self._labels = (float(target_real_label), float(target_fake_label))

    def get_target_tensor(self, prediction, target_is_real):
        return (self.real_label if target_is_real else self.fake_label).expand_as(prediction)

    def __call__(self, prediction, target_is_real):
        label = self._labels[0] if target_is_real else self._labels[1]
        if self.gan_mode == 'vanilla':
            return mean_loss(prediction, None, label, MODE_BCE_CONST)
        if self.gan_mode == 'lsgan':
            return mean_loss(prediction, None, label, MODE_MSE_CONST)
        return mean_loss(prediction, None, -1.0 if target_is_real else 1.0, MODE_MEAN)


# ---- architecture tensors (module globals like the reference: networks.py:441-484) -------------------
num_ops_conv = len(PRIMITIVES_conv)
conv_arch = (1e-3 * torch.randn(8, num_ops_conv)).requires_grad_(True)


def conv_arch_parameters():
    """The tensor the generator reads NOW: the reference returns a list captured at import time, which goes
    stale as soon as a script rebinds `networks.conv_arch` (pix2pix_model.py:59 does) -- its arch optimisers
    then own a tensor the forward pass never uses."""
    return [conv_arch, ]


num_ops_upconv = len(PRIMITIVES_upconv)
upconv_arch = (1e-3 * torch.randn(8, num_ops_upconv)).requires_grad_(True)


def upconv_arch_parameters():
    return [upconv_arch, ]


def arch_parameters():
    return [upconv_arch, conv_arch]


def _uses_instance_norm(norm_layer):
    """the reference's `use_bias` (networks.py:572-575, :631-634): the norm layer is InstanceNorm2d.  The engine runs the
    InstanceNorm the reference builds (affine=False, track_running_stats=False: no parameters, no buffers) and no other."""
    func = norm_layer.func if type(norm_layer) == functools.partial else norm_layer
    if func != nn.InstanceNorm2d:
        return False
    probe = norm_layer(8)
    for flag in ("affine", "track_running_stats"):
        if getattr(probe, flag):
            raise NotImplementedError("InstanceNorm2d with %s=True is not on the MI355X hot path (get_norm_layer('instance') "
                                      "builds affine=False, track_running_stats=False)" % flag)
    return True


def is_threed_layer(norm_layer):
    """GenSeg-3D/models/networks.py:89-93: the norm layer decides whether a discriminator is built on volumes"""
    func = norm_layer.func if type(norm_layer) == functools.partial else norm_layer
    return getattr(func, "__name__", "").find("3d") > -1


def add_bias(norm_layer, threed):
    """GenSeg-3D/models/networks.py:96-106: a conv in front of a norm carries a bias only under InstanceNorm (of the network's
    dimension).  As in 2-D the engine runs the InstanceNorm get_norm_layer builds (no parameters, no buffers) and no other."""
    if not threed:
        return _uses_instance_norm(norm_layer)
    func = norm_layer.func if type(norm_layer) == functools.partial else norm_layer
    if func != nn.InstanceNorm3d:
        return False
    probe = norm_layer(8)
    for flag in ("affine", "track_running_stats"):
        if getattr(probe, flag):
            raise NotImplementedError("InstanceNorm3d with %s=True is not on the MI355X hot path (get_norm_layer('instance', threed=True) "
                                      "builds affine=False, track_running_stats=False)" % flag)
    return True


class MixedOp_upconv(nn.Module):
    """networks.py:486-496: holds the three transposed-conv primitives (`_ops.{0,1,2}.op.*`)."""

    def __init__(self, C_in, C_out, bias):
        super(MixedOp_upconv, self).__init__()
        self._ops = nn.ModuleList()
        for primitive in PRIMITIVES_upconv:
            self._ops.append(OPS[primitive](C_in, C_out, bias))

    def forward(self, x, weights):
        """sum(w * op(x)) (networks.py:495-496) as ONE merged transposed conv on the HIP kernels (cell_engine.py)."""
        from .cell_engine import mixed_upconv
        return mixed_upconv(x, weights, list(self._ops))


class Cell_upconv(nn.Module):
    """networks.py:499-511."""

    def __init__(self, C_in, C_out, bias, layer_index):
        super(Cell_upconv, self).__init__()
        self._layer_index = layer_index
        self._ops = MixedOp_upconv(C_in, C_out, bias)

    def forward(self, input):
        """networks.py:507-511: softmax of this cell's row of the architecture tensor, then the mixed op."""
        weights = torch.softmax(upconv_arch[self._layer_index].to(input.device), dim=-1)
        return self._ops(input, weights)


class UnetSkipConnectionBlock(nn.Module):
    """networks.py:553-617: same Sequential layout (hence the same state-dict keys)."""

    def __init__(self, outer_nc, inner_nc, input_nc=None, layer_index=None, submodule=None, outermost=False,
                 innermost=False, norm_layer=nn.BatchNorm2d, use_dropout=False):
        super(UnetSkipConnectionBlock, self).__init__()
        self.outermost = outermost
        self.innermost = innermost
        use_bias = _uses_instance_norm(norm_layer)
        if input_nc is None:
            input_nc = outer_nc
        downconv = nn.Conv2d(input_nc, inner_nc, kernel_size=4, stride=2, padding=1, bias=use_bias)
        downrelu = nn.LeakyReLU(0.2, True)
        downnorm = norm_layer(inner_nc)
        uprelu = nn.ReLU(True)
        upnorm = norm_layer(outer_nc)
        if outermost:
            upconv = Cell_upconv(inner_nc * 2, outer_nc, bias=True, layer_index=layer_index)
            model = [downconv] + [submodule] + [uprelu, upconv, nn.Tanh()]
        elif innermost:
            upconv = Cell_upconv(inner_nc, outer_nc, bias=use_bias, layer_index=layer_index)
            model = [downrelu, downconv] + [uprelu, upconv, upnorm]
        else:
            upconv = Cell_upconv(inner_nc * 2, outer_nc, bias=use_bias, layer_index=layer_index)
            model = [downrelu, downconv, downnorm] + [submodule] + [uprelu, upconv, upnorm]
            if use_dropout:
                model = model + [nn.Dropout(0.5)]
        self.model = nn.Sequential(*model)

    def forward(self, x):
        raise RuntimeError("UnetSkipConnectionBlock runs inside UnetGenerator.forward (HIP engine)")


class UnetGenerator(nn.Module):
    """networks.py:514-550."""

    def __init__(self, input_nc, output_nc, num_downs, ngf=64, norm_layer=nn.BatchNorm2d, use_dropout=False,
                 compute_dtype=None):
        super(UnetGenerator, self).__init__()
        self.layer_index = 0
        unet_block = UnetSkipConnectionBlock(ngf * 8, ngf * 8, input_nc=None, layer_index=self.layer_index,
                                             submodule=None, norm_layer=norm_layer, innermost=True)
        self.layer_index += 1
        for i in range(num_downs - 5):
            unet_block = UnetSkipConnectionBlock(ngf * 8, ngf * 8, input_nc=None, layer_index=self.layer_index,
                                                 submodule=unet_block, norm_layer=norm_layer, use_dropout=use_dropout)
            self.layer_index += 1
        for mult in (4, 2, 1):
            unet_block = UnetSkipConnectionBlock(ngf * mult, ngf * mult * 2, input_nc=None,
                                                 layer_index=self.layer_index, submodule=unet_block,
                                                 norm_layer=norm_layer)
            self.layer_index += 1
        self.model = UnetSkipConnectionBlock(output_nc, ngf, input_nc=input_nc, layer_index=self.layer_index,
                                             submodule=unet_block, outermost=True, norm_layer=norm_layer)
        self.layer_index += 1
        from .pix2pix_engine import GeneratorEngine
        object.__setattr__(self, "_engine", GeneratorEngine(self, compute_dtype))

    @property
    def engine(self):
        return self._engine

    def forward(self, input, dropout_masks=None):
        """`dropout_masks`: optional list of uint8 keep-masks (NHWC) for the dropout blocks, innermost first;
        default draws them with torch.rand on the device (train mode) -- not the ATen Philox stream."""
        return self._engine.run(input, dropout_masks)


class ResnetBlock(nn.Module):
    """networks.py:382-439: same Sequential layout (ReflectionPad2d, Conv2d, norm, ReLU, [Dropout], ReflectionPad2d, Conv2d, norm)
    -- convs at conv_block.1 and .5 (.6 with dropout)."""

    def __init__(self, dim, padding_type, norm_layer, use_dropout, use_bias):
        super(ResnetBlock, self).__init__()
        self.conv_block = self.build_conv_block(dim, padding_type, norm_layer, use_dropout, use_bias)

    def build_conv_block(self, dim, padding_type, norm_layer, use_dropout, use_bias):
        if padding_type != 'reflect':
            raise NotImplementedError("ResnetBlock padding [%s] is not on the MI355X hot path: 'reflect' is supported" % padding_type)
        conv_block = [nn.ReflectionPad2d(1), nn.Conv2d(dim, dim, kernel_size=3, padding=0, bias=use_bias), norm_layer(dim),
                      nn.ReLU(True)]
        if use_dropout:
            conv_block += [nn.Dropout(0.5)]
        conv_block += [nn.ReflectionPad2d(1), nn.Conv2d(dim, dim, kernel_size=3, padding=0, bias=use_bias), norm_layer(dim)]
        return nn.Sequential(*conv_block)

    def forward(self, x):
        raise RuntimeError("ResnetBlock runs inside ResnetGenerator.forward (HIP engine)")


class ResnetGenerator(nn.Module):
    """networks.py:321-379 (the generator of `--netG resnet_9blocks`, the default of options/base_options.py:34, and
    `resnet_6blocks`): same Sequential indices, hence the same state-dict keys."""

    def __init__(self, input_nc, output_nc, ngf=64, norm_layer=nn.BatchNorm2d, use_dropout=False, n_blocks=6,
                 padding_type='reflect', compute_dtype=None):
        assert (n_blocks >= 0)
        super(ResnetGenerator, self).__init__()
        from .resnet_engine import ResnetGeneratorEngine, check_supported
        use_bias = check_supported(input_nc, output_nc, ngf, norm_layer, padding_type)
        model = [nn.ReflectionPad2d(3), nn.Conv2d(input_nc, ngf, kernel_size=7, padding=0, bias=use_bias), norm_layer(ngf),
                 nn.ReLU(True)]
        n_downsampling = 2
        for i in range(n_downsampling):
            mult = 2 ** i
            model += [nn.Conv2d(ngf * mult, ngf * mult * 2, kernel_size=3, stride=2, padding=1, bias=use_bias),
                      norm_layer(ngf * mult * 2), nn.ReLU(True)]
        mult = 2 ** n_downsampling
        for i in range(n_blocks):
            model += [ResnetBlock(ngf * mult, padding_type=padding_type, norm_layer=norm_layer, use_dropout=use_dropout,
                                  use_bias=use_bias)]
        for i in range(n_downsampling):
            mult = 2 ** (n_downsampling - i)
            model += [nn.ConvTranspose2d(ngf * mult, int(ngf * mult / 2), kernel_size=3, stride=2, padding=1, output_padding=1,
                                         bias=use_bias), norm_layer(int(ngf * mult / 2)), nn.ReLU(True)]
        model += [nn.ReflectionPad2d(3)]
        model += [nn.Conv2d(ngf, output_nc, kernel_size=7, padding=0)]
        model += [nn.Tanh()]
        self.model = nn.Sequential(*model)
        object.__setattr__(self, "_engine", ResnetGeneratorEngine(self, compute_dtype))

    @property
    def engine(self):
        return self._engine

    def forward(self, input, dropout_masks=None):
        """`dropout_masks`: optional list of uint8 keep-masks (NHWC [N,H/4,W/4,4*ngf]) for the blocks' dropout, one per block, first
        block first; default draws them with torch.rand on the device (train mode) -- not the ATen Philox stream."""
        return self._engine.run(input, dropout_masks)


class NLayerDiscriminator(nn.Module):
    """networks.py:620-665 PatchGAN (same Sequential indices: convs at 0,2,5,8,11; norms at 3,6,9).  With a 3-D norm layer
    (GenSeg-3D/models/networks.py:806-855) the leaves are nn.Conv3d -- same indices, 5-D weights -- and the plan is
    discriminator_engine.Discriminator3DEngine."""

    def __init__(self, input_nc, ndf=64, n_layers=3, norm_layer=nn.BatchNorm2d, compute_dtype=None):
        super(NLayerDiscriminator, self).__init__()
        threed = is_threed_layer(norm_layer)
        use_bias = add_bias(norm_layer, threed)
        conv_layer = nn.Conv3d if threed else nn.Conv2d
        kw, padw = 4, 1
        sequence = [conv_layer(input_nc, ndf, kernel_size=kw, stride=2, padding=padw), nn.LeakyReLU(0.2, True)]
        nf_mult = 1
        for n in range(1, n_layers):
            nf_mult_prev, nf_mult = nf_mult, min(2 ** n, 8)
            sequence += [conv_layer(ndf * nf_mult_prev, ndf * nf_mult, kernel_size=kw, stride=2, padding=padw,
                                    bias=use_bias), norm_layer(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        nf_mult_prev, nf_mult = nf_mult, min(2 ** n_layers, 8)
        sequence += [conv_layer(ndf * nf_mult_prev, ndf * nf_mult, kernel_size=kw, stride=1, padding=padw,
                                bias=use_bias), norm_layer(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        sequence += [conv_layer(ndf * nf_mult, 1, kernel_size=kw, stride=1, padding=padw)]
        self.model = nn.Sequential(*sequence)
        self.threed = threed
        if threed:
            from .discriminator_engine import Discriminator3DEngine
            object.__setattr__(self, "_engine", Discriminator3DEngine(self, compute_dtype))
        else:
            from .discriminator_engine import DiscriminatorEngine
            object.__setattr__(self, "_engine", DiscriminatorEngine(self, compute_dtype))

    @property
    def engine(self):
        return self._engine

    def forward(self, input):
        return self._engine.run(input)


class PixelDiscriminator(nn.Module):
    """networks.py:668-697 1x1 PatchGAN (pixelGAN): the reference's module tree (Sequential `net`: convs at 0, 2, 5; the norm at 3;
    the last conv carries a bias only under InstanceNorm, :691) on the PatchGAN plan with 1x1 kernels (DiscriminatorEngine)."""

    def __init__(self, input_nc, ndf=64, norm_layer=nn.BatchNorm2d, compute_dtype=None):
        super(PixelDiscriminator, self).__init__()
        threed = is_threed_layer(norm_layer)                   # GenSeg-3D/models/networks.py:858-886: Conv3d leaves, same indices
        use_bias = add_bias(norm_layer, threed)
        conv_layer = nn.Conv3d if threed else nn.Conv2d
        self.net = nn.Sequential(
            conv_layer(input_nc, ndf, kernel_size=1, stride=1, padding=0),
            nn.LeakyReLU(0.2, True),
            conv_layer(ndf, ndf * 2, kernel_size=1, stride=1, padding=0, bias=use_bias),
            norm_layer(ndf * 2),
            nn.LeakyReLU(0.2, True),
            conv_layer(ndf * 2, 1, kernel_size=1, stride=1, padding=0, bias=use_bias))
        self.threed = threed
        if threed:
            from .discriminator_engine import Discriminator3DEngine
            object.__setattr__(self, "_engine", Discriminator3DEngine(self, compute_dtype, seq="net"))
        else:
            from .discriminator_engine import DiscriminatorEngine
            object.__setattr__(self, "_engine", DiscriminatorEngine(self, compute_dtype, seq="net"))

    @property
    def engine(self):
        return self._engine

    def forward(self, input):
        return self._engine.run(input)
