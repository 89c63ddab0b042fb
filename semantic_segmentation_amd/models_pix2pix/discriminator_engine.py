"""Whole-network plan of the Pix2Pix discriminators on the HIP kernels, forward and backward, on images and on volumes.

One stage walk (_DiscriminatorPlan) serves NLayerDiscriminator (PatchGAN; reference models_pix2pix/networks.py:620-665) and
PixelDiscriminator (:668-697, the same stages with 1x1 kernels: seq="net"), and their 3-D forms (GenSeg-3D/models/networks.py:806-890
with a 3-D norm layer: nn.Conv3d leaves; the netD of `--model pix2pix3d`, GenSeg-3D/train_end2end.py:143-178):
  * the image-side conv (model.0 / net.0) reads the fp32 NCHW / NCDHW input directly and adds bias + LeakyReLU;
  * every middle conv (k4 s2 p1, k4 s1 p1, or k1 in the pixel net) is ONE gs_conv_igemm launch; BatchNorm statistics come out of
    the conv epilogue (count N*OD*OH*OW), InstanceNorm statistics per (sample, channel) from gs_in_stats;
  * the one-channel head writes fp32 logits.
Backward: the head's kernel; per middle stage the norm + LeakyReLU backward (pix2pix_engine.norm_act_bwd), the deterministic weight
gradient straight into the reference layout (gs_conv_wgrad_slabs + gs_wgrad_reduce_unpack) and the data gradient; weight gradient /
gs_colsum / data gradient at the image.  A middle conv's bias exists only under InstanceNorm, where it cancels in the norm: not
added, gradient exact zeros.  Gradients are carried times a power-of-two scale; weight packs are version-keyed; the data-parallel
hooks are those of the generators.
The two engines supply the facts that differ, as data or short hooks:
  DiscriminatorEngine    images [N,C,H,W], 16-bit tensors [N,H,W,C].  Image side: the direct kernels for 1..4 channels, the fp32-MFMA
                         kernels of csrc/ends_img.hip for 5..16 (pix2pix_engine.image_conv_*); stride-2 data gradient: four classes of
                         input pixels in one batched launch; head: gs_conv_smallcout_*.
  Discriminator3DEngine  volumes [N,C,D,H,W], which live as a stack of depth slices [N*D,H,W,C] as in unet3d_engine.py.  Image side:
                         csrc/ends_img.hip gs_conv3d_img_*; middle convs with up to 64 depth-strided taps (ops.geom_conv3d), InstanceNorm3d
                         statistics over the WHOLE volume on the [N, OD*OH, OW, C] view; stride-2 data gradient: the eight sub-voxel
                         classes of eight taps in two batched launches of four; head: gs_conv3d_head_* (logits [N,1,OD,OH,OW])."""
from __future__ import annotations

import math

import torch

from .. import ops
from .._lib import ACT_LEAKY02
from ..engine_common import ParamIndex, _flush_nbt, bn_coeffs, compute_dtype, pack_reuse_allowed
from .pix2pix_engine import (IMAGE_NC_MAX, _EmitDict, _PackCache, _bias32, _check_image_conv, _need_cuda, _ver, cached_geom,
                             conv_s2_dgrad, conv_wgrad, grad_scale, image_conv_dgrad, image_conv_fwd, image_conv_wgrad,
                             instance_stats, norm_act_bwd, pack_conv, param_grads, per_sample)

NDF_MAX = 128               # output channels of the 3-D image-side kernels: any multiple of 8 up to here


def _check_image_conv3d(who, cin, cout):
    """the refusals of the image-side conv, raised before any launch (and before the device check)"""
    if cin > IMAGE_NC_MAX:
        raise NotImplementedError(f"{who} input_nc {cin} is not supported: the first-layer kernels take up to {IMAGE_NC_MAX} image channels")
    if cout % 8 != 0 or cout > NDF_MAX or cout < 8:
        raise NotImplementedError(f"{who} needs a first layer (ndf) of a multiple of 8 and at most {NDF_MAX} output channels, got {cout}")


def _slices(N, size):
    """(N*D, H, W): the leading dimensions of the 16-bit tensor [N*D,H,W,C] that holds N images (H,W) or volumes (D,H,W)"""
    return (N * math.prod(size[:-2]), size[-2], size[-1])


class _DiscriminatorPlan(ParamIndex):
    """The stage walk.  A subclass names the leaf classes (conv_cls, norm_clss, inorm_cls), the geometry builders of a middle conv
    and of its stride-1 data gradient (taking N, *spatial size, Cin, Cout, k, ...), the weight view its pack needs (pack_view), the
    refusal text of a middle stage (mid_msg), and the hooks below `# ---- hooks`."""
    pack_view = None

    def __init__(self, net, dtype=None, seq="model"):
        """seq: the attribute of `net` that holds the reference's Sequential: `model` (NLayerDiscriminator, networks.py:661) or
        `net` (PixelDiscriminator, :693 -- the same conv / norm / LeakyReLU stages with 1x1 kernels, so the same plan)"""
        self.net = net
        self.seq = seq
        self.dtype, self.tdt = compute_dtype(dtype)
        self.packs = _PackCache()
        self.trust_versions = False      # see engine_common.pack_reuse_allowed
        self.grad_ready_hook = self.after_backward = self.grad_fetch = None      # parallel.GradReducer.attach

    def run(self, x):
        params = self.param_list()
        need_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        return _DiscriminatorFunction.apply(self, self.net.training, need_grad, x, *params)

    def layout(self):
        """(index in the Sequential, conv, the norm behind it or None) per conv"""
        seq = list(getattr(self.net, self.seq))
        stages = []
        for i, m in enumerate(seq):
            if isinstance(m, self.conv_cls):
                nxt = seq[i + 1] if i + 1 < len(seq) else None
                stages.append((i, m, nxt if isinstance(nxt, self.norm_clss) else None))
        return stages

    # ---- hooks ------------------------------------------------------------------------------------------
    @staticmethod
    def ksp(conv):
        return conv.kernel_size[0], conv.stride[0], conv.padding[0]

    def check_input(self, x, conv0):
        """the refusals of the input's rank and of the image-side conv (before the device check)"""
        raise NotImplementedError

    def check_head(self, conv):
        pass

    def check_stage_size(self, size, name, osize):
        pass

    # image_fwd(x, conv, z, k, s, p): z = leaky(conv(x) + bias) from the fp32 input; image_wgrad(x, dy, conv, k, s, p, inv_s) -> dw;
    # image_dgrad(dy, conv, x, k, s, p, inv_s) -> dx; head_fwd(x, conv, logits, k, s, p); head_bwd(x, conv, dl, dz, dw, k, s, p,
    # inv_s) -> db (or None); strided_dgrad(rec, dy, dz, N): the data gradient of a middle conv of stride 2 into dz

    # ---- forward ----------------------------------------------------------------------------------------
    def forward(self, x, training, need_grad):
        stages = self.layout()
        self.check_input(x, stages[0][1])
        _need_cuda(x)
        tdt = self.tdt
        dev = x.device
        x = x.contiguous().float()
        N, size = x.shape[0], tuple(x.shape[2:])
        sq = self.seq
        self.check_head(stages[-1][1])
        if not pack_reuse_allowed(need_grad, self.trust_versions):
            self.packs.clear()       # training forwards always re-pack: `.data` writes (Betty) bump no version counter

        def empty(*shape, dtype=tdt):
            return torch.empty(shape, dtype=dtype, device=dev)

        # InstanceNorm needs planes / volumes of more than one element (16 x 16 through three layers ends at 1 x 1): refused before
        # any launch, as is what check_stage_size refuses
        cur = size
        for (i, conv, bn) in stages:
            k, s, p = self.ksp(conv)
            cur = tuple(ops.conv_out_size(v, k, s, p) for v in cur)
            self.check_stage_size(size, f"{sq}.{i}", cur)
            if isinstance(bn, self.inorm_cls) and math.prod(cur) < 2:
                raise ValueError(f"Expected more than 1 spatial element when training, got input size "
                                 f"{[N, conv.out_channels, *cur]} ({self.inorm_cls.__name__} {sq}.{i + 1})")
        recs = []
        nbt_pending = []
        # stage 0: the conv on the fp32 input + bias + LeakyReLU (no norm)
        i0, conv0, _ = stages[0]
        k, s, p = self.ksp(conv0)
        size = tuple(ops.conv_out_size(v, k, s, p) for v in size)
        z = empty(*_slices(N, size), conv0.out_channels)
        self.image_fwd(x, conv0, z, k, s, p)
        recs.append(dict(kind="first", conv=conv0, x=x, z=z, k=k, s=s, p=p, name=f"{sq}.{i0}"))
        cur, cc = z, conv0.out_channels
        for (i, conv, bn) in stages[1:-1]:
            k, s, p = self.ksp(conv)
            inorm = isinstance(bn, self.inorm_cls)
            if bn is None or (conv.bias is not None and not inorm):
                raise NotImplementedError(self.mid_msg)
            cout = conv.out_channels
            wf, wd = self.packs.get(("conv", i), _ver(conv.weight), lambda conv=conv: pack_conv(conv.weight, tdt, view=self.pack_view))
            g = cached_geom(self.geom_conv, N, *size, cc, cout, k, s, p)
            osize = tuple(ops.conv_out_size(v, k, s, p) for v in size)
            y = empty(*_slices(N, osize), cout)
            z = empty(*_slices(N, osize), cout)
            rec = dict(kind="mid", conv=conv, bn=bn, inp=cur, y=y, geom=g, wd=wd, k=k, s=s, p=p, isize=size, cin=cc,
                       name=f"{sq}.{i}", bnname=f"{sq}.{i + 1}")
            if inorm:
                ops.conv_igemm(g, cur, wf, y, None, None)            # the conv's bias cancels in the norm: not added
                yv = per_sample(y, N)                                # per (sample, channel) over the whole plane / volume
                mi = instance_stats(yv, bn)
                ops.in_act_apply(yv, mi[0], mi[1], ACT_LEAKY02, z, cout, 0)
                rec.update(coef=None, stats=True, inorm=mi)
            else:
                mt = ops.conv_igemm_mtiles(g)
                use_stats = training or bn.running_mean is None
                part = empty(ops.bn_partials_numel(mt, cout), dtype=torch.float32) if use_stats else None
                ops.conv_igemm(g, cur, wf, y, None, part)
                coef, stats = bn_coeffs(bn, part, mt, cout, y.shape[0] * y.shape[1] * y.shape[2], training, dev, nbt_pending)
                ops.bn_act_apply(y, coef[0], coef[1], ACT_LEAKY02, z, cout, 0)
                rec.update(coef=coef, stats=stats)
            recs.append(rec)
            cur, size, cc = z, osize, cout
        il, convl, _ = stages[-1]
        k, s, p = self.ksp(convl)
        logits = torch.empty((N, convl.out_channels, *(ops.conv_out_size(v, k, s, p) for v in size)), dtype=torch.float32, device=dev)
        self.head_fwd(cur, convl, logits, k, s, p)
        recs.append(dict(kind="last", conv=convl, inp=cur, k=k, s=s, p=p, name=f"{sq}.{il}"))
        _flush_nbt(nbt_pending)
        return logits, (dict(recs=recs, N=N, H=x.shape[-2], W=x.shape[-1]) if need_grad else None)

    # ---- backward ---------------------------------------------------------------------------------------
    def backward(self, ctx, dlogits, need_dx):
        tdt = self.tdt
        recs, N = ctx["recs"], ctx["N"]
        dev = dlogits.device
        S = grad_scale(max(dlogits.numel(), 1))
        inv_s = 1.0 / S
        from ..parallel import GradEmitter
        emitter = GradEmitter(self.grad_ready_hook)          # data parallel: announced as soon as final
        grads = _EmitDict(emitter)

        def empty(*shape, dtype=tdt):
            return torch.empty(shape, dtype=dtype, device=dev)

        last = recs[-1]
        conv = last["conv"]
        dl = dlogits.contiguous().float() * S
        dw = torch.zeros_like(conv.weight, memory_format=torch.contiguous_format)
        dz = empty(*last["inp"].shape)
        db = self.head_bwd(last["inp"], conv, dl, dz, dw, last["k"], last["s"], last["p"], inv_s)
        grads[last["name"] + ".weight"] = dw
        if conv.bias is not None:
            grads[last["name"] + ".bias"] = db
        for rec in reversed(recs[1:-1]):
            conv = rec["conv"]
            k, s, p, cin, isize = rec["k"], rec["s"], rec["p"], rec["cin"], rec["isize"]
            cout = rec["y"].shape[3]
            dy, dgamma, dbeta = norm_act_bwd(rec["y"], rec["coef"], rec.get("inorm"), rec["stats"], dz, cout, 0, ACT_LEAKY02, inv_s, N)
            if dgamma is not None:
                grads[rec["bnname"] + ".weight"] = dgamma
                grads[rec["bnname"] + ".bias"] = dbeta
            grads[rec["name"] + ".weight"] = conv_wgrad(rec["geom"], rec["inp"], dy, conv.weight, cout, cin, rec["wd"].shape[0], inv_s)
            dz = empty(*_slices(N, isize), cin)
            if s == 1:
                ops.conv_igemm(cached_geom(self.geom_dgrad_s1, N, *isize, cin, cout, k, p), dy, rec["wd"], dz)
            else:
                self.strided_dgrad(rec, dy, dz, N)
            if conv.bias is not None:                                # (InstanceNorm only) cancelled by the norm: exact zeros
                grads[rec["name"] + ".bias"] = torch.zeros_like(conv.bias)
        first = recs[0]
        conv = first["conv"]
        z = first["z"]
        nd, oh, ow, c0 = z.shape
        # z = leaky(conv + bias): the activation gradient only needs the sign, which z preserves
        dy = norm_act_bwd(z, None, None, False, dz, c0, 0, ACT_LEAKY02, inv_s, N)[0]
        grads[first["name"] + ".weight"] = self.image_wgrad(first["x"], dy, conv, first["k"], first["s"], first["p"], inv_s)
        if conv.bias is not None:
            ws = empty(1024 * c0, dtype=torch.float32)
            db = empty(c0, dtype=torch.float32)
            ops.colsum(dy, c0, 0, nd, oh, ow, 0, 0, oh, ow, c0, inv_s, ws, db)
            grads[first["name"] + ".bias"] = db
        dx = None
        if need_dx:
            dx = self.image_dgrad(dy, conv, first["x"], first["k"], first["s"], first["p"], inv_s)
        if self.after_backward is not None:
            self.after_backward()
        return emitter.grads, dx


class DiscriminatorEngine(_DiscriminatorPlan):
    conv_cls, norm_clss, inorm_cls = torch.nn.Conv2d, (torch.nn.BatchNorm2d, torch.nn.InstanceNorm2d), torch.nn.InstanceNorm2d
    geom_conv, geom_dgrad_s1 = staticmethod(ops.geom_conv), staticmethod(ops.geom_conv_dgrad_s1)
    mid_msg = ("PatchGAN middle convs are expected as conv(no bias) -> BatchNorm -> LeakyReLU or "
               "conv -> InstanceNorm -> LeakyReLU")
    image_wgrad, image_dgrad = staticmethod(image_conv_wgrad), staticmethod(image_conv_dgrad)

    def check_input(self, x, conv0):
        if x.dim() != 4:
            raise ValueError(f"a 2-D discriminator takes an image batch [N,C,H,W], got a {x.dim()}-D tensor {tuple(x.shape)} "
                             "(volumes: define_D(..., threed=True))")
        _check_image_conv("discriminator", x.shape[1], conv0.out_channels)

    @staticmethod
    def image_fwd(x, conv, z, k, s, p):
        image_conv_fwd(x, conv, z, k, s, p, ACT_LEAKY02)

    @staticmethod
    def head_fwd(x, conv, logits, k, s, p):
        ops.conv_smallcout_fwd(x, conv.weight.detach().contiguous(), conv.bias.detach() if conv.bias is not None else None,
                               logits, k, s, p)

    @staticmethod
    def head_bwd(x, conv, dl, dz, dw, k, s, p, inv_s):
        db = torch.zeros_like(conv.bias) if conv.bias is not None else None
        ops.conv_smallcout_bwd(x, conv.weight.detach().contiguous(), dl, dz, dw, db, k, s, p, inv_s)
        return db

    @staticmethod
    def strided_dgrad(rec, dy, dz, N):
        conv_s2_dgrad(dy, rec["wd"], dz, rec["k"], rec["p"])


def _ksp3d(conv):
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    if len(set(k)) != 1 or len(set(s)) != 1 or len(set(p)) != 1:
        raise NotImplementedError("the 3-D discriminator plan takes cubic kernels, strides and pads")
    return k[0], s[0], p[0]


class Discriminator3DEngine(_DiscriminatorPlan):
    conv_cls, norm_clss, inorm_cls = torch.nn.Conv3d, (torch.nn.BatchNorm3d, torch.nn.InstanceNorm3d), torch.nn.InstanceNorm3d
    geom_conv, geom_dgrad_s1 = staticmethod(ops.geom_conv3d), staticmethod(ops.geom_conv3d_dgrad_s1)
    # [Cout][Cin][k][k][k] -> the engine's packs [k^3][Cout][Cin] / [k^3][Cin][Cout]; slot (kz*k + ky)*k + kx is the tensor's own tap
    # order, so gs_pack_weight takes the [Cout][Cin][k*k][k] view unchanged
    pack_view = staticmethod(ops.conv3d_weight_view)
    mid_msg = ("the 3-D discriminators' middle convs are expected as conv(no bias) -> BatchNorm3d -> LeakyReLU "
               "or conv -> InstanceNorm3d -> LeakyReLU")
    ksp = staticmethod(_ksp3d)

    def check_input(self, x, conv0):
        if x.dim() != 5:
            raise ValueError(f"a 3-D discriminator takes a volume [N,C,D,H,W], got a {x.dim()}-D tensor {tuple(x.shape)}")
        _check_image_conv3d("3-D discriminator", x.shape[1], conv0.out_channels)

    def check_head(self, conv):
        if conv.out_channels != 1 or _ksp3d(conv)[1] != 1:
            raise NotImplementedError("the 3-D discriminator's last conv is expected as Conv3d(C, 1, k, stride 1)")

    def check_stage_size(self, size, name, osize):
        """every stage must leave a voxel"""
        if min(osize) < 1:
            raise ValueError(f"input volume {list(size)} is too small: {name} would have the output size {list(osize)}")

    @staticmethod
    def image_fwd(x, conv, z, k, s, p):
        ops.conv3d_img_fwd(x, conv.weight.detach().contiguous(), _bias32(conv), z, k, s, p, ACT_LEAKY02)

    @staticmethod
    def image_wgrad(x, dy, conv, k, s, p, inv_s):
        dw = torch.empty_like(conv.weight, memory_format=torch.contiguous_format)
        ops.conv3d_img_wgrad(x, dy, dw, k, s, p, inv_s)
        return dw

    @staticmethod
    def image_dgrad(dy, conv, x, k, s, p, inv_s):
        dx = torch.empty_like(x)
        ops.conv3d_img_dgrad(dy, conv.weight.detach().contiguous(), dx, k, s, p, inv_s)
        return dx

    @staticmethod
    def head_fwd(x, conv, logits, k, s, p):
        ops.conv3d_head_fwd(x, conv.weight.detach().contiguous(), _bias32(conv), logits, k, p)

    @staticmethod
    def head_bwd(x, conv, dl, dz, dw, k, s, p, inv_s):
        db = torch.zeros(1, dtype=torch.float32, device=dl.device)          # (the kernel always writes it)
        ops.conv3d_head_bwd(x, conv.weight.detach().contiguous(), dl, dz, dw, db, k, p, inv_s)
        return db

    @staticmethod
    def strided_dgrad(rec, dy, dz, N):
        if rec["s"] != 2:
            raise NotImplementedError("middle convs of stride 1 or 2")
        gds = [cached_geom(ops.geom_conv3d_s2_dgrad_class, N, *rec["isize"], rec["cin"], dy.shape[3], rec["k"], rec["p"],
                           cls >> 2, (cls >> 1) & 1, cls & 1) for cls in range(8)]
        # gs_conv_igemm_batch takes four GEMMs of up to 16 taps: the eight 8-tap classes are two launches
        ops.conv_igemm_batch(gds[:4], dy, [rec["wd"]] * 4, dz)
        ops.conv_igemm_batch(gds[4:], dy, [rec["wd"]] * 4, dz)


class _DiscriminatorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, training, need_grad, x, *plist):
        logits, ectx = engine.forward(x, training, need_grad)
        ctx.engine, ctx.ectx, ctx.plist = engine, ectx, plist
        ctx.x_needs_grad = x.requires_grad
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        if ctx.ectx is None:
            raise RuntimeError("NLayerDiscriminator forward ran without gradient tracking")
        grads, dx = ctx.engine.backward(ctx.ectx, dlogits, ctx.x_needs_grad)
        return (None, None, None, dx, *param_grads(ctx.engine, grads, ctx.plist))
