"""Whole-network plan of the 3-D Pix2Pix discriminators on the HIP kernels (reference: GenSeg-3D/models/networks.py:806-890 with a
3-D norm layer -- NLayerDiscriminator and PixelDiscriminator holding nn.Conv3d leaves; the netD of `--model pix2pix3d`,
GenSeg-3D/train_end2end.py:143-178).

A volume [N,C,D,H,W] lives as a stack of depth slices [N*D,H,W,C] in 16 bits, as in unet3d_engine.py.
  * the image-side conv (model.0 / net.0) reads the fp32 NCDHW volume directly: csrc/ends3d.hip gs_conv3d_img_fwd (+ bias + LeakyReLU);
  * every middle conv (k4 s2 p1, k4 s1 p1, or k1 in the pixel net) is ONE gs_conv_igemm launch with up to 64 depth-strided taps
    (ops.geom_conv3d); BatchNorm3d statistics come out of the conv epilogue (count N*OD*OH*OW), InstanceNorm3d statistics per
    (sample, channel) over the WHOLE volume from gs_in_stats on the [N, OD*OH, OW, C] view (csrc/instnorm.hip only uses H*W);
  * the one-channel head is the reduction kernel gs_conv3d_head_fwd (fp32 logits [N,1,OD,OH,OW]).
Backward: gs_conv3d_head_bwd; per middle stage the norm + LeakyReLU backward, the deterministic weight gradient straight into
[Cout][Cin][k][k][k] (gs_conv_wgrad_slabs + gs_wgrad_reduce_unpack) and the data gradient (stride 1: one 64-tap launch; stride 2: the
eight sub-voxel classes of eight taps in two batched launches of four); gs_conv3d_img_wgrad / gs_colsum / gs_conv3d_img_dgrad at the
image.  A middle conv's bias exists only under InstanceNorm3d, where it cancels in the norm: not added, gradient exact zeros.
The contract is DiscriminatorEngine's (pix2pix_engine.py): forward(x, training, need_grad) -> (logits, ctx), backward(ctx, dlogits,
need_dx) -> (grads, dx), gradients carried times a power-of-two scale, version-keyed weight packs, the data-parallel hooks."""
from __future__ import annotations

import math

import torch

from .. import ops
from .._lib import ACT_LEAKY02
from ..engine_common import ParamIndex, _flush_nbt, bn_coeffs, compute_dtype, pack_reuse_allowed
from .pix2pix_engine import IMAGE_NC_MAX, _DiscriminatorFunction, _EmitDict, _PackCache, _bias32, _need_cuda, _ver, cached_geom, instance_stats

NDF_MAX = 128               # output channels of the image-side kernels: any multiple of 8 up to here


def is_instance_norm3d(m):
    return isinstance(m, torch.nn.InstanceNorm3d)


def _check_image_conv3d(who, cin, cout):
    """the refusals of the image-side conv, raised before any launch (and before the device check)"""
    if cin > IMAGE_NC_MAX:
        raise NotImplementedError(f"{who} input_nc {cin} is not supported: the first-layer kernels take up to {IMAGE_NC_MAX} image channels")
    if cout % 8 != 0 or cout > NDF_MAX or cout < 8:
        raise NotImplementedError(f"{who} needs a first layer (ndf) of a multiple of 8 and at most {NDF_MAX} output channels, got {cout}")


def _ksp(conv):
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    if len(set(k)) != 1 or len(set(s)) != 1 or len(set(p)) != 1:
        raise NotImplementedError("the 3-D discriminator plan takes cubic kernels, strides and pads")
    return k[0], s[0], p[0]


def _nv(t, N):
    """[N*D,H,W,C] -> the [N, D*H, W, C] view the per-sample norm kernels take (a volume is one plane of D*H rows)"""
    ND, H, W, C = t.shape
    return t.view(N, (ND // N) * H, W, C)


class Discriminator3DEngine(ParamIndex):
    def __init__(self, net, dtype=None, seq="model"):
        """seq: the attribute of `net` that holds the reference's Sequential: `model` (NLayerDiscriminator) or `net` (PixelDiscriminator)"""
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
        seq = list(getattr(self.net, self.seq))
        stages = []
        for i, m in enumerate(seq):
            if isinstance(m, torch.nn.Conv3d):
                nxt = seq[i + 1] if i + 1 < len(seq) else None
                stages.append((i, m, nxt if isinstance(nxt, (torch.nn.BatchNorm3d, torch.nn.InstanceNorm3d)) else None))
        return stages

    def forward(self, x, training, need_grad):
        stages = self.layout()
        if x.dim() != 5:
            raise ValueError(f"a 3-D discriminator takes a volume [N,C,D,H,W], got a {x.dim()}-D tensor {tuple(x.shape)}")
        _check_image_conv3d("3-D discriminator", x.shape[1], stages[0][1].out_channels)
        _need_cuda(x)
        tdt = self.tdt
        dev = x.device
        x = x.contiguous().float()
        N, cin0, D, H, W = x.shape
        sq = self.seq
        convl = stages[-1][1]
        if convl.out_channels != 1 or _ksp(convl)[1] != 1:
            raise NotImplementedError("the 3-D discriminator's last conv is expected as Conv3d(C, 1, k, stride 1)")
        if not pack_reuse_allowed(need_grad, self.trust_versions):
            self.packs.clear()       # training forwards always re-pack: `.data` writes bump no version counter

        def empty(*shape, dtype=tdt):
            return torch.empty(shape, dtype=dtype, device=dev)

        # every stage must leave a voxel, and InstanceNorm needs volumes of more than one: refused before any launch
        cd, ch, cw = D, H, W
        for (i, conv, bn) in stages:
            k, s, p = _ksp(conv)
            cd, ch, cw = (ops.conv_out_size(v, k, s, p) for v in (cd, ch, cw))
            if min(cd, ch, cw) < 1:
                raise ValueError(f"input volume {[D, H, W]} is too small: {sq}.{i} would have the output size {[cd, ch, cw]}")
            if is_instance_norm3d(bn) and cd * ch * cw < 2:
                raise ValueError(f"Expected more than 1 spatial element when training, got input size "
                                 f"{[N, conv.out_channels, cd, ch, cw]} (InstanceNorm3d {sq}.{i + 1})")
        recs = []
        nbt_pending = []
        # stage 0: the conv on the fp32 volume + bias + LeakyReLU (no norm)
        i0, conv0, _ = stages[0]
        k, s, p = _ksp(conv0)
        cd, ch, cw = (ops.conv_out_size(v, k, s, p) for v in (D, H, W))
        z = empty(N * cd, ch, cw, conv0.out_channels)
        ops.conv3d_img_fwd(x, conv0.weight.detach().contiguous(), _bias32(conv0), z, k, s, p, ACT_LEAKY02)
        recs.append(dict(kind="first", conv=conv0, x=x, z=z, k=k, s=s, p=p, name=f"{sq}.{i0}"))
        cur, cc = z, conv0.out_channels
        for (i, conv, bn) in stages[1:-1]:
            k, s, p = _ksp(conv)
            inorm = is_instance_norm3d(bn)
            if bn is None or (conv.bias is not None and not inorm):
                raise NotImplementedError("the 3-D discriminators' middle convs are expected as conv(no bias) -> BatchNorm3d -> LeakyReLU "
                                          "or conv -> InstanceNorm3d -> LeakyReLU")
            cout = conv.out_channels
            wf, wd = self.packs.get(("conv", i), _ver(conv.weight), lambda conv=conv: self._pack(conv.weight))
            g = cached_geom(ops.geom_conv3d, N, cd, ch, cw, cc, cout, k, s, p)
            od, oh, ow = g.Dg, g.OH, g.OW
            y = empty(N * od, oh, ow, cout)
            z = empty(N * od, oh, ow, cout)
            rec = dict(kind="mid", conv=conv, bn=bn, inp=cur, y=y, geom=g, wd=wd, k=k, s=s, p=p, idd=cd, ih=ch, iw=cw, cin=cc,
                       name=f"{sq}.{i}", bnname=f"{sq}.{i + 1}")
            if inorm:
                ops.conv_igemm(g, cur, wf, y, None, None)            # the conv's bias cancels in the norm: not added
                mi = instance_stats(_nv(y, N), bn)                   # per (sample, channel) over the whole volume
                ops.in_act_apply(_nv(y, N), mi[0], mi[1], ACT_LEAKY02, z, cout, 0)
                rec.update(coef=None, stats=True, inorm=mi)
            else:
                mt = ops.conv_igemm_mtiles(g)
                use_stats = training or bn.running_mean is None
                part = empty(ops.bn_partials_numel(mt, cout), dtype=torch.float32) if use_stats else None
                ops.conv_igemm(g, cur, wf, y, None, part)
                coef, stats = bn_coeffs(bn, part, mt, cout, N * od * oh * ow, training, dev, nbt_pending)
                ops.bn_act_apply(y, coef[0], coef[1], ACT_LEAKY02, z, cout, 0)
                rec.update(coef=coef, stats=stats)
            recs.append(rec)
            cur, cd, ch, cw, cc = z, od, oh, ow, cout
        il = stages[-1][0]
        k, s, p = _ksp(convl)
        od, oh, ow = (ops.conv_out_size(v, k, s, p) for v in (cd, ch, cw))
        logits = torch.empty((N, 1, od, oh, ow), dtype=torch.float32, device=dev)
        ops.conv3d_head_fwd(cur, convl.weight.detach().contiguous(), _bias32(convl), logits, k, p)
        recs.append(dict(kind="last", conv=convl, inp=cur, k=k, s=s, p=p, name=f"{sq}.{il}"))
        _flush_nbt(nbt_pending)
        return logits, (dict(recs=recs, N=N) if need_grad else None)

    def _pack(self, w):
        """[Cout][Cin][k][k][k] -> the engine's packs [k^3][Cout][Cin] / [k^3][Cin][Cout]; slot (kz*k + ky)*k + kx is the tensor's own
        tap order, so gs_pack_weight takes the [Cout][Cin][k*k][k] view unchanged (ops.conv3d_weight_view)"""
        cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
        wf = torch.empty((k ** 3, cout, cin), dtype=self.tdt, device=w.device)
        wd = torch.empty((k ** 3, cin, cout), dtype=self.tdt, device=w.device)
        ops.pack_weight(ops.conv3d_weight_view(w.detach().contiguous()), wf, wd, False)
        return wf, wd

    @staticmethod
    def _mid_conv_bwd(rec, dy, N, grads, inv_s, empty):
        """weight gradient (emitted) and data gradient (returned) of a middle conv from dy"""
        conv = rec["conv"]
        cout = dy.shape[3]
        k, s, p, cin = rec["k"], rec["s"], rec["p"], rec["cin"]
        D, H, W = rec["idd"], rec["ih"], rec["iw"]
        dw = torch.empty_like(conv.weight, memory_format=torch.contiguous_format)
        wsl = empty(max(ops.conv_wgrad_ws_floats(rec["geom"]), 1), dtype=torch.float32)
        # K parts in slabs + ordered reduction fused with scale / unpack (one part: a plain store): deterministic
        ops.conv_wgrad_det(rec["geom"], rec["inp"], dy, wsl, dw, cout, cin, k ** 3, inv_s)
        grads[rec["name"] + ".weight"] = dw
        dz = empty(N * D, H, W, cin)
        if s == 1:
            ops.conv_igemm(cached_geom(ops.geom_conv3d_dgrad_s1, N, D, H, W, cin, cout, k, p), dy, rec["wd"], dz)
        elif s == 2:
            gds = [cached_geom(ops.geom_conv3d_s2_dgrad_class, N, D, H, W, cin, cout, k, p, cls >> 2, (cls >> 1) & 1, cls & 1)
                   for cls in range(8)]
            # gs_conv_igemm_batch takes four GEMMs of up to 16 taps: the eight 8-tap classes are two launches
            ops.conv_igemm_batch(gds[:4], dy, [rec["wd"]] * 4, dz)
            ops.conv_igemm_batch(gds[4:], dy, [rec["wd"]] * 4, dz)
        else:
            raise NotImplementedError("middle convs of stride 1 or 2")
        return dz

    def backward(self, ctx, dlogits, need_dx):
        tdt = self.tdt
        recs, N = ctx["recs"], ctx["N"]
        dev = dlogits.device
        S = float(2 ** round(math.log2(max(dlogits.numel(), 1))))
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
        db = torch.zeros(1, dtype=torch.float32, device=dev)
        dz = empty(*last["inp"].shape)
        ops.conv3d_head_bwd(last["inp"], conv.weight.detach().contiguous(), dl, dz, dw, db, last["k"], last["p"], inv_s)
        grads[last["name"] + ".weight"] = dw
        if conv.bias is not None:
            grads[last["name"] + ".bias"] = db
        for rec in reversed(recs[1:-1]):
            conv, coef = rec["conv"], rec["coef"]
            y = rec["y"]
            nd, oh, ow, cout = y.shape
            inorm = rec.get("inorm")
            dy = empty(nd, oh, ow, cout)
            if inorm is not None:
                yv = _nv(y, N)
                ops.in_act_bwd(yv, inorm[0], inorm[1], dz, cout, 0, ACT_LEAKY02, dy, empty(2, N, cout, dtype=torch.float32),
                               ops.in_workspace(N, yv.shape[1], ow, cout, dev))
                dz = self._mid_conv_bwd(rec, dy, N, grads, inv_s, empty)
                if conv.bias is not None:                            # cancelled by the norm: exact zeros
                    grads[rec["name"] + ".bias"] = torch.zeros_like(conv.bias)
                continue
            nt = ops.bn_bwd_tiles_used(nd, oh, ow, False)
            part = empty(ops.bn_partials_numel(ops.bn_bwd_tiles(nd, oh, ow), cout), dtype=torch.float32)
            ops.bn_act_bwd_reduce(y, dz, cout, 0, None, coef[0], coef[1], coef[2], coef[3], ACT_LEAKY02, part)
            dgamma = empty(cout, dtype=torch.float32)
            dbeta = empty(cout, dtype=torch.float32)
            c12 = empty(2, cout, dtype=torch.float32)
            ops.bn_bwd_coeffs(part, nt, cout, nd * oh * ow, inv_s, dgamma, dbeta, c12[0], c12[1])
            if not rec["stats"]:
                c12.zero_()
            ops.bn_act_bwd_apply(y, dz, cout, 0, None, coef[0], coef[1], coef[2], coef[3], c12[0], c12[1], ACT_LEAKY02, True, dy)
            grads[rec["bnname"] + ".weight"] = dgamma
            grads[rec["bnname"] + ".bias"] = dbeta
            dz = self._mid_conv_bwd(rec, dy, N, grads, inv_s, empty)
        first = recs[0]
        conv = first["conv"]
        z = first["z"]
        nd, oh, ow, c0 = z.shape
        dy = empty(nd, oh, ow, c0)
        # z = leaky(conv + bias): the activation gradient only needs the sign, which z preserves
        ops.bn_act_bwd_apply(z, dz, c0, 0, None, None, None, None, None, None, None, ACT_LEAKY02, False, dy)
        dw = torch.empty_like(conv.weight, memory_format=torch.contiguous_format)
        ops.conv3d_img_wgrad(first["x"], dy, dw, first["k"], first["s"], first["p"], inv_s)
        grads[first["name"] + ".weight"] = dw
        if conv.bias is not None:
            ws = empty(1024 * c0, dtype=torch.float32)
            db = empty(c0, dtype=torch.float32)
            ops.colsum(dy, c0, 0, nd, oh, ow, 0, 0, oh, ow, c0, inv_s, ws, db)
            grads[first["name"] + ".bias"] = db
        dx = None
        if need_dx:
            dx = torch.empty_like(first["x"])
            ops.conv3d_img_dgrad(dy, conv.weight.detach().contiguous(), dx, first["k"], first["s"], first["p"], inv_s)
        if self.after_backward is not None:
            self.after_backward()
        return emitter.grads, dx
