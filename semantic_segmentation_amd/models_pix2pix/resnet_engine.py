"""Whole-network plan of the ResNet generator (`--netG resnet_9blocks` / `resnet_6blocks`; reference
models_pix2pix/networks.py:321-439) on the HIP kernels, forward and backward.

  stem   : ReflectionPad2d(3) of the fp32 NCHW image (gs_reflect_pad_image) -> direct 7x7 conv (gs_conv_ends_to_c16, pad 0: weights
           tiled through LDS, any ngf % 8 == 0) -> norm + ReLU.
  down   : two Conv2d(3, stride 2, padding 1) on the MFMA implicit GEMM (zero padding: the existing geometry), norm + ReLU.
  blocks : every 3x3 conv of a ResnetBlock sits behind ReflectionPad2d(1).  The pass that applies the norm of the conv in front
           (gs_reflect_norm_apply) writes its result INTO a tensor padded by one pixel, interior and reflected border together, so
           the conv is a pad-0 MFMA conv on a dense tensor.  Block b's input lives in the interior of P_b, the padded input of its
           first conv; `out = x + conv_block(x)` (:438) is the `res` operand of the pass behind the second conv, which writes P_{b+1}
           (the last block writes dense).  No stand-alone pad pass and no stand-alone add pass.
  up     : two ConvTranspose2d(3, 2, 1, output_padding=1) as four sub-pixel classes of 1 / 2 / 2 / 4 taps in one
           gs_conv_igemm_batch; the second one's norm + ReLU pass writes the tensor padded by 3 for the head.
  head   : direct 7x7 conv (gs_conv_ends_to_img, pad 0) + bias -> fp32 NCHW, gs_tanh_fwd in place.
Backward: the data gradient of a pad-0 conv is a gradient w.r.t. the PADDED tensor; gs_reflect_fold_add folds its border onto the
interior and adds the residual stream's gradient in the same pass (d out_b = fold(d P_{b+1}) + d out_{b+1}); the norm backward is
the existing gs_bn_act_bwd_* / gs_in_act_bwd.  Weight gradients go through the deterministic slab path; no atomics anywhere, so two
runs give equal bits.  Gradients are carried multiplied by a power-of-two scale (see unet_engine.py).
A conv bias directly in front of an InstanceNorm cancels: it is not added and its gradient is exact zeros (pix2pix_engine.py)."""
from __future__ import annotations

import torch

from .. import ops
from .._lib import ACT_NONE, ACT_RELU
from ..engine_common import ParamIndex, _flush_nbt, bn_coeffs, compute_dtype, pack_reuse_allowed
from .pix2pix_engine import (_PackCache, _need_cuda, _ver, cached_geom, conv_s2_dgrad, conv_wgrad, dropout_keep, grad_scale,
                             instance_stats, is_instance_norm, norm_act_bwd, pack_conv, param_grads)

PAD_MSG = "Padding size should be less than the corresponding input dimension"


def check_supported(input_nc, output_nc, ngf, norm_layer, padding_type):
    """the constructor's refusals (NotImplementedError naming what is supported); returns use_bias"""
    import functools
    if padding_type != 'reflect':
        raise NotImplementedError("ResnetGenerator padding_type [%s] is not on the MI355X hot path: 'reflect' (what define_G "
                                  "builds) is supported" % padding_type)
    func = norm_layer.func if type(norm_layer) == functools.partial else norm_layer
    if func not in (torch.nn.BatchNorm2d, torch.nn.InstanceNorm2d):
        raise NotImplementedError("ResnetGenerator norm layer is not on the MI355X hot path: norm='batch' (BatchNorm2d) and "
                                  "norm='instance' (InstanceNorm2d) are supported, norm='none' is not")
    if not 1 <= input_nc <= 4 or not 1 <= output_nc <= 4:
        raise NotImplementedError("ResnetGenerator input_nc / output_nc above 4 are not supported by the direct 7x7 kernels "
                                  "(1..4 channels)")
    if ngf < 8 or ngf % 8:
        raise NotImplementedError("ResnetGenerator ngf=%d: ngf must be a multiple of 8 (16-byte channel chunks)" % ngf)
    from .networks import _uses_instance_norm
    return _uses_instance_norm(norm_layer)


class ResnetGeneratorEngine(ParamIndex):
    def __init__(self, net, dtype=None):
        self.net = net
        self.dtype, self.tdt = compute_dtype(dtype)
        self.packs = _PackCache()
        self.trust_versions = False      # see engine_common.pack_reuse_allowed
        self.grad_ready_hook = self.after_backward = self.grad_fetch = None      # parallel.GradReducer.attach

    def layout(self):
        """(stem, downs, blocks, ups, head) as (name, conv, norm) triples; a block is (name, conv1, norm1, drop, conv2, norm2)"""
        seq = list(self.net.model)
        nb = sum(1 for m in seq if m.__class__.__name__ == "ResnetBlock")
        stem = ("model.1", seq[1], seq[2])
        downs = [("model.%d" % i, seq[i], seq[i + 1]) for i in (4, 7)]
        blocks = []
        for b in range(nb):
            cb = list(seq[10 + b].conv_block)
            drop = cb[4] if isinstance(cb[4], torch.nn.Dropout) else None
            j = 6 if drop is not None else 5
            blocks.append(("model.%d.conv_block" % (10 + b), cb[1], cb[2], drop, cb[j], cb[j + 1], j))
        ups = [("model.%d" % i, seq[i], seq[i + 1]) for i in (10 + nb, 13 + nb)]
        head = ("model.%d" % (17 + nb), seq[17 + nb], None)
        return stem, downs, blocks, ups, head

    def run(self, x, dropout_masks=None):
        params = self.param_list()
        need_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        return _ResnetGeneratorFunction.apply(self, self.net.training, need_grad, dropout_masks, x, *params)

    def _packs_of(self, name, conv, transposed=False):
        return self.packs.get(("conv", name), _ver(conv.weight), lambda: pack_conv(conv.weight, self.tdt, transposed))

    def invalidate_packs(self):
        self.packs.clear()

    @staticmethod
    def check_input(x):
        """refusals of an input size, before any launch.  (The pad check leaves every plane at 2 x 2 or more, so an InstanceNorm
        plane of fewer than two elements -- what DiscriminatorEngine.forward refuses -- cannot get past it.)"""
        N, _, H, W = x.shape
        if H % 4 or W % 4:
            raise ValueError("input size must be a multiple of 4 (two stride-2 convs and their transposed twins), got %d x %d" % (H, W))
        for size, pad in ((H, 3), (W, 3), (H // 4, 1), (W // 4, 1)):
            if size <= pad:
                raise ValueError("%s: pad %d at a dimension of %d (input %d x %d)" % (PAD_MSG, pad, size, H, W))

    # -------------------------------------------------------------------------------------------------
    def forward(self, x, training, need_grad, dropout_masks=None):
        stem, downs, blocks, ups, head = self.layout()
        N, cin0, H, W = x.shape
        self.check_input(x)                                          # (sizes are refused before any device work)
        _need_cuda(x)
        tdt, dev = self.tdt, x.device
        x = x.contiguous().float()
        if not pack_reuse_allowed(need_grad, self.trust_versions):
            self.packs.clear()       # training forwards always re-pack: `.data` writes (Betty) bump no version counter

        def empty(*shape, dtype=tdt):
            return torch.empty(shape, dtype=dtype, device=dev)

        nbt_pending = []

        def coefs(norm, y, part, mt):
            """the norm's coefficients from the conv output y (InstanceNorm: gs_in_stats) or the conv epilogue's partials"""
            n, h, w, C = y.shape
            if is_instance_norm(norm):
                mi = instance_stats(y, norm)
                return dict(kind=ops.NORM_INSTANCE, a=mi[0], b=mi[1], inorm=mi, coef=None, stats=True, norm=norm)
            coef, stats = bn_coeffs(norm, part, mt, C, n * h * w, training, dev, nbt_pending)
            return dict(kind=ops.NORM_BATCH, a=coef[0], b=coef[1], inorm=None, coef=coef, stats=stats, norm=norm)

        def partials(norm, mt, C):
            if is_instance_norm(norm) or not (training or norm.running_mean is None):
                return None
            return empty(ops.bn_partials_numel(mt, C), dtype=torch.float32)

        def apply(nc, y, act, pad, res=None, res_pad=0, keep=None, kscale=1.0):
            n, h, w, C = y.shape
            z = empty(n, h + 2 * pad, w + 2 * pad, C)
            ops.reflect_norm_apply(y, nc["a"], nc["b"], nc["kind"], act, z, pad, res, res_pad, keep, kscale)
            return z

        # ---- stem ----------------------------------------------------------------------------------------
        name, conv, norm = stem
        ngf = conv.out_channels
        xp = empty(N, cin0, H + 6, W + 6, dtype=torch.float32)
        ops.reflect_pad_image(x, xp, 3)
        y = empty(N, H, W, ngf)
        mt = ops.conv_ends_mtiles(N, H, W)
        part = partials(norm, mt, ngf)
        ops.conv_ends_to_c16(xp, conv.weight.detach().contiguous(), y, part)
        nc = coefs(norm, y, part, mt)
        cur = apply(nc, y, ACT_RELU, 0)
        ctx = dict(N=N, H=H, W=W, x=x, xp=xp, training=training,
                   stem=dict(name=name, conv=conv, y=y, nc=nc, z=cur), downs=[], blocks=[], ups=[])
        # ---- down ----------------------------------------------------------------------------------------
        ch, cw, cc = H, W, ngf
        for i, (name, conv, norm) in enumerate(downs):
            wf, wd = self._packs_of(name, conv)
            g = cached_geom(ops.geom_conv, N, ch, cw, cc, conv.out_channels, 3, 2, 1)
            y = empty(N, g.OH, g.OW, conv.out_channels)
            mt = ops.conv_igemm_mtiles(g)
            part = partials(norm, mt, conv.out_channels)
            ops.conv_igemm(g, cur, wf, y, None, part)                # (a bias in front of an InstanceNorm cancels: not added)
            nc = coefs(norm, y, part, mt)
            z = apply(nc, y, ACT_RELU, 1 if i == 1 and blocks else 0)    # the second one writes P_0, padded for the first block
            ctx["downs"].append(dict(name=name, conv=conv, inp=cur, y=y, nc=nc, geom=g, wd=wd, ih=ch, iw=cw, cin=cc, z=z))
            cur, ch, cw, cc = z, g.OH, g.OW, conv.out_channels
        # ---- blocks --------------------------------------------------------------------------------------
        h, w, C = ch, cw, cc
        P = cur                                                      # [N,h+2,w+2,C]: block input in the interior
        if blocks:
            g3 = cached_geom(ops.geom_conv, N, h + 2, w + 2, C, C, 3, 1, 0)
            mt3 = ops.conv_igemm_mtiles(g3)
        for b, (name, conv1, norm1, drop, conv2, norm2, j2) in enumerate(blocks):
            wf1, wd1 = self._packs_of(name + ".1", conv1)
            wf2, wd2 = self._packs_of(name + ".%d" % j2, conv2)
            y1 = empty(N, h, w, C)
            part = partials(norm1, mt3, C)
            ops.conv_igemm(g3, P, wf1, y1, None, part)
            n1 = coefs(norm1, y1, part, mt3)
            keep, kscale = dropout_keep(drop, training, dropout_masks, b, N, h, w, C, dev)
            Q = apply(n1, y1, ACT_RELU, 1, keep=keep, kscale=kscale)
            y2 = empty(N, h, w, C)
            part = partials(norm2, mt3, C)
            ops.conv_igemm(g3, Q, wf2, y2, None, part)
            n2 = coefs(norm2, y2, part, mt3)
            last = b == len(blocks) - 1
            Pn = apply(n2, y2, ACT_NONE, 0 if last else 1, res=P, res_pad=1)
            ctx["blocks"].append(dict(name=name, j2=j2, conv1=conv1, conv2=conv2, P=P, y1=y1, n1=n1, keep=keep, kscale=kscale,
                                      Q=Q, y2=y2, n2=n2, wd1=wd1, wd2=wd2, geom=g3, out=Pn))
            P = Pn
        cur = P
        # ---- up ------------------------------------------------------------------------------------------
        for i, (name, conv, norm) in enumerate(ups):
            cout = conv.out_channels
            wf, wd = self._packs_of(name, conv, transposed=True)
            geoms = [cached_geom(ops.geom_convT3_class, N, ch, cw, cc, cout, cls >> 1, cls & 1) for cls in range(4)]
            mts = [ops.conv_igemm_mtiles(g) for g in geoms]          # (the classes' tap counts differ, and so may their tile rows)
            y = empty(N, 2 * ch, 2 * cw, cout)
            part = partials(norm, sum(mts) + max(mts), cout)         # class after class; room for the last slice's scratch
            pslices = [part[sum(mts[:cls]) * 2 * cout:] for cls in range(4)] if part is not None else None
            ops.conv_igemm_batch(geoms, cur, [wf] * 4, y, None, pslices)
            nc = coefs(norm, y, part, sum(mts))
            z = apply(nc, y, ACT_RELU, 3 if i == 1 else 0)           # the second one writes the head's input, padded by 3
            ctx["ups"].append(dict(name=name, conv=conv, inp=cur, y=y, nc=nc, wd=wd, ih=ch, iw=cw, cin=cc, z=z))
            cur, ch, cw, cc = z, 2 * ch, 2 * cw, cout
        # ---- head ----------------------------------------------------------------------------------------
        name, conv, _ = head
        out = torch.empty((N, conv.out_channels, H, W), dtype=torch.float32, device=dev)
        ops.conv_ends_to_img(cur, conv.weight.detach().contiguous(), conv.bias.detach() if conv.bias is not None else None, out)
        ops.tanh_fwd(out, out)
        ctx["head"] = dict(name=name, conv=conv, inp=cur)
        ctx["t"] = out
        _flush_nbt(nbt_pending)
        return out, (ctx if need_grad else None)


def resnet_generator_backward(engine, ctx, dout, need_dx):
    """(grads by parameter name, dx or None) from the state engine.forward saved: the launches listed in DESIGN.md"""
    tdt = engine.tdt
    N, H, W = ctx["N"], ctx["H"], ctx["W"]
    dev = dout.device
    S = grad_scale(N * H * W)
    inv_s = 1.0 / S
    from ..parallel import GradEmitter
    emitter = GradEmitter(getattr(engine, "grad_ready_hook", None))     # data parallel: announced as soon as final

    def empty(*shape, dtype=tdt):
        return torch.empty(shape, dtype=dtype, device=dev)

    def emit(name, g):
        emitter.emit(name, g)

    def norm_bwd(y, nc, name, dz, act, keep=None, kscale=1.0):
        """gradient w.r.t. the conv output y of act(norm(y)) [* keep]; emits the BatchNorm parameters' gradients under `name`"""
        dy, dgamma, dbeta = norm_act_bwd(y, nc["coef"], nc["inorm"], nc["stats"], dz, y.shape[3], 0, act, inv_s, N,
                                         keep=keep, kscale=kscale)
        if dgamma is not None:
            emit(name + ".weight", dgamma)
            emit(name + ".bias", dbeta)
        return dy

    def cancelled_bias(name, conv):
        if conv.bias is not None:                                    # in front of an InstanceNorm: exact zeros
            emit(name + ".bias", torch.zeros_like(conv.bias))

    def wgrad(g, x, dy, name, conv, A, B):
        emit(name + ".weight", conv_wgrad(g, x, dy, conv.weight, A, B, 9, inv_s))

    def seq_name(name, off):
        head, _, idx = name.rpartition(".")
        return "%s.%d" % (head, int(idx) + off)

    # ---- head: out = tanh(conv(T) + bias) ------------------------------------------------------------------
    hd = ctx["head"]
    conv = hd["conv"]
    d = torch.empty_like(ctx["t"])
    ops.tanh_bwd(ctx["t"], dout.contiguous().float(), S, d)
    dw = torch.empty_like(conv.weight, memory_format=torch.contiguous_format)
    db = torch.empty_like(conv.bias) if conv.bias is not None else None
    dT = empty(*hd["inp"].shape)                                     # the gradient w.r.t. the PADDED head input: full correlation
    ops.conv_ends_to_c16(d, conv.weight.detach().contiguous(), dT, None, pad=6, flip=True, w_img_major=True)
    ops.conv_ends_wgrad(hd["inp"], d, dw, db, pad=6, flip=True, w_img_major=True, gscale=inv_s)
    emit(hd["name"] + ".weight", dw)
    if db is not None:
        emit(hd["name"] + ".bias", db)
    # ---- up ----------------------------------------------------------------------------------------------
    dz = None
    for i in (1, 0):
        rec = ctx["ups"][i]
        conv, y = rec["conv"], rec["y"]
        cout = conv.out_channels
        if i == 1:                                                   # its output feeds the head through ReflectionPad2d(3)
            dz = empty(*y.shape)
            ops.reflect_fold_add(dT, dz, 3)
        dy = norm_bwd(y, rec["nc"], seq_name(rec["name"], 1), dz, ACT_RELU)
        # seen from its output side a transposed conv is Conv2d(3, stride 2, padding 1): its data gradient IS that conv, and its
        # weight gradient is that conv's with the roles of input and output exchanged ([Cin][Cout][3][3], the reference layout)
        g = cached_geom(ops.geom_conv, N, 2 * rec["ih"], 2 * rec["iw"], cout, rec["cin"], 3, 2, 1)
        wgrad(g, dy, rec["inp"], rec["name"], conv, rec["cin"], cout)
        cancelled_bias(rec["name"], conv)
        dz = empty(N, rec["ih"], rec["iw"], rec["cin"])
        ops.conv_igemm(g, dy, rec["wd"], dz)
    # ---- blocks, last first: dz = d out_b ----------------------------------------------------------------
    for rec in reversed(ctx["blocks"]):
        name, g3 = rec["name"], rec["geom"]
        n_, h, w, C = rec["y2"].shape
        gd = cached_geom(ops.geom_conv_dgrad_s1, N, h + 2, w + 2, C, C, 3, 0)
        dy2 = norm_bwd(rec["y2"], rec["n2"], "%s.%d" % (name, rec["j2"] + 1), dz, ACT_NONE)
        wgrad(g3, rec["Q"], dy2, "%s.%d" % (name, rec["j2"]), rec["conv2"], C, C)
        cancelled_bias("%s.%d" % (name, rec["j2"]), rec["conv2"])
        dQ = empty(N, h + 2, w + 2, C)
        ops.conv_igemm(gd, dy2, rec["wd2"], dQ)
        dq = empty(N, h, w, C)
        ops.reflect_fold_add(dQ, dq, 1)
        dy1 = norm_bwd(rec["y1"], rec["n1"], name + ".2", dq, ACT_RELU, rec["keep"], rec["kscale"])
        wgrad(g3, rec["P"], dy1, name + ".1", rec["conv1"], C, C)
        cancelled_bias(name + ".1", rec["conv1"])
        dP = dQ                                                      # (dQ is dead: its fold is taken)
        ops.conv_igemm(gd, dy1, rec["wd1"], dP)
        dx_b = empty(N, h, w, C)
        ops.reflect_fold_add(dP, dx_b, 1, add=dz)                    # both routes to the block's input in one pass
        dz = dx_b
    # ---- down ----------------------------------------------------------------------------------------------
    for rec in reversed(ctx["downs"]):
        conv, y = rec["conv"], rec["y"]
        cin, cout = rec["cin"], conv.out_channels
        dy = norm_bwd(y, rec["nc"], seq_name(rec["name"], 1), dz, ACT_RELU)
        wgrad(rec["geom"], rec["inp"], dy, rec["name"], conv, cout, cin)
        cancelled_bias(rec["name"], conv)
        dz = empty(N, rec["ih"], rec["iw"], cin)
        conv_s2_dgrad(dy, rec["wd"], dz, 3, 1)
    # ---- stem ----------------------------------------------------------------------------------------------
    st = ctx["stem"]
    conv = st["conv"]
    dy = norm_bwd(st["y"], st["nc"], seq_name(st["name"], 1), dz, ACT_RELU)
    dw = torch.empty_like(conv.weight, memory_format=torch.contiguous_format)
    ops.conv_ends_wgrad(dy, ctx["xp"], dw, None, gscale=inv_s)
    emit(st["name"] + ".weight", dw)
    cancelled_bias(st["name"], conv)
    dx = None
    if need_dx:
        dxp = torch.empty_like(ctx["xp"])
        ops.conv_ends_to_img(dy, conv.weight.detach().contiguous(), None, dxp, pad=6, flip=True, w_img_major=False, gscale=inv_s)
        dx = torch.empty_like(ctx["x"])
        ops.reflect_fold_image(dxp, dx, 3)
    if getattr(engine, "after_backward", None) is not None:
        engine.after_backward()
    return emitter.grads, dx


class _ResnetGeneratorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, training, need_grad, dropout_masks, x, *plist):
        out, ectx = engine.forward(x, training, need_grad, dropout_masks)
        ctx.engine, ctx.ectx, ctx.plist = engine, ectx, plist
        ctx.x_needs_grad = x.requires_grad
        if ectx is not None:
            ctx.save_for_backward(out)              # the tanh backward reads the image itself: autograd guards it against in-place edits
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.ectx is None:
            raise RuntimeError("ResnetGenerator forward ran without gradient tracking")
        ctx.saved_tensors                           # (raises if the image was modified in place)
        grads, dx = resnet_generator_backward(ctx.engine, ctx.ectx, dout, ctx.x_needs_grad)
        return (None, None, None, None, dx, *param_grads(ctx.engine, grads, ctx.plist))
