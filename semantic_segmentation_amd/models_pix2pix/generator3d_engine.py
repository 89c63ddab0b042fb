"""Whole-network plan of the 3-D Pix2Pix generator on the HIP kernels, forward and backward (reference:
GenSeg-3D/models/networks.py:604-728, `UnetGenerator` built from `LinearUpsampleUnetSkipConnectionBlock`s, upsampling='linear').

Plan code over the layout-level steps of cell3d_engine.py and the steps every Pix2Pix plan shares (pix2pix_engine.py); the one kernel
of its own is the image-side tail (csrc/gen3d.hip).  A volume is a stack of depth slices, 16-bit [N*D,H,W,C].  With `num_downs`
levels, c = [input_nc, ngf, 2 ngf, 4 ngf, 8 ngf, 8 ngf, ...] and level k at 1 / 2^k of the input size:
  down  cell k (block depth k-1, `layer_index` num_downs-k): gather -> merged pack -> one 64-tap conv over the gathered volume, y_k
        dense.  The outermost cell reads the fp32 image.  No norm behind cells 1 and num_downs (their bias, under InstanceNorm3d, is
        added); a bias in front of a norm cancels: not added, gradient exact zeros, no share in d conv_arch.
  norm  one pass per consumer under BatchNorm3d (count N*D*H*W, conv-epilogue partials; running statistics in eval), one pass for
        both under InstanceNorm3d (per (sample, channel) over the whole volume): L_k = leaky(norm(y_k)) feeds cell k+1,
        relu(norm(y_k)) is the first half of the level's concat buffer R_k -- the in-place LeakyReLU has changed the skip operand,
        and the parent's in-place ReLU then sees relu(leaky(x)) = relu(x), as in the 2-D plan.
  up    block depth d reads R_{d+1} (all 2 c channels; the innermost block relu(y) of its own cell): upsample_forward -> v_d dense,
        then Conv3d k3 / s1 / p1 on the generic engine (ops.geom_conv3d) -> u_d dense, norm (+ dropout keep mask x 2) + ReLU into
        the second half of R_d.  The up-conv's bias is always there and always in front of batch / instance statistics for d > 0:
        not added, gradient exact zeros (BatchNorm3d: folded into the running mean; on running statistics, in eval mode, it sits
        in the shift and its gradient is gs_colsum).  d = 0: the tail kernel, bias + tanh + fp32 NCDHW in one pass.
Backward mirrors pix2pix_backward.generator_backward: tail backward -> upsample_backward into dR_1 -> per level norm_act_bwd with
the two consumers, conv_wgrad + the 27-tap data gradient + upsample_backward on the way in, wgrad_split + dgrad per cell on the
way out; the outermost cell's data gradient runs only when the input requires grad.  Gradients are carried times a power of two."""
from __future__ import annotations

import functools

import torch

from .. import ops
from .._lib import ACT_LEAKY02, ACT_RELU, ACT_TANH
from ..engine_common import ParamIndex, _flush_nbt, bn_coeffs, compute_dtype, pack_reuse_allowed
from . import cell3d_engine as ce
from .pix2pix_engine import (_PackCache, _bias32, _ver, cached_geom, conv_wgrad, dropout_keep, grad_scale, instance_stats,
                             norm_act_bwd, pack_conv, param_grads, per_sample)

LIMITS = ("the 3-D linear-upsample U-Net generator on the HIP path: upsampling='linear', num_downs 5 or 6 (the reference's conv_arch has "
          "6 rows), ngf a multiple of 16 (the outermost upsample takes 2 ngf channels, a multiple of 32, and the tail ngf / 2, a "
          "multiple of 8), input_nc and output_nc 1..4, and a norm layer of get_norm_layer('batch' | 'instance', threed=True)")


def check_supported(input_nc, output_nc, num_downs, ngf, norm_layer, upsampling='linear'):
    """the refusals of construction (NotImplementedError naming the limits)"""
    got = f"; got input_nc={input_nc}, output_nc={output_nc}, num_downs={num_downs}, ngf={ngf}, upsampling={upsampling!r}"
    if upsampling != 'linear':
        raise NotImplementedError(LIMITS + got)
    if num_downs not in (5, 6) or ngf <= 0 or ngf % 16 or not 1 <= input_nc <= 4 or not 1 <= output_nc <= 4:
        raise NotImplementedError(LIMITS + got)
    func = norm_layer.func if type(norm_layer) == functools.partial else norm_layer
    if func not in (torch.nn.BatchNorm3d, torch.nn.InstanceNorm3d):
        raise NotImplementedError(LIMITS + f"; got norm layer {getattr(func, '__name__', func)!r}")
    probe = norm_layer(8)
    want = (True, True) if func is torch.nn.BatchNorm3d else (False, False)
    if (bool(probe.affine), bool(probe.track_running_stats)) != want:
        raise NotImplementedError(LIMITS + f"; got {func.__name__}(affine={probe.affine}, track_running_stats={probe.track_running_stats})")


def _inorm(m):
    return isinstance(m, torch.nn.InstanceNorm3d)


class Generator3DEngine(ParamIndex):
    def __init__(self, net, dtype=None):
        self.net = net
        self.dtype, self.tdt = compute_dtype(dtype)
        self.packs = _PackCache()
        self.trust_versions = False      # see engine_common.pack_reuse_allowed
        self.grad_ready_hook = self.after_backward = self.grad_fetch = None      # parallel.GradReducer.attach

    def blocks(self):
        """LinearUpsampleUnetSkipConnectionBlocks from the outermost (depth 0) to the innermost"""
        out, b = [], self.net.model
        while b is not None:
            out.append(b)
            sub = None
            for m in b.model:
                if m.__class__.__name__ == "LinearUpsampleUnetSkipConnectionBlock":
                    sub = m
            b = sub
        return out

    @staticmethod
    def _parts(block):
        """(cell, downnorm, upconv, upnorm, dropout) of a block; absent ones None"""
        cell = conv = drop = None
        norms = []
        for m in block.model:
            n = m.__class__.__name__
            if n == "Cell_conv":
                cell = m
            elif n == "Conv3d":
                conv = m
            elif n in ("BatchNorm3d", "InstanceNorm3d"):
                norms.append(m)
            elif n == "Dropout":
                drop = m
        if block.outermost:
            downnorm = upnorm = None
        elif block.innermost:
            downnorm, upnorm = None, norms[0]
        else:
            downnorm, upnorm = norms[0], norms[1]
        return cell, downnorm, conv, upnorm, drop

    def layout(self):
        """(depth, cell, downnorm, up-conv, upnorm, dropout) per block, outermost first"""
        return [(d, *self._parts(b)) for d, b in enumerate(self.blocks())]

    def check_input(self, x):
        """the refusals of an input, raised before any launch (and before the device check)"""
        nd = len(self.blocks())
        if x.dim() != 5:
            raise ValueError(f"the 3-D generator takes a volume [N,C,D,H,W], got a {x.dim()}-D tensor {tuple(x.shape)}")
        if any(s % (1 << nd) or s <= 0 for s in x.shape[2:]):
            raise ValueError(f"input volume {list(x.shape[2:])}: every spatial size must be a multiple of {1 << nd} "
                             f"(2^num_downs, num_downs = {nd})")
        if not x.is_cuda:
            raise RuntimeError("semantic_segmentation_amd Pix2Pix networks run on the MI355X only (no CPU / ATen fallback)")

    def run(self, x, dropout_masks=None):
        from . import networks3d
        arch = networks3d.conv_arch                      # the module global, read per call (as Cell_conv does)
        self.check_input(x)
        params = self.param_list()
        need_grad = torch.is_grad_enabled() and (x.requires_grad or arch.requires_grad or any(p.requires_grad for p in params))
        return _Generator3DFunction.apply(self, self.net.training, need_grad, dropout_masks, x, arch, *params)

    def _cell_weights(self, cell):
        w = [cell._ops._ops[j].op.weight for j in range(3)]
        b = [cell._ops._ops[j].op.bias for j in range(3)]
        return w, (None if any(bi is None for bi in b) else b)

    def _cell_pack(self, k, plan, w, sm, arch, dgrad):
        """the merged forward (or data-gradient) pack of cell k, cached on the versions of its three kernels and of conv_arch"""
        def build():
            ws = [t.detach().float().contiguous() for t in w]
            pf, pd = ce.merge_packs(plan, ws[0], ws[1], ws[2], sm, self.tdt, fwd=not dgrad, dgrad=dgrad)
            return pd if dgrad else pf
        return self.packs.get(("cell", k, dgrad, plan.dt0, plan.nd), _ver(w[0], w[1], w[2], arch), build)

    # -------------------------------------------------------------------------------------------------
    def forward(self, x, arch, training, need_grad, dropout_masks):
        self.check_input(x)
        lay = self.layout()
        tdt = self.tdt
        nd = len(lay)
        dev = x.device
        x = x.contiguous().float()
        N, cin0 = x.shape[0], x.shape[1]
        if not pack_reuse_allowed(need_grad, self.trust_versions):
            self.packs.clear()       # training forwards always re-pack: `.data` writes (Betty) bump no version counter

        def empty(*shape, dtype=tdt):
            return torch.empty(shape, dtype=dtype, device=dev)

        c = [cin0] + [p[1]._ops._ops[0].op.weight.shape[0] for p in lay]     # c[k]: channels after k cells
        size = [tuple(s >> k for s in x.shape[2:]) for k in range(nd + 1)]

        def nd_hw(k):
            return (N * size[k][0], size[k][1], size[k][2])

        sm_all = torch.softmax(arch.detach().float().to(dev), dim=-1).contiguous()
        levels = [None] * (nd + 1)
        ups = [None] * nd
        L = [None] * (nd + 1)            # leaky(norm(y_k)), dense: input of cell k+1
        R = [None] * (nd + 1)            # [N*D_k,H_k,W_k,2 c_k]: relu(skip) | relu(up); the innermost level: relu(y) alone
        nbt_pending = []

        # ---- down path ---------------------------------------------------------------------------------
        for k in range(1, nd + 1):
            _, cell, downnorm, _, _, _ = lay[k - 1]
            li = cell._layer_index
            w, b = self._cell_weights(cell)
            sm = sm_all[li]
            plan = cached_geom(ce.cell_plan, N, *size[k - 1], c[k - 1], c[k])
            pf = self._cell_pack(k, plan, w, sm, arch, dgrad=False)
            xg = ce.gather(plan, x if k == 1 else L[k - 1], tdt)
            y = empty(*nd_hw(k), c[k])
            inorm = _inorm(downnorm)
            has_bn = downnorm is not None and not inorm
            bias = None
            if b is not None and downnorm is None:                   # (in front of a norm the bias cancels)
                bias = ((sm[0] * b[0].detach() + sm[1] * b[1].detach()) + sm[2] * b[2].detach()).float().contiguous()
            lv = dict(plan=plan, xg=xg, y=y, sm=sm, li=li, coef=None, stats=False, cancelled=downnorm is not None)
            if has_bn:
                mt = ops.conv_igemm_mtiles(plan.gfwd)
                use_stats = training or downnorm.running_mean is None
                part = empty(ops.bn_partials_numel(mt, c[k]), dtype=torch.float32) if use_stats else None
                ops.conv_igemm(plan.gfwd, xg, pf, y, None, part)
                lv["coef"], lv["stats"] = bn_coeffs(downnorm, part, mt, c[k], y.shape[0] * y.shape[1] * y.shape[2], training, dev,
                                                    nbt_pending)
            else:
                ops.conv_igemm(plan.gfwd, xg, pf, y, bias)
            levels[k] = lv
            if k == nd:                                              # innermost: cell -> uprelu -> upsample
                R[k] = empty(*nd_hw(k), c[k])
                ops.bn_act_apply(y, None, None, ACT_RELU, R[k], c[k], 0)
                continue
            L[k] = empty(*nd_hw(k), c[k])
            R[k] = empty(*nd_hw(k), 2 * c[k])
            if inorm:
                yv = per_sample(y, N)
                mi = instance_stats(yv, downnorm)
                lv.update(stats=True, inorm=mi)
                ops.in_act_apply(yv, mi[0], mi[1], ACT_LEAKY02, L[k], c[k], 0, z2=R[k], act2=ACT_RELU, z2_stride=2 * c[k], z2_coff=0)
            else:
                sc, sh = (lv["coef"][0], lv["coef"][1]) if has_bn else (None, None)
                ops.bn_act_apply(y, sc, sh, ACT_LEAKY02, L[k], c[k], 0)
                ops.bn_act_apply(y, sc, sh, ACT_RELU, R[k], 2 * c[k], 0)

        # ---- up path -----------------------------------------------------------------------------------
        out = None
        mask_i = 0
        for d in range(nd - 1, -1, -1):                              # block depth d consumes R[d+1]
            _, _, _, conv, upnorm, drop = lay[d]
            C = R[d + 1].shape[3]
            v = ce.upsample_forward(R[d + 1], N, *size[d + 1], C)    # [N*D_d,H_d,W_d,C/4], dense
            cin, cout = C // 4, conv.out_channels
            if conv.in_channels != cin or conv.kernel_size != (3, 3, 3) or conv.stride != (1, 1, 1) or conv.padding != (1, 1, 1):
                raise NotImplementedError("the 3-D generator's up-convs are expected as Conv3d(C/4, outer_nc, k 3, stride 1, pad 1)")
            if d == 0:                                               # the tail: + bias, tanh, fp32 NCDHW image
                out = torch.empty((N, cout, *size[0]), dtype=torch.float32, device=dev)
                ops.conv3d_tail_fwd(v, conv.weight.detach().float().contiguous(), _bias32(conv), out, ACT_TANH)
                ups[0] = dict(v=v, conv=conv)
                continue
            wf, wd = self.packs.get(("up", d), _ver(conv.weight), lambda conv=conv: pack_conv(conv.weight, tdt, view=ops.conv3d_weight_view))
            g = cached_geom(ops.geom_conv3d, N, *size[d], cin, cout, 3, 1, 1)
            u = empty(*nd_hw(d), cout)
            inorm = _inorm(upnorm)
            up = dict(v=v, u=u, conv=conv, geom=g, wd=wd, cin=cin, cout=cout, coef=None, stats=True)
            if inorm:
                ops.conv_igemm(g, v, wf, u, None, None)              # the conv's bias cancels in the norm: not added
                uv = per_sample(u, N)
                mi = instance_stats(uv, upnorm)
                up["inorm"] = mi
            else:
                mt = ops.conv_igemm_mtiles(g)
                use_stats = training or upnorm.running_mean is None
                part = empty(ops.bn_partials_numel(mt, cout), dtype=torch.float32) if use_stats else None
                ops.conv_igemm(g, v, wf, u, None, part)
                up["coef"], up["stats"] = bn_coeffs(upnorm, part, mt, cout, u.shape[0] * u.shape[1] * u.shape[2], training, dev,
                                                    nbt_pending, conv_bias=conv.bias)
            keep, kscale = dropout_keep(drop, training, dropout_masks, mask_i, *nd_hw(d), cout, dev)
            if drop is not None:
                mask_i += 1
            if inorm:
                ops.in_act_apply(uv, mi[0], mi[1], ACT_RELU, R[d], 2 * c[d], c[d], keep, kscale)
            else:
                ops.bn_act_apply(u, up["coef"][0], up["coef"][1], ACT_RELU, R[d], 2 * c[d], c[d], None, keep, kscale)
            up.update(keep=keep, kscale=kscale)
            ups[d] = up
        _flush_nbt(nbt_pending)
        if not need_grad:
            return out, None
        return out, dict(N=N, nd=nd, c=c, size=size, lay=lay, x=x, out=out.detach(), levels=levels, ups=ups, arch_dev=arch.device)

    # -------------------------------------------------------------------------------------------------
    def backward(self, ctx, arch, dout, need_dx):
        tdt = self.tdt
        N, nd, c, size, lay, levels, ups = ctx["N"], ctx["nd"], ctx["c"], ctx["size"], ctx["lay"], ctx["levels"], ctx["ups"]
        dev = dout.device
        S = grad_scale(N * size[0][0] * size[0][1] * size[0][2])
        inv_s = 1.0 / S
        from ..parallel import GradEmitter
        emitter = GradEmitter(self.grad_ready_hook)          # data parallel: announced as soon as final
        names = {id(p): n for n, p in zip(self.param_names(), self.param_list())}
        darch = torch.zeros(arch.shape, dtype=torch.float32, device=dev)

        def empty(*shape, dtype=tdt):
            return torch.empty(shape, dtype=dtype, device=dev)

        def emit(p, g):
            emitter.emit(names[id(p)], g)

        def nd_hw(k):
            return (N * size[k][0], size[k][1], size[k][2])

        def stage_bwd(y, st, norm, dz_a, sa, ca, act, **kw):
            dy, dgamma, dbeta = norm_act_bwd(y, st["coef"], st.get("inorm"), st["stats"], dz_a, sa, ca, act, inv_s, N, **kw)
            if dgamma is not None:
                emit(norm.weight, dgamma)
                emit(norm.bias, dbeta)
            return dy

        # ---- the tail: out = tanh(conv(v_0) + bias) ----------------------------------------------------
        conv = ups[0]["conv"]
        v0 = ups[0]["v"]
        w0 = conv.weight.detach().float().contiguous()
        dv = torch.empty_like(v0)
        dw, db = torch.empty_like(w0), torch.empty(w0.shape[0], dtype=torch.float32, device=dev)
        ops.conv3d_tail_bwd(v0, w0, ctx["out"], dout.contiguous().float(), dv, dw, db, ACT_TANH, S)
        emit(conv.weight, dw * inv_s)
        if conv.bias is not None:
            emit(conv.bias, db * inv_s)
        dR = {1: ce.upsample_backward(dv, N, *size[1], 2 * c[1])}    # gradient w.r.t. R_1 [.., 2 c_1]

        # ---- walk inwards through the up path ----------------------------------------------------------
        for d in range(1, nd):
            up = ups[d]
            conv, upnorm = up["conv"], lay[d][4]
            du = stage_bwd(up["u"], up, upnorm, dR[d], 2 * c[d], c[d], ACT_RELU, keep=up["keep"], kscale=up["kscale"])
            emit(conv.weight, conv_wgrad(up["geom"], up["v"], du, conv.weight, up["cout"], up["cin"], 27, inv_s))
            if conv.bias is not None and up["stats"]:                # in front of batch / instance statistics: cancelled
                emit(conv.bias, torch.zeros_like(conv.bias))
            elif conv.bias is not None:                              # running statistics: the bias sits in the shift
                db = empty(up["cout"], dtype=torch.float32)
                ops.colsum(du, up["cout"], 0, *nd_hw(d), 0, 0, size[d][1], size[d][2], up["cout"], inv_s,
                           empty(1024 * up["cout"], dtype=torch.float32), db)
                emit(conv.bias, db)
            dv = empty(*nd_hw(d), up["cin"])
            ops.conv_igemm(cached_geom(ops.geom_conv3d_dgrad_s1, N, *size[d], up["cin"], up["cout"], 3, 1), du, up["wd"], dv)
            dR[d + 1] = ce.upsample_backward(dv, N, *size[d + 1], 4 * up["cin"])

        # ---- down path, innermost first ----------------------------------------------------------------
        dL = None                                                    # gradient w.r.t. L_k (dense), from cell k+1
        dx = None
        for k in range(nd, 0, -1):
            lv = levels[k]
            _, cell, downnorm, _, _, _ = lay[k - 1]
            plan, sm = lv["plan"], lv["sm"]
            if k == nd:                                              # innermost: only the ReLU consumer
                dy = stage_bwd(lv["y"], lv, downnorm, dR[k], c[k], 0, ACT_RELU)
            else:
                dy = stage_bwd(lv["y"], lv, downnorm, dR[k], 2 * c[k], 0, ACT_RELU, dz_b=dL, act_b=ACT_LEAKY02)
            w, b = self._cell_weights(cell)
            ws = [t.detach().float().contiguous() for t in w]
            dw4, dw6, dw8, dots = ce.wgrad_split(plan, lv["xg"], dy, ws[0], ws[1], ws[2], sm, inv_s)
            for p, g in zip(w, (dw4, dw6, dw8)):
                emit(p, g)
            if b is not None and lv["cancelled"]:                    # in front of a norm: exact zeros, no share in d conv_arch
                for bj in b:
                    emit(bj, torch.zeros_like(bj))
            elif b is not None:
                dbm = empty(c[k], dtype=torch.float32)
                ops.colsum(dy, c[k], 0, *nd_hw(k), 0, 0, size[k][1], size[k][2], c[k], inv_s, empty(1024 * c[k], dtype=torch.float32), dbm)
                for j, bj in enumerate(b):
                    emit(bj, (sm[j] * dbm).contiguous())
                    dots[j] += (dbm * bj.detach()).sum()
            darch[lv["li"]] += sm * (dots - (sm * dots).sum())       # through the softmax of the row
            if k > 1 or need_dx:                                     # the outermost cell's eight launches only for an input gradient
                pd = self._cell_pack(k, plan, w, sm, arch, dgrad=True)
                d16 = ce.dgrad(plan, dy, pd)
                if k > 1:
                    dL = d16
                else:
                    dx = ce._to_volume(d16, N, c[0], *size[0], plan.cin_pad) * inv_s
        if self.after_backward is not None:
            self.after_backward()
        return emitter.grads, darch.to(ctx["arch_dev"]), dx

    def invalidate_packs(self):
        self.packs.clear()


class _Generator3DFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, training, need_grad, dropout_masks, x, arch, *plist):
        out, ectx = engine.forward(x, arch, training, need_grad, dropout_masks)
        ctx.engine, ctx.ectx, ctx.plist, ctx.arch = engine, ectx, plist, arch
        ctx.x_needs_grad = x.requires_grad
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.ectx is None:
            raise RuntimeError("UnetGenerator forward ran without gradient tracking")
        grads, darch, dx = ctx.engine.backward(ctx.ectx, ctx.arch, dout, ctx.x_needs_grad)
        return (None, None, None, None, dx, darch, *param_grads(ctx.engine, grads, ctx.plist))
