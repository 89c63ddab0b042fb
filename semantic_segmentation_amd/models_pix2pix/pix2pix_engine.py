"""Whole-network plan of the Pix2Pix U-Net generator on the HIP kernels, and the steps every Pix2Pix plan shares (this generator,
resnet_engine.py, and the discriminators of discriminator_engine.py -- the "Discriminator" notes below describe that plan on images).

Generator (reference models_pix2pix/networks.py:514-617, 8 levels at 256x256):
  * every 4x4/stride-2 down-conv is one MFMA implicit GEMM (the 1-channel outermost one a direct kernel that
    reads the fp32 NCHW mask); BatchNorm statistics come out of the conv epilogue.
  * the LeakyReLU(0.2, inplace=True) that opens every inner block mutates its input, which is also the skip
    operand of `torch.cat([x, model(x)], 1)` (:617): the skip carries leaky(x).  After the parent's in-place
    `uprelu` the up-conv therefore sees relu(leaky(x)) = relu(x): one BN pass per level writes leaky(bn(y))
    (next down-conv input) and relu(bn(y)) straight into the first half of the level's concat buffer R_k.
  * every mixed transposed conv (softmax(arch)-weighted k4/k6/k8, :486-511) runs as ONE merged k8/s2/p3
    transposed conv (exact; csrc/pix2pix.hip), split into 4 sub-pixel classes of 16 taps on the MFMA engine;
    BN (+dropout keep-mask) + ReLU write into the second half of R_{k-1}.
Discriminator (:620-665): direct 2->64 conv, three MFMA convs with BN+LeakyReLU, direct 512->1 head (fp32 logits).
PixelDiscriminator (:668-697) is the same stage list with 1x1 kernels and runs on DiscriminatorEngine(seq="net").
Images of 5..16 channels (an RGB pair is six; one-hot masks into the generator): the image-side conv, its weight and data gradient
are the fp32-MFMA kernels of csrc/ends_img.hip (image_conv_* below) instead of the direct ones; 1..4 channels launch what they did.
Gradients are carried multiplied by a power-of-two scale (see unet_engine.py).
`--norm instance` (InstanceNorm2d without parameters or running statistics, networks.py:23-38): the same plans with the norm's
statistics per (sample, channel) from gs_in_stats after each normed conv (train and eval alike) and gs_in_act_apply in place of
gs_bn_act_apply -- on the down path ONE pass writes both consumers.  The reference's convs then carry a bias: one directly in front
of an InstanceNorm cancels exactly in the norm, so the conv does not add it and its gradient is exact zeros (as the 3-D engine does
for BatchNorm, engine_common.bn_coeffs); the others (outermost / innermost down conv, image cell, the PatchGAN's first and last
conv) go through the convs' bias arguments and gs_colsum."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional

import torch

from .. import ops
from .._lib import ACT_LEAKY02, ACT_NONE, ACT_RELU, ACT_TANH
from ..engine_common import ParamIndex, _flush_nbt, bn_coeffs, compute_dtype, pack_key, pack_reuse_allowed


def is_instance_norm(m):
    return isinstance(m, torch.nn.InstanceNorm2d)


def instance_stats(y, norm):
    """[2, N, C] fp32 (mean, invstd) of the stored conv output y [N,H,W,C] per (sample, channel): gs_in_stats"""
    N, H, W, C = y.shape
    mi = torch.empty((2, N, C), dtype=torch.float32, device=y.device)
    ops.in_stats(y, norm.eps, mi[0], mi[1], ops.in_workspace(N, H, W, C, y.device))
    return mi


def _bias32(conv):
    return None if conv.bias is None else conv.bias.detach().float().contiguous()


def _need_cuda(x):
    if not x.is_cuda:
        raise RuntimeError("semantic_segmentation_amd Pix2Pix networks run on the MI355X only (no CPU / ATen fallback)")


IMAGE_NC_MAX = 16           # image channels of the first-layer kernels: 1..4 csrc/direct.hip, 5..16 csrc/ends_img.hip


def _check_image_conv(who, cin, cout):
    """the refusals of the image-side conv, raised before any launch (and before the device check)"""
    if cin > IMAGE_NC_MAX:
        raise NotImplementedError(f"{who} input_nc {cin} is not supported: the first-layer kernels take up to {IMAGE_NC_MAX} image channels")
    if cin > 4 and (cout % 8 != 0 or cout > 128):
        raise NotImplementedError(f"{who} with input_nc {cin} (5..{IMAGE_NC_MAX}) needs a first layer of a multiple of 8 and at most 128 "
                                  f"output channels, got {cout}")


def image_conv_fwd(x, conv, y, k, s, p, act):
    """the conv on the fp32 NCHW image: direct kernel for 1..4 channels, the fp32-MFMA kernel for 5..16"""
    w = conv.weight.detach().contiguous()
    b = _bias32(conv)
    if x.shape[1] > 4:
        ops.conv_imgwide_fwd(x, w, b, y, k, s, p, act)
    else:
        ops.conv_smallcin_fwd(x, w, b, y, None, k, s, p, act)


def image_conv_wgrad(x, dy, conv, k, s, p, inv_s):
    if x.shape[1] > 4:
        dw = torch.empty_like(conv.weight, memory_format=torch.contiguous_format)
        ops.conv_imgwide_wgrad(x, dy, dw, k, s, p, inv_s)
    else:
        dw = torch.zeros_like(conv.weight, memory_format=torch.contiguous_format)
        ops.conv_smallcin_wgrad(x, dy, dw, k, s, p, inv_s)
    return dw


def image_conv_dgrad(dy, conv, x, k, s, p, inv_s):
    dx = torch.empty_like(x)
    w = conv.weight.detach().contiguous()
    if x.shape[1] > 4:
        ops.conv_imgwide_dgrad(dy, w, dx, k, s, p, inv_s)
    else:
        ops.conv_smallcin_dgrad(dy, w, dx, k, s, p, inv_s)
    return dx


# GSSEG_PIX2PIX_DIRECT_IMAGE=0: run the outermost generator layer on the MFMA engine (4 class launches + tanh + layout pass)
DIRECT_IMAGE_LAYER = os.environ.get("GSSEG_PIX2PIX_DIRECT_IMAGE", "1") != "0"


_GEOMS = {}


def cached_geom(builder, *args, identity_slots=False, **kw):
    """ops.geom_* / ops.make_geom results, memoised: building one fills 64-entry tap tables from Python (5-10 us) and a step asked for
    ~180 of them.  The geometries are read-only here (identity_slots: tap t lives in weight slot t, set once)."""
    key = (builder.__name__, args, tuple(sorted(kw.items())), identity_slots)
    g = _GEOMS.get(key)
    if g is None:
        g = builder(*args, **kw)
        if identity_slots:
            g_tapw_identity(g)
        if len(_GEOMS) > 4096:
            _GEOMS.clear()
        _GEOMS[key] = g
    return g


class _PackCache:
    """version-keyed 16-bit weight packs.  Entries built while a stream capture is running (harness hip_graphs) live in the
    graph's memory pool and are rebuilt by every replay of that graph; a capture reuses ONLY such entries (a pack built by eager
    code belongs to eager code, which may free it: a graph must not read it), eager code reuses any entry whose version matches
    (eager updates bump the versions, so it never sees a captured entry of older weights)."""

    def __init__(self):
        self._d = {}
        self._captured = []          # (key, tensor, refill) of every entry built during a stream capture: graphs hold their pointers

    def get(self, key, versions, build, refill=None):
        """refill(val): re-runs the build INTO the existing tensor `val` (kept for captured entries: refresh() below)"""
        capturing = torch.cuda.is_current_stream_capturing()
        ent = self._d.get(key)
        if ent is not None and ent[0] == versions and (ent[2] or not capturing):
            return ent[1]
        val = build()
        self._d[key] = (versions, val, capturing)
        if capturing and refill is not None:
            self._captured.append((key, val, refill))
        return val

    def refresh(self, match, versions_of):
        """Re-fill, in place, EVERY captured tensor whose key satisfies match(key).  A captured pack is written only by replays of
        the graph that built it; a graph captured LATER that merely reads it (harness: the Generator graph reads the forward packs
        the Discriminator graph merges) sees stale contents when an eager update of an input (the arch step) falls between that
        writer's replay and its own -- the eager code that made the update calls this to bring the buffers up to date.  It does not
        go by the cache entries (an eager forward in between may have replaced them): every buffer a graph may read is re-filled.
        versions_of(key) -> the current version tuple, stamped on the cache entry that still points at a re-filled tensor."""
        n = 0
        for key, val, refill in self._captured:
            if not match(key):
                continue
            refill(val)
            ent = self._d.get(key)
            if ent is not None and ent[1] is val:
                self._d[key] = (versions_of(key), val, ent[2])
            n += 1
        return n

    def clear(self):
        self._d.clear()              # (the captured tensors stay registered: graphs that read them may still be replayed)


def _ver(*ts):
    """version key of a pack made from the tensors ts: (data_ptr, _version) of each (engine_common.pack_key; GSSEG_PACK_CACHE=0,
    for loops that write parameters through `.data`: a key that no earlier one equals)"""
    return tuple(pack_key(t)[:2] for t in ts)


class _EmitDict:
    """`grads[name] = g` of a backward pass routed through parallel.GradEmitter (each name is assigned once)"""

    def __init__(self, emitter):
        self._e = emitter

    def __setitem__(self, name, g):
        self._e.emit(name, g)


# =====================================================================================================
# Steps every Pix2Pix plan shares (generator, ResNet generator, the discriminators of discriminator_engine.py)
# =====================================================================================================
def grad_scale(n):
    """the power of two nearest to n: gradients are carried multiplied by it (see unet_engine.py)"""
    return float(2 ** round(math.log2(n)))


def pack_conv(w, tdt, transposed=False, view=None):
    """(forward pack [taps][Cout][Cin], data-gradient pack [taps][Cin][Cout]) in the 16-bit dtype tdt of a conv weight
    [Cout][Cin][kh][kw] (transposed: [Cin][Cout][kh][kw]).  view: what turns a weight of another rank into the 4-D tensor
    gs_pack_weight takes (ops.conv3d_weight_view for [Cout][Cin][k][k][k])."""
    w = w.detach().contiguous()
    if view is not None:
        w = view(w)
    a, b, kh, kw = w.shape
    cout, cin = (b, a) if transposed else (a, b)
    wf = torch.empty((kh * kw, cout, cin), dtype=tdt, device=w.device)
    wd = torch.empty((kh * kw, cin, cout), dtype=tdt, device=w.device)
    ops.pack_weight(w, wf, wd, transposed)
    return wf, wd


def dropout_keep(drop, training, masks, i, N, h, w, C, dev):
    """(uint8 keep-mask [N,h,w,C] or None, scale) of the Dropout module `drop`: masks[i] where the caller brought masks, else drawn
    with torch.rand on the device"""
    if drop is None or not training or not drop.p > 0:
        return None, 1.0
    if masks is not None:
        keep = masks[i].to(dev).contiguous()
    else:
        keep = (torch.rand((N, h, w, C), device=dev) >= drop.p).to(torch.uint8)
    return keep, 1.0 / (1.0 - drop.p)


def per_sample(t, N):
    """[N*D,H,W,C] -> the [N, D*H, W, C] view the per-sample norm kernels take (a volume is one plane of D*H rows; csrc/instnorm.hip
    only uses H*W).  An image batch [N,H,W,C] is that view already and is returned as it is."""
    ND, H, W, C = t.shape
    return t if ND == N else t.view(N, (ND // N) * H, W, C)


def norm_act_bwd(y, coef, inorm, stats, dz_a, sa, ca, act, inv_s, N, dz_b=None, act_b=ACT_NONE, keep=None, kscale=1.0):
    """Gradient w.r.t. the stored conv output y [N*D,H,W,C] of  act(norm(y)) [two consumers dz_a/act and dz_b/act_b, dropout
    keep * kscale] -> (dy, dgamma, dbeta); the last two are None unless the norm is a BatchNorm.
    inorm: the (mean, invstd) [2,N,C] of an InstanceNorm stage (no parameters), taken per sample on the [N, D*H, W, C] view;
    else coef: the [4,C] scale / shift / mean / invstd of a BatchNorm stage (engine_common.bn_coeffs), stats: whether they are
    the batch's -- a stage that ran on running statistics has no gradient through mean and variance, so its c1 / c2 are zeros;
    neither: no norm, the activation's gradient alone."""
    nd, h, w, C = y.shape
    dev = y.device
    dy = torch.empty_like(y)
    if inorm is not None:
        yv = per_sample(y, N)
        ops.in_act_bwd(yv, inorm[0], inorm[1], dz_a, sa, ca, act, dy, torch.empty((2, N, C), dtype=torch.float32, device=dev),
                       ops.in_workspace(N, yv.shape[1], w, C, dev), dz_b=dz_b, act_b=act_b, keep_mask=keep, keep_scale=kscale)
        return dy, None, None
    if coef is None:
        ops.bn_act_bwd_apply(y, dz_a, sa, ca, None, None, None, None, None, None, None, act, False, dy,
                             dz_b=dz_b, act_b=act_b, keep_mask=keep, keep_scale=kscale)
        return dy, None, None
    nt = ops.bn_bwd_tiles_used(nd, h, w, False)
    part = torch.empty(ops.bn_partials_numel(ops.bn_bwd_tiles(nd, h, w), C), dtype=torch.float32, device=dev)
    ops.bn_act_bwd_reduce(y, dz_a, sa, ca, None, coef[0], coef[1], coef[2], coef[3], act, part,
                          dz_b=dz_b, act_b=act_b, keep_mask=keep, keep_scale=kscale)
    dgamma = torch.empty(C, dtype=torch.float32, device=dev)
    dbeta = torch.empty(C, dtype=torch.float32, device=dev)
    c12 = torch.empty((2, C), dtype=torch.float32, device=dev)
    ops.bn_bwd_coeffs(part, nt, C, nd * h * w, inv_s, dgamma, dbeta, c12[0], c12[1])
    if not stats:
        c12.zero_()
    ops.bn_act_bwd_apply(y, dz_a, sa, ca, None, coef[0], coef[1], coef[2], coef[3], c12[0], c12[1], act, True, dy,
                         dz_b=dz_b, act_b=act_b, keep_mask=keep, keep_scale=kscale)
    return dy, dgamma, dbeta


def conv_wgrad(g, x, dy, w, A, B, taps, inv_s):
    """weight gradient of the conv of geometry g straight into w's own layout [A][B][taps], from its input x and dy.
    K parts in slabs + ordered reduction fused with scale / unpack (one part: a plain store): deterministic"""
    dw = torch.empty_like(w, memory_format=torch.contiguous_format)
    wsl = torch.empty(max(ops.conv_wgrad_ws_floats(g), 1), dtype=torch.float32, device=dy.device)
    ops.conv_wgrad_det(g, x, dy, wsl, dw, A, B, taps, inv_s)
    return dw


def conv_s2_dgrad(dy, wd, dz, k, p):
    """data gradient dz [N,IH,IW,Cin] of Conv2d(k, stride 2, padding p) from dy and the data-gradient pack wd: the four classes
    of input pixels (row / column parity) in ONE launch"""
    N, ih, iw, cin = dz.shape
    gds = [cached_geom(ops.geom_conv_s2_dgrad_class, N, ih, iw, cin, dy.shape[3], k, p, cls >> 1, cls & 1) for cls in range(4)]
    ops.conv_igemm_batch(gds, dy, [wd] * 4, dz)


def param_grads(engine, grads, plist):
    """what an autograd Function of these plans returns for the parameters plist (engine.param_list() at forward time) from the
    gradients `grads` its backward emitted by state-dict name"""
    fetch = engine.grad_fetch               # data parallel: the reduced gradients
    return [(fetch(n) if (fetch is not None and n in grads) else grads.get(n)) if p.requires_grad else None
            for n, p in zip(engine.param_names(), plist)]


# =====================================================================================================
# Generator
# =====================================================================================================
class GeneratorEngine(ParamIndex):
    def __init__(self, net, dtype=None):
        self.net = net
        self.dtype, self.tdt = compute_dtype(dtype)
        self.packs = _PackCache()
        self._layer_of, self._merge_inputs = {}, {}      # per block depth: arch row / the three kernels of its merged pack
        self.trust_versions = False      # see engine_common.pack_reuse_allowed
        self.grad_ready_hook = self.after_backward = self.grad_fetch = None      # parallel.GradReducer.attach

    def blocks(self):
        """UnetSkipConnectionBlocks from the outermost (depth 0) to the innermost."""
        out, b = [], self.net.model
        while b is not None:
            out.append(b)
            sub = None
            for m in b.model:
                if m.__class__.__name__ == "UnetSkipConnectionBlock":
                    sub = m
            b = sub
        return out

    @staticmethod
    def _parts(block):
        conv = cell = None
        norms, drop = [], None
        for m in block.model:
            n = m.__class__.__name__
            if n == "Conv2d":
                conv = m
            elif n == "Cell_upconv":
                cell = m
            elif n in ("BatchNorm2d", "InstanceNorm2d"):
                norms.append(m)
            elif n == "Dropout":
                drop = m
        if block.outermost:
            downnorm = upnorm = None
        elif block.innermost:
            downnorm, upnorm = None, norms[0]
        else:
            downnorm, upnorm = norms[0], norms[1]
        return conv, downnorm, cell, upnorm, drop

    def run(self, x, dropout_masks=None):
        from . import networks
        arch = networks.upconv_arch
        params = self.param_list()
        need_grad = torch.is_grad_enabled() and (x.requires_grad or arch.requires_grad or
                                                 any(p.requires_grad for p in params))
        return _GeneratorFunction.apply(self, self.net.training, need_grad, dropout_masks, x, arch, *params)

    # -------------------------------------------------------------------------------------------------
    def forward(self, x, arch, training, need_grad, dropout_masks):
        blocks = self.blocks()
        _check_image_conv("generator", x.shape[1], self._parts(blocks[0])[0].out_channels)
        _need_cuda(x)
        net, tdt = self.net, self.tdt
        D = len(blocks)
        N, cin0, H, W = x.shape
        if H % (1 << D) or W % (1 << D):
            raise ValueError(f"input size must be a multiple of {1 << D}")
        dev = x.device
        x = x.contiguous().float()
        arch = arch.to(dev)
        if not pack_reuse_allowed(need_grad, self.trust_versions):
            self.packs.clear()       # training forwards always re-pack: `.data` writes (Betty) bump no version counter

        def empty(*shape, dtype=tdt):
            return torch.empty(shape, dtype=dtype, device=dev)

        parts = [self._parts(b) for b in blocks]
        c = [cin0] + [p[0].out_channels for p in parts]            # c[k]: channels after k down-convs
        hs = [H >> k for k in range(D + 1)]
        ws = [W >> k for k in range(D + 1)]
        ctx = dict(N=N, D=D, c=c, hs=hs, ws=ws, parts=parts, training=training, x=x, levels=[None] * (D + 1),
                   ups=[None] * D)
        L: List[Optional[torch.Tensor]] = [None] * (D + 1)          # leaky(bn(y_k)), dense: next down-conv input
        R: List[Optional[torch.Tensor]] = [None] * (D + 1)          # [N,h_k,w_k,2c_k]: relu(skip) | relu(up)

        nbt_pending = []                 # num_batches_tracked counters of this pass: ONE foreach increment at the end
        # ---- down path -------------------------------------------------------------------------------
        conv0 = parts[0][0]
        y1 = empty(N, hs[1], ws[1], c[1])
        image_conv_fwd(x, conv0, y1, 4, 2, 1, ACT_NONE)
        L[1] = empty(N, hs[1], ws[1], c[1])
        R[1] = empty(N, hs[1], ws[1], 2 * c[1])
        ops.bn_act_apply(y1, None, None, ACT_LEAKY02, L[1], c[1], 0)
        ops.bn_act_apply(y1, None, None, ACT_RELU, R[1], 2 * c[1], 0)
        ctx["levels"][1] = dict(y=y1, coef=None, stats=False)
        for k in range(2, D + 1):
            conv, downnorm = parts[k - 1][0], parts[k - 1][1]
            wf, wd = self.packs.get(("down", k), _ver(conv.weight),
                                    lambda conv=conv: pack_conv(conv.weight, tdt))
            g = cached_geom(ops.geom_conv, N, hs[k - 1], ws[k - 1], c[k - 1], c[k], 4, 2, 1)
            y = empty(N, hs[k], ws[k], c[k])
            if is_instance_norm(downnorm):                           # (never the innermost level: that one has no norm)
                ops.conv_igemm(g, L[k - 1], wf, y, None, None)       # the conv's bias cancels in the norm: not added
                mi = instance_stats(y, downnorm)
                ctx["levels"][k] = dict(y=y, coef=None, stats=True, inorm=mi, geom=g, wd=wd, inp=L[k - 1])
                L[k] = empty(N, hs[k], ws[k], c[k])
                R[k] = empty(N, hs[k], ws[k], 2 * c[k])
                ops.in_act_apply(y, mi[0], mi[1], ACT_LEAKY02, L[k], c[k], 0, z2=R[k], act2=ACT_RELU, z2_stride=2 * c[k], z2_coff=0)
                continue
            has_bn = downnorm is not None
            mt = ops.conv_igemm_mtiles(g)
            use_stats = has_bn and (training or downnorm.running_mean is None)
            part = empty(ops.bn_partials_numel(mt, c[k]), dtype=torch.float32) if use_stats else None
            ops.conv_igemm(g, L[k - 1], wf, y, None if has_bn else _bias32(conv), part)
            coef, stats = (None, False)
            if has_bn:
                coef, stats = bn_coeffs(downnorm, part, mt, c[k], N * hs[k] * ws[k], training, dev, nbt_pending)
            sc, sh = (coef[0], coef[1]) if has_bn else (None, None)
            ctx["levels"][k] = dict(y=y, coef=coef, stats=stats, geom=g, wd=wd, inp=L[k - 1])
            if k < D:
                L[k] = empty(N, hs[k], ws[k], c[k])
                R[k] = empty(N, hs[k], ws[k], 2 * c[k])
                ops.bn_act_apply(y, sc, sh, ACT_LEAKY02, L[k], c[k], 0)
                ops.bn_act_apply(y, sc, sh, ACT_RELU, R[k], 2 * c[k], 0)
            else:                                                    # innermost: conv -> uprelu -> upconv
                R[k] = empty(N, hs[k], ws[k], c[k])
                ops.bn_act_apply(y, sc, sh, ACT_RELU, R[k], c[k], 0)

        # ---- up path -----------------------------------------------------------------------------------
        sm_all = torch.softmax(arch.detach().float(), dim=-1).contiguous()      # every layer's mixing weights in one launch
        out = None
        mask_i = 0
        for d in range(D - 1, -1, -1):                               # block depth d consumes R[d+1]
            conv, downnorm, cell, upnorm, drop = parts[d]
            cin_t = R[d + 1].shape[3]
            cout_t = cell._ops._ops[0].op.weight.shape[1]
            li = cell._layer_index
            w4, w6, w8 = (cell._ops._ops[j].op.weight for j in range(3))
            sm = sm_all[li]
            cpad = cout_t if cout_t % 8 == 0 else ((cout_t + 7) // 8) * 8
            pf = self._merge_pack(d, w4, w6, w8, sm, cin_t, cout_t, cpad, dgrad=False, arch=arch, li=li)
            h, w = hs[d + 1], ws[d + 1]
            H2, W2 = 2 * h, 2 * w
            bias = None
            inorm = d > 0 and is_instance_norm(upnorm)
            if cell._ops._ops[0].op.bias is not None and not inorm:       # (in front of an InstanceNorm the bias cancels)
                bias = sum(sm[j] * cell._ops._ops[j].op.bias.detach() for j in range(3)).float().contiguous()
            if d > 0:
                u = empty(N, H2, W2, cout_t)
                mt = ops.conv_igemm_mtiles(cached_geom(ops.geom_convT_class, N, h, w, cin_t, cout_t, 8, 3, 0, 0, identity_slots=True))
                use_stats = not inorm and (training or upnorm.running_mean is None)
                part = empty(ops.bn_partials_numel(4 * mt, cout_t), dtype=torch.float32) if use_stats else None
                geoms = []
                for cls in range(4):
                    geoms.append(cached_geom(ops.geom_convT_class, N, h, w, cin_t, cout_t, 8, 3, cls >> 1, cls & 1, identity_slots=True))
                pslices = [part[cls * mt * 2 * cout_t:] for cls in range(4)] if part is not None else None
                # the four sub-pixel classes in ONE launch (each is latency bound on its own at the script's batch size)
                ops.conv_igemm_batch(geoms, R[d + 1], [pf[cls] for cls in range(4)], u, bias, pslices)
                if inorm:
                    coef, stats, mi = None, True, instance_stats(u, upnorm)
                else:
                    coef, stats = bn_coeffs(upnorm, part, 4 * mt, cout_t, N * H2 * W2, training, dev, nbt_pending)
                keep, kscale = dropout_keep(drop, training, dropout_masks, mask_i, N, H2, W2, cout_t, dev)
                if drop is not None:
                    mask_i += 1
                if inorm:
                    ops.in_act_apply(u, mi[0], mi[1], ACT_RELU, R[d], 2 * c[d], c[d], keep, kscale)
                else:
                    ops.bn_act_apply(u, coef[0], coef[1], ACT_RELU, R[d], 2 * c[d], c[d], None, keep, kscale)
                ctx["ups"][d] = dict(u=u, coef=coef, stats=stats, keep=keep, kscale=kscale, sm=sm, cin=cin_t,
                                     cout=cout_t, li=li)
                if inorm:
                    ctx["ups"][d]["inorm"] = mi
            else:                                                    # outermost: + bias, tanh, fp32 NCHW image
                u = empty(N, H2, W2, cpad)
                bpad = None
                if bias is not None:
                    bpad = torch.zeros(cpad, dtype=torch.float32, device=dev)
                    bpad[:cout_t] = bias
                out = torch.empty((N, cout_t, H2, W2), dtype=torch.float32, device=dev)
                if DIRECT_IMAGE_LAYER and cpad == 8 and ops.upconv8_image_fits(cin_t, cout_t):
                    # direct kernel: bias + tanh + fp32 NCHW in one pass (the MFMA engine would use 1 of 64 N columns)
                    ops.upconv8_image_fwd(R[1], pf, bpad, out, u if need_grad else None, N, h, w, cin_t, cout_t, ACT_TANH)
                else:
                    geoms = []
                    for cls in range(4):
                        geoms.append(cached_geom(ops.geom_convT_class, N, h, w, cin_t, cpad, 8, 3, cls >> 1, cls & 1, identity_slots=True))
                    ops.conv_igemm_batch(geoms, R[1], [pf[cls] for cls in range(4)], u, bpad, None)
                    t = empty(N, H2, W2, cpad)
                    ops.bn_act_apply(u, None, None, ACT_TANH, t, cpad, 0)
                    ops.nhwc_to_nchw(t, out, cpad, 0)
                ctx["ups"][0] = dict(u=u, sm=sm, cin=cin_t, cout=cout_t, cpad=cpad, li=li)
        ctx["R"], ctx["L"] = R, L
        _flush_nbt(nbt_pending)
        return out, (ctx if need_grad else None)

    def refresh_arch_packs(self, arch):
        """After an EAGER update of the architecture tensor while hipGraphs hold merged forward packs (harness.EndToEndTrainer):
        re-merge, in place, the captured packs whose version key no longer matches (see _PackCache.refresh)."""
        def versions_of(key):
            w4, w6, w8 = self._merge_inputs[key[1:]]
            return _ver(w4, w6, w8, arch)
        # (forward packs only: a graph that needs the data-gradient packs merges them itself)
        return self.packs.refresh(lambda k: k[0] == "merged" and not k[2] and k[1:] in self._merge_inputs, versions_of)

    def _merge_pack(self, d, w4, w6, w8, sm, cin_t, cout_t, cpad, dgrad, arch=None, li=None, out=None):
        """class-major forward pack [4][16][cpad][cin] (or dgrad pack [64][cin][cpad]) of the merged kernel.  Cached per
        (weights, architecture parameters) version: in the end-to-end loop the generator runs three times per iteration
        (Generator, Discriminator and Unet steps) between two updates of its weights, and re-merging reads all 1.09 GB
        of fp32 kernels each time."""
        if arch is not None:
            if li is None:
                li = self._layer_of.get(d)
            else:
                self._layer_of[d] = li
            self._merge_inputs[(d, dgrad, cpad)] = (w4, w6, w8)

            def refill(out, li=li):
                sm_now = torch.softmax(arch.detach().float(), dim=-1)[li].contiguous()
                self._merge_pack(d, w4, w6, w8, sm_now, cin_t, cout_t, cpad, dgrad, out=out)
            return self.packs.get(("merged", d, dgrad, cpad), _ver(w4, w6, w8, arch),
                                  lambda: self._merge_pack(d, w4, w6, w8, sm, cin_t, cout_t, cpad, dgrad),
                                  refill if li is not None else None)
        dev = w8.device
        if cpad == cout_t:
            w4p, w6p, w8p = w4.detach().contiguous(), w6.detach().contiguous(), w8.detach().contiguous()
        else:                                    # 1-channel image head: pad Cout to 8 with zero kernels
            def pad(w):
                z = torch.zeros((w.shape[0], cpad, w.shape[2], w.shape[3]), dtype=torch.float32, device=dev)
                z[:, :cout_t] = w.detach()
                return z
            w4p, w6p, w8p = pad(w4), pad(w6), pad(w8)
        if dgrad:
            pd = torch.empty((64, cin_t, cpad), dtype=self.tdt, device=dev) if out is None else out
            ops.upconv_merge_pack(w4p, w6p, w8p, sm, None, pd, None)
            return pd
        pf = torch.empty((4, 16, cpad, cin_t), dtype=self.tdt, device=dev) if out is None else out
        ops.upconv_merge_pack(w4p, w6p, w8p, sm, pf, None, None)
        return pf

    def invalidate_packs(self):
        self.packs.clear()


def g_tapw_identity(g):
    """class-major packs: tap t of the class lives in slot t."""
    for t in range(g.ntaps):
        g.tap_w[t] = t


class _GeneratorFunction(torch.autograd.Function):
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
        from .pix2pix_backward import generator_backward
        grads, darch, dx = generator_backward(ctx.engine, ctx.ectx, ctx.arch, dout, ctx.x_needs_grad)
        return (None, None, None, None, dx, darch, *param_grads(ctx.engine, grads, ctx.plist))
