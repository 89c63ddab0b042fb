"""The two operators of the 3-D Pix2Pix generator on the HIP path (reference: GenSeg-3D/models/networks.py:570-601 `MixedOp_conv` /
`Cell_conv` over architecture_pix2pix/operations.py:41-66 `conv_421 / 622 / 823`, and networks.py:50-81 `LinearAdditiveUpsample`).

Layout-level steps first -- they take and return the device layout, dense 16-bit depth-slice stacks [N*D,H,W,C] with a channel stride
and offset where a concat buffer is the source or target -- and are what a generator plan calls:
    cell_plan / merge_packs / gather / conv_forward / wgrad_split / dgrad          the mixed stride-2 Conv3d cell
    upsample_forward / upsample_backward                                           the linear additive upsample
The weighted sum of the three convs is ONE 8x8x8 / stride-2 / pad-3 conv (exact by linearity; a single primitive is the one-hot
case): 512 taps.  It runs as a 64-tap stride-1 conv over the parity-gathered volume x'[a,(pz,py,px,c)] = x[2a+pz-1, ...] on the generic
MFMA engine ("3-D Pix2Pix cells"); its weight gradient over the same geometry yields all 512 taps in one deterministic
launch, and its data gradient goes straight to x through the eight sub-voxel classes.  Only the taps that can meet data are merged
and run (ops.cell3d_boxes): at a 2x2x2 input that is 8 of 512.

The autograd Functions below are thin wrappers: fp32 NCDHW in and out like the stand-alone 2-D cells (cell_engine.py), first-order
autograd, CPU tensors raise."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from .. import ops
from ..unet.block_engine import _grad_scale, _tdt

LIMITS_CELL = ("mixed Conv3d cell (conv_421 / conv_622 / conv_823, MixedOp_conv, Cell_conv): C_in must be 1..4 (the image side) or a "
               "multiple of 8, C_out a multiple of 8, and every spatial size >= 2 (odd sizes are allowed)")
LIMITS_UP = ("LinearAdditiveUpsample on the HIP path: threed=True, scale_factor == 2, n_splits == 4 and a channel count that is a "
             "multiple of 32 (C/4 is then a whole number of 16-byte chunks)")


# ------------------------------------------------------------------------------------------------ layout-level steps: the cell
def cell_plan(N, D, H, W, Cin, Cout, dy_stride=None, dy_coff=0, full_box=False):
    """geometry of one mixed cell: the gathered sizes, the tap boxes, the forward / weight-gradient geometry over x' and the
    data-gradient classes.  dy_stride / dy_coff: where the cell's OUTPUT (and its gradient) lives, if not dense."""
    if not ((1 <= Cin <= 4) or (Cin > 0 and Cin % 8 == 0)) or Cout <= 0 or Cout % 8 or min(D, H, W) < 2:
        raise NotImplementedError(f"{LIMITS_CELL}; got C_in={Cin}, C_out={Cout}, volume {D}x{H}x{W}")
    dt0, nd, k0, nk = ops.cell3d_boxes(D, H, W, full_box)
    p = SimpleNamespace(N=N, D=D, H=H, W=W, Cin=Cin, Cout=Cout, image=Cin < 8, cin_pad=(Cin + 7) // 8 * 8,
                        GD=ops.cell3d_gathered_size(D), GH=ops.cell3d_gathered_size(H), GW=ops.cell3d_gathered_size(W),
                        OD=D // 2, OH=H // 2, OW=W // 2, dt0=dt0, nd=nd, k0=k0, nk=nk,
                        ntaps=nd[0] * nd[1] * nd[2], nktaps=nk[0] * nk[1] * nk[2], dy_stride=dy_stride, dy_coff=dy_coff)
    p.gfwd = ops.geom_cell3d_fwd(N, D, H, W, Cin, Cout, dt0, nd, out_stride=dy_stride, out_coff=dy_coff)
    p.gdgrad = None
    return p


def merge_packs(p, w4, w6, w8, sm, tdt, fwd=True, dgrad=True):
    """(forward pack [taps][C_out][8 C_in], data-gradient pack [k taps][cin_pad][C_out]) of sm0 w4 + sm1 w6 + sm2 w8 over the plan's
    boxes; either may be left out (None)"""
    dev = w8.device
    pf = torch.empty((p.ntaps, p.Cout, 8 * p.Cin), dtype=tdt, device=dev) if fwd else None
    pd = torch.empty((p.nktaps, p.cin_pad, p.Cout), dtype=tdt, device=dev) if dgrad else None
    ops.cell3d_merge_pack(w4, w6, w8, sm, pf, pd, p.dt0, p.nd, p.k0, p.nk, p.cin_pad)
    return pf, pd


def gather(p, src, tdt, in_stride=None, in_coff=0):
    """x' of the plan's volume: src 16-bit [N*D,H,W,*] (C_in % 8 == 0) or the fp32 NCDHW image (C_in 1..4)"""
    xg = torch.empty((p.N * p.GD, p.GH, p.GW, 8 * p.Cin), dtype=tdt, device=src.device)
    ops.cell3d_gather(src, xg, p.N, p.D, p.H, p.W, p.Cin, in_stride, in_coff)
    return xg


def conv_forward(p, xg, pf, bias=None, y=None):
    """y [N*OD,OH,OW,C_out] (or the plan's channel slice of a wider y) = cell(x) + bias"""
    if y is None:
        y = torch.empty((p.N * p.OD, p.OH, p.OW, p.Cout if p.dy_stride is None else p.dy_stride), dtype=xg.dtype, device=xg.device)
    ops.conv_igemm(p.gfwd, xg, pf, y, bias)
    return y


def wgrad_split(p, xg, du, w4, w6, w8, sm, gscale=1.0):
    """du = d(output) 16-bit -> (dw4, dw6, dw8, dots[3]): all 512 taps from one deterministic launch over the gathered geometry, split
    into sm_j times the centred crops; dots[j] = <dWm, embed(W_j)>, the derivative with respect to the mixing weight j"""
    dev = xg.device
    dwm = torch.empty((p.ntaps, p.Cout, 8 * p.Cin), dtype=torch.float32, device=dev)
    ws = torch.empty(max(ops.conv_wgrad_ws_floats(p.gfwd), 1), dtype=torch.float32, device=dev)
    ops.conv_wgrad_det(p.gfwd, xg, du, ws, dwm, p.Cout, 8 * p.Cin, p.ntaps, 1.0, packed=True)
    dw4, dw6, dw8 = (torch.empty((p.Cout, p.Cin, k, k, k), dtype=torch.float32, device=dev) for k in (4, 6, 8))
    dots = torch.empty(3, dtype=torch.float32, device=dev)
    ops.cell3d_split_wgrad(dwm, w4, w6, w8, sm, gscale, dw4, dw6, dw8, dots, p.dt0, p.nd)
    return dw4, dw6, dw8, dots


def dgrad(p, du, pd, dx=None, dx_stride=None, dx_coff=0):
    """dx 16-bit [N*D,H,W,cin_pad] (or a channel slice of a wider dx): the eight sub-voxel classes of the stride-2 data gradient, each a
    launch of at most 64 taps of the compact pack"""
    if p.gdgrad is None or p.gdgrad[0] != (dx_stride, dx_coff):
        gs = [ops.geom_cell3d_dgrad_class(p.N, p.D, p.H, p.W, p.cin_pad, p.Cout, p.k0, p.nk, c >> 2, (c >> 1) & 1, c & 1,
                                          in_stride=p.dy_stride, in_coff=p.dy_coff, out_stride=dx_stride, out_coff=dx_coff) for c in range(8)]
        p.gdgrad = ((dx_stride, dx_coff), gs)
    if dx is None:
        dx = torch.empty((p.N * p.D, p.H, p.W, p.cin_pad if dx_stride is None else dx_stride), dtype=du.dtype, device=du.device)
    for g in p.gdgrad[1]:
        if g is None:
            raise RuntimeError("mixed Conv3d cell: a sub-voxel class without taps")     # cannot happen for sizes >= 2
        ops.conv_igemm(g, du, pd, dx)
    return dx


# ------------------------------------------------------------------------------------------------ layout-level steps: the upsample
def upsample_forward(x16, N, D, H, W, C, y=None, in_stride=None, in_coff=0, out_stride=None, out_coff=0):
    if C % 32:
        raise NotImplementedError(f"{LIMITS_UP}; got C={C}")
    if y is None:
        y = torch.empty((N * 2 * D, 2 * H, 2 * W, C // 4 if out_stride is None else out_stride), dtype=x16.dtype, device=x16.device)
    ops.upsample_add3d_fwd(x16, y, N, D, H, W, C, in_stride, in_coff, out_stride, out_coff)
    return y


def upsample_backward(dy16, N, D, H, W, C, dx=None, dy_stride=None, dy_coff=0, dx_stride=None, dx_coff=0):
    if C % 32:
        raise NotImplementedError(f"{LIMITS_UP}; got C={C}")
    if dx is None:
        dx = torch.empty((N * D, H, W, C if dx_stride is None else dx_stride), dtype=dy16.dtype, device=dy16.device)
    ops.upsample_add3d_bwd(dy16, dx, N, D, H, W, C, dy_stride, dy_coff, dx_stride, dx_coff)
    return dx


# ------------------------------------------------------------------------------------------------ fp32 NCDHW <-> the device layout
def _to_slices(x, tdt, scale=None):
    """fp32 [N,C,D,H,W] -> 16-bit [N*D,H,W,C] (the 2-D pass with the plane taken as D*H x W)"""
    N, C, D, H, W = x.shape
    src = x.detach().float()
    if scale is not None:
        src = src * scale
    dst = torch.empty((N * D, H, W, C), dtype=tdt, device=x.device)
    ops.nchw_to_nhwc(src.contiguous().view(N, C, D * H, W), dst)
    return dst


def _to_volume(t16, N, C, D, H, W, stride=None):
    out = torch.empty((N, C, D, H, W), dtype=torch.float32, device=t16.device)
    ops.nhwc_to_nchw(t16, out.view(N, C, D * H, W), stride, 0)
    return out


def _check_volume(x, what):
    if not x.is_cuda:
        raise RuntimeError(f"{what} (semantic_segmentation_amd) runs on the MI355X only: no CPU / ATen fallback")
    if x.dim() != 5:
        raise ValueError(f"{what}: expected an NCDHW tensor, got shape {tuple(x.shape)}")


# ------------------------------------------------------------------------------------------------ autograd wrappers
class _MixedConv3dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weights3, w4, w6, w8, b4, b6, b8):
        _check_volume(x, "mixed Conv3d cell")
        N, Cin, D, H, W = x.shape
        Cout = w8.shape[0]
        p = cell_plan(N, D, H, W, Cin, Cout)
        dev, tdt = x.device, _tdt()
        sm = weights3.detach().float().contiguous().to(dev)
        ws = [w.detach().float().contiguous() for w in (w4, w6, w8)]
        pf, _ = merge_packs(p, ws[0], ws[1], ws[2], sm, tdt, dgrad=False)
        bias = None
        if b8 is not None:
            bias = ((sm[0] * b4.detach() + sm[1] * b6.detach()) + sm[2] * b8.detach()).float().contiguous()
        xg = gather(p, x.detach().float().contiguous() if p.image else _to_slices(x, tdt), tdt)
        y = conv_forward(p, xg, pf, bias)
        ctx.save_for_backward(xg, sm, w4, w6, w8, b4, b6, b8)
        ctx.plan, ctx.need_dx = p, x.requires_grad
        return _to_volume(y, N, Cout, p.OD, p.OH, p.OW)

    @staticmethod
    def backward(ctx, dy):
        xg, sm, w4, w6, w8, b4, b6, b8 = ctx.saved_tensors
        p = ctx.plan
        dev, tdt = dy.device, _tdt()
        r = _grad_scale(dy)
        inv_r = torch.reciprocal(r)
        du = _to_slices(dy, tdt, r)
        ws = [w.detach().float().contiguous() for w in (w4, w6, w8)]
        dw4, dw6, dw8, dots = wgrad_split(p, xg, du, ws[0], ws[1], ws[2], sm)
        db = [None, None, None]
        if b8 is not None:
            colws = torch.empty(1024 * p.Cout, dtype=torch.float32, device=dev)
            dbm = torch.empty(p.Cout, dtype=torch.float32, device=dev)
            ops.colsum(du, p.Cout, 0, p.N * p.OD, p.OH, p.OW, 0, 0, p.OH, p.OW, p.Cout, 1.0, colws, dbm)
            for j, bj in enumerate((b4, b6, b8)):
                db[j] = (sm[j] * dbm * inv_r).contiguous()
                dots[j] += (dbm * bj.detach()).sum()
        dx = None
        if ctx.need_dx:
            _, pd = merge_packs(p, ws[0], ws[1], ws[2], sm, tdt, fwd=False)
            dx16 = dgrad(p, du, pd)
            dx = _to_volume(dx16, p.N, p.Cin, p.D, p.H, p.W, p.cin_pad) * inv_r
        return dx, dots * inv_r, dw4 * inv_r, dw6 * inv_r, dw8 * inv_r, db[0], db[1], db[2]


def mixed_conv3d(x, weights3, ops_list):
    """sum_j weights3[j] * ops_list[j](x) for the (k4, k6, k8) stride-2 Conv3d primitives: MixedOp_conv.forward"""
    w = [o.op.weight for o in ops_list]
    b = [o.op.bias for o in ops_list]
    if any(bi is None for bi in b):
        b = [None, None, None]
    return _MixedConv3dFunction.apply(x, weights3, w[0], w[1], w[2], b[0], b[1], b[2])


def single_conv3d(module, x):
    """One primitive on its own (conv_421 / 622 / 823): the one-hot case of the merged kernel; the two absent kernels are zero tensors
    whose (zero-weighted) gradients are dropped."""
    _check_volume(x, type(module).__name__)
    k = module.op.kernel_size[0]
    j = {4: 0, 6: 1, 8: 2}[k]
    cout, cin = module.op.weight.shape[0], module.op.weight.shape[1]
    dev = x.device
    ws, bs = [], []
    for jj, kk in enumerate((4, 6, 8)):
        if jj == j:
            ws.append(module.op.weight)
            bs.append(module.op.bias)
        else:
            ws.append(torch.zeros((cout, cin, kk, kk, kk), dtype=torch.float32, device=dev))
            bs.append(torch.zeros(cout, dtype=torch.float32, device=dev) if module.op.bias is not None else None)
    onehot = torch.zeros(3, dtype=torch.float32, device=dev)
    onehot[j] = 1.0
    return _MixedConv3dFunction.apply(x, onehot, ws[0], ws[1], ws[2], bs[0], bs[1], bs[2])


class _UpsampleAddFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        N, C, D, H, W = x.shape
        y = upsample_forward(_to_slices(x, _tdt()), N, D, H, W, C)
        ctx.dims = (N, C, D, H, W)
        return _to_volume(y, N, C // 4, 2 * D, 2 * H, 2 * W)

    @staticmethod
    def backward(ctx, dy):
        N, C, D, H, W = ctx.dims
        r = _grad_scale(dy)
        dx16 = upsample_backward(_to_slices(dy, _tdt(), r), N, D, H, W, C)
        return _to_volume(dx16, N, C, D, H, W) * torch.reciprocal(r)


def linear_additive_upsample(x, scale_factor, n_splits, threed):
    _check_volume(x, "LinearAdditiveUpsample")
    if not threed or scale_factor != 2 or n_splits != 4 or x.shape[1] % 32:
        raise NotImplementedError(f"{LIMITS_UP}; got threed={threed}, scale_factor={scale_factor}, n_splits={n_splits}, C={x.shape[1]}")
    return _UpsampleAddFunction.apply(x)
