"""fp64 statements of the two 3-D Pix2Pix generator operators (reference: GenSeg-3D/models/networks.py:570-601 MixedOp_conv / Cell_conv
over architecture_pix2pix/operations.py:41-66 conv_421 / 622 / 823, and networks.py:50-81 LinearAdditiveUpsample), the exact cases of
tests/test_cell3d_kernels_gpu.py, the cases of tests/test_cell3d_modules_gpu.py, and the comparers.  tests/test_cell3d_reference_cpu.py
proves the statements against torch.autograd and the fixture, and that the bounds tell the stated wrong implementations from a right one.

The mixed cell:  y = sum_j sm_j (Conv3d_j(x) + b_j),  (k, stride, pad) = (4,2,1), (6,2,2), (8,2,3), sm = softmax(conv_arch[layer]).
By linearity  y = Conv3d(x, Wm, k 8 / s 2 / p 3) + bm  with  Wm = sm0 embed(W4, offset 2) + sm1 embed(W6, offset 1) + sm2 W8,  bm = sum sm_j b_j;
    dW_j = sm_j crop_j(dWm),  db_j = sm_j colsum(dy),  d sm_j = <dWm, embed(W_j)> + <colsum(dy), b_j>,  dx = ConvTranspose3d(dy, Wm).
The gathered form:  x'[a,(pz,py,px,c)] = x[2a+pz-1, 2i+py-1, 2j+px-1, c]  (zero outside),  W'[co,(pz,py,px,c),t] = Wm[co,c,2t+p]:  the cell is the
stride-1 / pad-1 conv of 4x4x4 taps of x' with W'.
`store` (a 16-bit dtype) rounds what the engine stores in 16 bits: the source, the packs, the output, dy and dx  (e16 of the bound)."""
import math

import torch
import torch.nn.functional as F

from tests import exact_reference as er
from tests.backward_replay import FLOOR32, compare

KSP = {4: (2, 1), 6: (2, 2), 8: (2, 3)}
KS = (4, 6, 8)
CELL_MUTANTS = ("unshifted_parity", "embed0", "no_sm_dw", "no_bias_share", "sample_leak")
UP_MUTANTS = ("align_corners", "swapped_weights", "strided_groups", "no_clamp", "unequal_bwd")
DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def rnd(t, store):
    return t if store is None else t.to(store).to(t.dtype)


def slices(t):
    """[N,C,D,H,W] -> the device layout [N*D,H,W,C]"""
    N, C, D, H, W = t.shape
    return t.permute(0, 2, 3, 4, 1).reshape(N * D, H, W, C).contiguous()


def volume(t, N):
    """[N*D,H,W,C] -> [N,C,D,H,W]"""
    ND, H, W, C = t.shape
    return t.reshape(N, ND // N, H, W, C).permute(0, 4, 1, 2, 3).contiguous()


# ------------------------------------------------------------------------------------------------ the mixed cell
def embed(w, offset=None):
    """[Co,Ci,k,k,k] -> [Co,Ci,8,8,8], centred (offset (8 - k) / 2) unless another offset is given"""
    k = w.shape[-1]
    o = (8 - k) // 2 if offset is None else offset
    return F.pad(w, (o, 8 - k - o) * 3)


def crop(w8, k, offset=None):
    o = (8 - k) // 2 if offset is None else offset
    return w8[:, :, o:o + k, o:o + k, o:o + k]


def merged_weight(ws, sm, offset=None):
    return (sm[0] * embed(ws[0], offset) + sm[1] * embed(ws[1], offset)) + sm[2] * ws[2]


def three_convs(x, ws, bs, sm):
    """the reference's own form: MixedOp_conv.forward"""
    return sum(sm[j] * F.conv3d(x, ws[j], None if bs is None else bs[j], stride=2, padding=KSP[k][1]) for j, k in enumerate(KS))


def gathered_size(d):
    return d // 2 + 1


def gather(x, mutant=None):
    """x [N,C,D,H,W] -> x' [N,8C,GD,GH,GW], channel (pz,py,px,c).  unshifted_parity: x'[a,p] = x[2a+p]; sample_leak: the depth slices
    outside a sample are those of its neighbours in the [N*D] stack instead of zeros."""
    N, C, D, H, W = x.shape
    sh = 0 if mutant == "unshifted_parity" else 1
    G = [gathered_size(d) for d in (D, H, W)]
    pads = []
    for d, g in zip((W, H, D), reversed(G)):
        pads += [sh, 2 * g - d - sh]
    if mutant == "sample_leak":
        flat = x.permute(1, 0, 2, 3, 4).reshape(1, C, N * D, H, W)
        flat = F.pad(flat, pads[:4] + [sh, 2 * G[0]])
        xp = torch.cat([flat[:, :, n * D:n * D + 2 * G[0]] for n in range(N)], 0)
    else:
        xp = F.pad(x, pads)
    return torch.cat([xp[:, :, pz::2, py::2, px::2] for pz in (0, 1) for py in (0, 1) for px in (0, 1)], 1)


def gathered_weight(wm):
    """Wm [Co,Ci,8,8,8] -> W' [Co,8Ci,4,4,4]"""
    return torch.cat([wm[:, :, pz::2, py::2, px::2] for pz in (0, 1) for py in (0, 1) for px in (0, 1)], 1)


def ungathered_weight(wg):
    Co, C8 = wg.shape[:2]
    C = C8 // 8
    wm = wg.new_zeros((Co, C, 8, 8, 8))
    for q in range(8):
        wm[:, :, (q >> 2)::2, ((q >> 1) & 1)::2, (q & 1)::2] = wg[:, q * C:(q + 1) * C]
    return wm


def gathered_conv(x, wm, mutant=None):
    return F.conv3d(gather(x, mutant), gathered_weight(wm), None, stride=1, padding=1)


def reachable_taps(d):
    """taps k of the 8 / s2 / p3 conv that meet data on an axis of d entries, by brute force over every (output, tap) pair"""
    return sorted({k for o in range(d // 2) for k in range(8) if 0 <= 2 * o + k - 3 < d})


def cell_statement(x, ws, bs, sm, dy=None, store=None, mutant=None, form="k8", dtype=torch.float64):
    """dict(y, dx, dw4, dw6, dw8, [db4, db6, db8,] dsm): the cell and its gradients for d(output) = dy, in `dtype`.  form 'gathered':
    through x' and W' (the engine's route; the mutants of the gather act there)."""
    if mutant in ("unshifted_parity", "sample_leak"):
        form = "gathered"
    off = 0 if mutant == "embed0" else None
    x, sm = x.to(dtype), sm.to(dtype)
    ws = [w.to(dtype) for w in ws]
    bs = None if bs is None else [b.to(dtype) for b in bs]
    wm = merged_weight(ws, sm, off)
    xs = rnd(x, store).requires_grad_(True)
    wr = rnd(wm, store).requires_grad_(True)
    y = gathered_conv(xs, wr, mutant) if form == "gathered" else F.conv3d(xs, wr, None, stride=2, padding=3)
    out = y.detach()
    if bs is not None:
        out = out + ((sm[0] * bs[0] + sm[1] * bs[1]) + sm[2] * bs[2]).view(1, -1, 1, 1, 1)
    r = {"y": rnd(out, store)}
    if dy is None:
        return r
    dyr = rnd(dy.to(dtype), store)
    dx, dwm = torch.autograd.grad(y, [xs, wr], dyr)
    r["dx"], r["dwm"] = rnd(dx, store), dwm
    cs = dyr.sum((0, 2, 3, 4))
    dsm = []
    for j, k in enumerate(KS):
        r[f"dw{k}"] = (1.0 if mutant == "no_sm_dw" else sm[j]) * crop(dwm, k, off)
        d = (dwm * embed(ws[j], off)).sum()
        if bs is not None:
            r[f"db{k}"] = sm[j] * cs
            if mutant != "no_bias_share":
                d = d + (cs * bs[j]).sum()
        dsm.append(d)
    r["dsm"] = torch.stack(dsm)
    return r


def softmax_row_grad(row, dsm):
    """d(loss)/d(conv_arch row) from d(loss)/d(softmax(row))"""
    sm = torch.softmax(row.double(), -1)
    return sm * (dsm.double() - (sm * dsm.double()).sum())


# ------------------------------------------------------------------------------------------------ the additive upsample
def up_matrix(n, mutant=None, dtype=torch.float64):
    """[2n, n]: output 2i = 0.25 x[i-1] + 0.75 x[i], output 2i+1 = 0.75 x[i] + 0.25 x[i+1], indices clamped"""
    U = torch.zeros((2 * n, n), dtype=dtype)
    near, far = (0.25, 0.75) if mutant == "swapped_weights" else (0.75, 0.25)
    for o in range(2 * n):
        i = o // 2
        if mutant == "align_corners":
            s = o * (n - 1) / (2 * n - 1) if n > 1 else 0.0
            i0 = min(int(math.floor(s)), n - 1)
            i1 = min(i0 + 1, n - 1)
            U[o, i0] += 1 - (s - i0)
            U[o, i1] += s - i0
            continue
        j = i + 1 if o & 1 else i - 1
        U[o, i] += near
        if 0 <= j < n:
            U[o, j] += far
        elif mutant != "no_clamp":
            U[o, i] += far
    return U


def upsample_statement(x, dy=None, store=None, mutant=None, dtype=torch.float64):
    """dict(y, dx) of LinearAdditiveUpsample(2, 4, threed=True): x [N,C,D,H,W] -> y [N,C/4,2D,2H,2W]"""
    N, C, D, H, W = x.shape
    xs = rnd(x.to(dtype), store)
    xg = xs.view(N, 4, C // 4, D, H, W).sum(1) if mutant == "strided_groups" else xs.view(N, C // 4, 4, D, H, W).sum(2)
    Uz, Uy, Ux = (up_matrix(n, mutant, dtype) for n in (D, H, W))
    y = torch.einsum("ad,bh,cw,ngdhw->ngabc", Uz, Uy, Ux, xg)
    r = {"y": rnd(y, store)}
    if dy is None:
        return r
    dyr = rnd(dy.to(dtype), store)
    dg = torch.einsum("ad,bh,cw,ngabc->ngdhw", Uz, Uy, Ux, dyr)
    if mutant == "strided_groups":
        dx = dg.unsqueeze(1).expand(N, 4, C // 4, D, H, W).reshape(N, C, D, H, W)
    else:
        dx = dg.unsqueeze(2).expand(N, C // 4, 4, D, H, W)
        if mutant == "unequal_bwd":
            dx = dx * torch.tensor([1.0, 1.0, 1.0, 0.5], dtype=dtype).view(1, 1, 4, 1, 1, 1)
        dx = dx.reshape(N, C, D, H, W)
    r["dx"] = rnd(dx, store)
    return r


def torch_upsample(x):
    """the reference's own form: LinearAdditiveUpsample.forward"""
    r = F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=False)
    return torch.sum(torch.stack(torch.split(r, 4, dim=1), dim=1), dim=2)


# ------------------------------------------------------------------------------------------------ exact cases (kernels, zero tolerance)
# (C_in, C_out, N, (D, H, W)): one output voxel with 8 live taps; non-cubic with every border and a sample boundary; odd sizes; channel
# counts that are no multiple of 64; a long K (the split-K form); the image side with 1, 3 (batch 2) and 4 channels.
CELL_CASES = [(8, 8, 1, (2, 2, 2)), (8, 16, 2, (4, 6, 8)), (16, 8, 1, (5, 7, 6)), (24, 40, 1, (8, 8, 8)), (128, 8, 1, (4, 4, 4)),
              (1, 8, 1, (8, 8, 8)), (3, 16, 2, (4, 8, 6)), (4, 8, 1, (6, 4, 4))]
COFF_CASE = (8, 16, 2, (4, 6, 8))          # read again from channels 8..15 of a 32-channel buffer
SM_SETS = {"k4": (1.0, 0.0, 0.0), "k6": (0.0, 1.0, 0.0), "k8": (0.0, 0.0, 1.0), "mixed": (0.25, 0.25, 0.5)}
# (C, N, (D, H, W)): a single voxel; batch 2, non-cubic; odd sizes; three channel groups of 32
UP_CASES = [(32, 1, (1, 1, 1)), (32, 2, (2, 3, 4)), (64, 1, (3, 2, 5)), (96, 1, (4, 4, 4))]
UP_CONCAT_CASE = (64, 1, (3, 2, 5))        # written to channels 8..23 of a 40-channel buffer


def cell_id(c):
    return "c%dto%d_n%d_%dx%dx%d" % (c[0], c[1], c[2], *c[3])


def up_id(c):
    return "c%d_n%d_%dx%dx%d" % (c[0], c[1], *c[2])


def cell_build(case, smn):
    """integer operands: x in -8..8, |w| <= 3 (sm (1/4, 1/4, 1/2) leaves quarter-integers of at most 5 bits: exact in bf16), b in -4..4,
    dy in {-1, 0, 1} at the densest of 1, 1/2, 1/4, ... for which every sum the kernels form is an exact fp32 number in ANY order: the
    sums of the absolute values of the terms of y, dx and dWm stay below 2^24 in the unit of the values (1/4).  The three dot products
    <dWm, embed(W_j)> run over up to 512 C_in C_out terms and need a sparser gradient for the same guarantee: `dots` is the same case
    with dy at the densest such density (checked too: its weight and bias gradients)."""
    Cin, Cout, N, (D, H, W) = case
    g = er.generator(("cell3d", case, smn))
    x = torch.randint(-8, 9, (N, Cin, D, H, W), generator=g).float()
    ws = [torch.randint(-3, 4, (Cout, Cin, k, k, k), generator=g).float() for k in KS]
    bs = [torch.randint(-4, 5, (Cout,), generator=g).float() for _ in KS]
    sm = torch.tensor(SM_SETS[smn], dtype=torch.float32)
    shape = (N, Cout, D // 2, H // 2, W // 2)
    sign = (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    u = torch.rand(shape, generator=g)
    u.view(-1)[int(torch.randint(0, u.numel(), (1,), generator=g))] = 0.0          # never an all-zero gradient
    absw, absb = [w.abs() for w in ws], [b.abs() for b in bs]

    def densest(keys):
        for e in range(0, 13):
            dy = sign * (u < 0.5 ** e)
            a = cell_statement(x.abs(), absw, absb, torch.ones(3), dy.abs())
            if max(float(a[k].max()) for k in keys) * 4 < er.LIMIT:
                return dy, 0.5 ** e
        raise AssertionError(("no exact density for", case, smn, keys))

    dy, dens = densest(("y", "dx", "dwm"))
    dy2, dens2 = densest(("y", "dx", "dwm", "dsm"))
    r = cell_statement(x, ws, bs, sm, dy)
    r.update(x=x, ws=ws, bs=bs, sm=sm, dy=dy, density=dens, wm=merged_weight([w.double() for w in ws], sm.double()))
    r["dots"] = r if dens2 == dens else dict(cell_statement(x, ws, bs, sm, dy2), dy=dy2, density=dens2)
    return r


def up_build(case):
    """integers x in -8..8 and dy in -8..8: every weight is a multiple of 1/64, every sum has at most 64 terms: exact in fp32"""
    C, N, (D, H, W) = case
    g = er.generator(("upadd3d", case))
    x = torch.randint(-8, 9, (N, C, D, H, W), generator=g).float()
    dy = torch.randint(-8, 9, (N, C // 4, 2 * D, 2 * H, 2 * W), generator=g).float()
    r = upsample_statement(x, dy)
    r.update(x=x, dy=dy)
    return r


# ------------------------------------------------------------------------------------------------ module cases (the project's bound)
# (C_in, C_out, bias, N, (D, H, W), dtype, what runs): 'cell' = Cell_conv through networks3d.conv_arch, 'mixed' = MixedOp_conv with given
# weights, 'k4' / 'k6' / 'k8' = one primitive on its own.  Non-cubic volumes so that an exchanged axis shows.
MODULE_SEED = 31
MODULE_CASES = {
    "cell_img1_f16": (1, 16, True, 2, (8, 12, 10), "f16", "cell"),
    "cell_c16_bf16": (16, 24, True, 2, (6, 4, 8), "bf16", "cell"),
    "cell_c32_odd_nobias": (32, 8, False, 1, (5, 7, 6), "f16", "cell"),
    "mixed_c8_deep": (8, 16, True, 2, (2, 2, 2), "f16", "mixed"),
    "k4_c8": (8, 8, True, 1, (4, 6, 4), "f16", "k4"),
    "k6_img3": (3, 8, True, 1, (6, 4, 6), "f16", "k6"),
    "k8_c8_bf16": (8, 8, False, 2, (4, 4, 6), "bf16", "k8"),
}
UP_MODULE_CASES = {"up_c32_f16": (32, 2, (2, 3, 4), "f16"), "up_c64_bf16": (64, 1, (3, 2, 5), "bf16")}
LAYER_INDEX = 4


def module_inputs(cid):
    """(x, [w4, w6, w8], [b4, b6, b8] or None, conv_arch [6, 3], dy) of a module case: weights N(0, 1 / sqrt(fan_in)) (outputs of order one),
    arch rows of order one (mixing weights well apart from 1/3), dy of the size of a mean-loss gradient"""
    Cin, Cout, bias, N, (D, H, W), dtn, kind = MODULE_CASES[cid]
    g = torch.Generator().manual_seed(MODULE_SEED + sorted(MODULE_CASES).index(cid))
    x = torch.randn((N, Cin, D, H, W), generator=g)
    ws = [torch.randn((Cout, Cin, k, k, k), generator=g) * (Cin * k ** 3) ** -0.5 for k in KS]
    bs = [torch.randn((Cout,), generator=g) * 0.1 for _ in KS] if bias else None
    arch = torch.randn((6, 3), generator=g, dtype=torch.float64)
    shape = (N, Cout, D // 2, H // 2, W // 2)
    dy = (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) / math.prod(shape)
    return x, ws, bs, arch, dy


def module_sm(cid, arch):
    kind = MODULE_CASES[cid][6]
    if kind in ("cell", "mixed"):
        return torch.softmax(arch[LAYER_INDEX], -1)
    return torch.tensor([float(kind == "k4"), float(kind == "k6"), float(kind == "k8")], dtype=torch.float64)


def up_module_inputs(cid):
    C, N, (D, H, W), dtn = UP_MODULE_CASES[cid]
    g = torch.Generator().manual_seed(MODULE_SEED + 100 + sorted(UP_MODULE_CASES).index(cid))
    x = torch.randn((N, C, D, H, W), generator=g)
    shape = (N, C // 4, 2 * D, 2 * H, 2 * W)
    dy = (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) / math.prod(shape)
    return x, dy


def hold(got, r64, r16):
    """the project's bound (backward_replay.compare, d_U = 0: there is no activation in these operators): per tensor and per
    output-channel row, err <= 4 max(e16, FLOOR32 / 4) ... with the forward held to 4 max(e16, FLOOR32).  Returns (report, failures)."""
    keys = [k for k in r64 if k != "y"]
    rep, bad = compare({k: got[k] for k in keys}, {k: r64[k] for k in keys}, {k: r16[k] for k in keys}, {k: 0.0 for k in keys})
    n = float(r64["y"].norm())
    err = float((got["y"].double() - r64["y"]).norm()) / n
    e16 = float((r16["y"] - r64["y"]).norm()) / n
    rep["y"] = dict(err=err, e16=e16, ratio=err / max(e16, FLOOR32), bound=4 * max(e16, FLOOR32), ok=err <= 4 * max(e16, FLOOR32))
    if not rep["y"]["ok"]:
        bad.append("y")
    return rep, bad


# ------------------------------------------------------------------------------------------------ expected device tensors
def pack_fwd_expected(wm, dt0, nd):
    """[taps of the box][Co][8 Ci] in gathered channel order, tap (dtz,dty,dtx) row-major"""
    wg = gathered_weight(wm)
    b = wg[:, :, dt0[0] + 1:dt0[0] + 1 + nd[0], dt0[1] + 1:dt0[1] + 1 + nd[1], dt0[2] + 1:dt0[2] + 1 + nd[2]]
    return b.permute(2, 3, 4, 0, 1).reshape(-1, wg.shape[0], wg.shape[1]).contiguous()


def pack_dgrad_expected(wm, k0, nk, cin_pad):
    """[taps of the box][cin_pad][Co], rows ci >= Ci zero"""
    b = wm[:, :, k0[0]:k0[0] + nk[0], k0[1]:k0[1] + nk[1], k0[2]:k0[2] + nk[2]]
    b = b.permute(2, 3, 4, 1, 0).reshape(-1, wm.shape[1], wm.shape[0])
    return F.pad(b, (0, 0, 0, cin_pad - wm.shape[1])).contiguous()


# ------------------------------------------------------------------------------------------------ module references
def module_reference(cid, store=None, mutant=None, dtype=torch.float64, form="k8"):
    """what tests/test_cell3d_modules_gpu.py compares: y, dx, the gradients of the parameters the case has (w4 / w6 / w8, b4 / b6 / b8),
    and the gradient of the mixing weights -- 'darch' (the conv_arch row, through the softmax) for a Cell_conv, 'dsm' for a MixedOp_conv"""
    Cin, Cout, bias, N, vol, dtn, kind = MODULE_CASES[cid]
    x, ws, bs, arch, dy = module_inputs(cid)
    sm = module_sm(cid, arch)
    r = cell_statement(x, ws, bs, sm, dy, store=store, mutant=mutant, dtype=dtype, form=form)
    r.pop("dwm")
    dsm = r.pop("dsm").double()
    if kind == "cell":
        r["darch"] = softmax_row_grad(arch[LAYER_INDEX], dsm)
    elif kind == "mixed":
        r["dsm"] = dsm
    else:
        keep = kind[1]
        for k in KS:
            if str(k) != keep:
                r.pop(f"dw{k}")
                r.pop(f"db{k}", None)
    return {k: v.double() for k, v in r.items()}


def up_module_reference(cid, store=None, mutant=None, dtype=torch.float64):
    x, dy = up_module_inputs(cid)
    return {k: v.double() for k, v in upsample_statement(x, dy, store=store, mutant=mutant, dtype=dtype).items()}
