"""fp64 statements of the 3-D Pix2Pix generator (reference: GenSeg-3D/models/networks.py:604-728, `UnetGenerator` built from
`LinearUpsampleUnetSkipConnectionBlock`s with upsampling='linear') and of its image-side tail, the outermost block's
Conv3d(C_in -> C_out, k 3, s 1, p 1) + bias + Tanh (csrc/gen3d.hip); the exact cases of tests/test_gen3d_kernels_gpu.py, the cases of
tests/test_gen3d_networks_gpu.py and the list of mutants.  tests/test_gen3d_reference_cpu.py proves the statements against
torch.autograd through plain nn modules.  The cell and upsample statements, `hold` and the comparers are those of
tests/cell3d_reference.py.

The tail:  t = act(conv3d(x, w, pad 1) + b),  du = gscale * dout * (1 - t^2)  (act none: gscale * dout),
    dx = conv_transpose3d(du, w, pad 1)  (the flipped-tap sum),  dw = sum du * x(shifted),  db = sum du.
`store` (a 16-bit dtype) rounds what the engine stores in 16 bits: x and dx (the weights stay fp32 in the tail)."""
import math

import torch
import torch.nn.functional as F

from tests import cell3d_reference as c3
from tests import exact_reference as er
from tests.cell3d_reference import rnd

DT = c3.DT
TAIL_MUTANTS = ("tail_no_bias", "no_tanh_grad", "tail_unflipped", "tail_sample_leak")


# ------------------------------------------------------------------------------------------------ the tail
def tail_conv(x, w, b, mutant=None):
    """conv3d k3 / s1 / p1.  tail_sample_leak: the depth slices outside a sample are those of its neighbours in the [N*D] stack"""
    if mutant == "tail_sample_leak":
        N, C, D, H, W = x.shape
        flat = F.pad(x.permute(1, 0, 2, 3, 4).reshape(1, C, N * D, H, W), (1, 1, 1, 1, 1, 1))
        xp = torch.cat([flat[:, :, n * D:n * D + D + 2] for n in range(N)], 0)
        return F.conv3d(xp, w, b)
    return F.conv3d(x, w, b, padding=1)


def tail_statement(x, w, b, dout=None, act="tanh", gscale=1.0, store=None, mutant=None, t_given=None, dtype=torch.float64):
    """dict(t, [dx, dw, db]) of the tail for x [N,C_in,D,H,W], w [C_out,C_in,3,3,3], b [C_out] or None.  t_given: the tanh output to
    take the derivative at (the kernel's own t), instead of the statement's"""
    x, w = x.to(dtype), w.to(dtype)
    b = None if b is None or mutant == "tail_no_bias" else b.to(dtype)
    xs = rnd(x, store).requires_grad_(dout is not None)
    wr = w.clone().requires_grad_(dout is not None)
    pre = tail_conv(xs, wr, None, mutant)
    full = pre.detach() if b is None else pre.detach() + b.view(1, -1, 1, 1, 1)
    t = torch.tanh(full) if act == "tanh" else full
    r = {"t": t}
    if dout is None:
        return r
    tt = t if t_given is None else t_given.to(dtype)
    du = gscale * dout.to(dtype)
    if act == "tanh" and mutant != "no_tanh_grad":
        du = du * (1 - tt * tt)
    if mutant == "tail_unflipped":
        dw = torch.autograd.grad(pre, wr, du)[0]
        dx = F.conv3d(du, w.transpose(0, 1), None, padding=1)
    else:
        dx, dw = torch.autograd.grad(pre, [xs, wr], du)
    r.update(dx=rnd(dx, store), dw=dw, db=du.sum((0, 2, 3, 4)), du=du)
    return r


# (C_in, C_out, N, (D, H, W)): only the centre tap meets data; every border at once; a sample boundary with planted voxels on the last
# slice of sample 0 and the first of sample 1; a volume that crosses the 8 x 32 tile edge in both plane axes (and two channel chunks of
# the forward: 32 + 8); the widest form; a one-row plane wider than a tile.
TAIL_CASES = [(8, 1, 1, (1, 1, 1)), (8, 4, 2, (2, 2, 2)), (16, 3, 2, (2, 3, 5)), (40, 2, 1, (3, 17, 33)), (64, 4, 1, (4, 8, 8)),
              (32, 1, 1, (5, 1, 40))]
TAIL_GSCALE = 2.0


def tail_id(c):
    return "c%dto%d_n%d_%dx%dx%d" % (c[0], c[1], c[2], *c[3])


def tail_build(case):
    """integer operands: x in -8..8, w in -3..3, b in -4..4, dout in {-1, 0, 1} at the densest of 1, 1/2, 1/4 ... for which the sums
    of the absolute values of the terms of t, dx, dw and db stay below 2^24: every fp32 sum is then exact in ANY order."""
    Cin, Cout, N, (D, H, W) = case
    g = er.generator(("tail3d", case))
    x = torch.randint(-8, 9, (N, Cin, D, H, W), generator=g).float()
    if N > 1:                                                         # a leak across the sample boundary must show
        x[0, :, D - 1, H // 2, W // 2] = 8.0
        x[1, :, 0, H // 2, W // 2] = -8.0
    w = torch.randint(-3, 4, (Cout, Cin, 3, 3, 3), generator=g).float()
    w[:, :, 0] += (w[:, :, 0] == 0).float()                           # no zero tap in the kz planes that would reach a neighbour
    w[:, :, 2] -= (w[:, :, 2] == 0).float()
    b = torch.randint(-4, 5, (Cout,), generator=g).float()
    shape = (N, Cout, D, H, W)
    sign = (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    u = torch.rand(shape, generator=g)
    u.view(-1)[int(torch.randint(0, u.numel(), (1,), generator=g))] = 0.0
    if N > 1:
        u[0, :, D - 1, H // 2, W // 2] = 0.0
        u[1, :, 0, H // 2, W // 2] = 0.0
    for e in range(0, 13):
        dout = sign * (u < 0.5 ** e)
        a = tail_statement(x.abs(), w.abs(), b.abs(), dout.abs(), act="none", gscale=TAIL_GSCALE)
        if max(float(a[k].max()) for k in ("t", "dx", "dw", "db")) < er.LIMIT:
            break
    else:
        raise AssertionError(("no exact density for", case))
    r = tail_statement(x, w, b, dout, act="none", gscale=TAIL_GSCALE)
    r.update(x=x, w=w, b=b, dout=dout, density=0.5 ** e)
    return r


def tail_tanh_inputs(case):
    """dyadic operands whose pre-activation is an exact fp32 number of order one: integers x in -8..8 and w in -3..3 times a power of
    two near 1 / (10 sqrt(27 C_in)), b in quarters; dout of order one"""
    Cin, Cout, N, (D, H, W) = case
    g = er.generator(("tail3d_tanh", case))
    x = torch.randint(-8, 9, (N, Cin, D, H, W), generator=g).float()
    s = 2.0 ** -round(math.log2(10 * math.sqrt(27 * Cin)))
    w = torch.randint(-3, 4, (Cout, Cin, 3, 3, 3), generator=g).float() * s
    b = torch.randint(-4, 5, (Cout,), generator=g).float() / 4
    dout = torch.randn((N, Cout, D, H, W), generator=g)
    return x, w, b, dout


# ------------------------------------------------------------------------------------------------ the whole generator
# The statement is the reference's forward written out over plain tensors in fp64 (one 8x8x8 conv per cell by linearity, the upsample as
# three interpolation matrices, the norms by their definition), differentiated by torch.autograd: ReLU'(0) = 0, LeakyReLU'(0) = 0.2,
# keep masks times 2, and a BatchNorm on running statistics has no gradient through mean and variance (c1 = c2 = 0) -- the plan's
# conventions.  `store` rounds every tensor the engine keeps in 16 bits where it is stored, forward and (times the loss scale S, as
# the engine carries them) backward.  Mutants are the wrong plans tests/test_gen3d_reference_cpu.py holds the bound against.
GEN_MUTANTS = ("no_up_relu", "skip_leaky", "halves_swapped", "layer_index_outside", "innermost_norm", "tail_no_bias", "no_tanh_grad",
               "up_unflipped", "tail_sample_leak", "keep_factor", "eval_c12", "strided_groups")
BN_EPS = 1e-5


class _Store(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, dt, S):
        ctx.dt, ctx.S = dt, S
        return rnd(t, dt)

    @staticmethod
    def backward(ctx, g):
        return rnd(g * ctx.S, ctx.dt) / ctx.S, None, None


class _Conv3Unflipped(torch.autograd.Function):
    """conv3d k3 / p1 whose data gradient forgets to flip the taps (mutant)"""
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return F.conv3d(x, w, None, padding=1)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        with torch.enable_grad():
            ww = w.detach().requires_grad_(True)
            dw = torch.autograd.grad(F.conv3d(x.detach(), ww, None, padding=1), ww, g)[0]
        return F.conv3d(g, w.transpose(0, 1), None, padding=1), dw


class _TanhNoGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return torch.tanh(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _EvalNormC12(torch.autograd.Function):
    """BatchNorm on running statistics whose backward keeps the c1 / c2 terms of batch statistics (mutant)"""
    @staticmethod
    def forward(ctx, y, mean, invstd):
        xh = (y - mean) * invstd
        ctx.save_for_backward(xh, invstd)
        return xh

    @staticmethod
    def backward(ctx, g):
        xh, invstd = ctx.saved_tensors
        dims = (0, 2, 3, 4)
        return invstd * (g - g.mean(dims, keepdim=True) - xh * (g * xh).mean(dims, keepdim=True)), None, None


def _up(x, mutant=None):
    """LinearAdditiveUpsample(2, 4, threed=True), differentiable (cell3d_reference.upsample_statement's forward)"""
    N, C, D, H, W = x.shape
    xg = x.view(N, 4, C // 4, D, H, W).sum(1) if mutant == "strided_groups" else x.view(N, C // 4, 4, D, H, W).sum(2)
    Uz, Uy, Ux = (c3.up_matrix(n, None, x.dtype) for n in (D, H, W))
    y = torch.einsum("ad,ngdhw->ngahw", Uz, xg)               # one axis at a time: the joint contraction asks einsum for 64 GB at 64^3
    y = torch.einsum("bh,ngahw->ngabw", Uy, y)
    return torch.einsum("cw,ngabw->ngabc", Ux, y)


def generator_statement(f, sd, arch, x, dense=None, masks=None, store=None, mutant=None, train=None, dtype=torch.float64):
    """dict(y, [dx, darch, grads {key: tensor}]) of UnetGenerator(**f) with state dict sd on x, for loss = sum(y * dense).
    f: dict(input_nc, output_nc, num_downs, ngf, norm, use_dropout[, train]) (golden_util_gen3d's fixture form); masks: keep masks
    [N,C,D,H,W] of the dropout blocks, innermost first (train mode with dropout)."""
    from golden_util_gen3d import block_layout, block_prefix, channels
    train = f.get("train", True) if train is None else train
    nd, c = f["num_downs"], channels(f)
    inst = f["norm"] == "instance"
    N = x.shape[0]
    S = float(2 ** round(math.log2(N * x.shape[2] * x.shape[3] * x.shape[4])))
    P = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    run = {k: v.detach().to(dtype) for k, v in sd.items() if "running" in k}
    arch = arch.detach().to(dtype).requires_grad_(True)
    x = x.detach().to(dtype).requires_grad_(True)

    def st(t):
        return t if store is None else _Store.apply(t, store, S)

    def norm(y, key, eval_c12_ok=True):
        if inst or key is None:
            dims = (2, 3, 4)
            m, v = y.mean(dims, keepdim=True), y.var(dims, unbiased=False, keepdim=True)
            return (y - m) / torch.sqrt(v + BN_EPS)
        g, b = P[key + ".weight"].view(1, -1, 1, 1, 1), P[key + ".bias"].view(1, -1, 1, 1, 1)
        if train:
            dims = (0, 2, 3, 4)
            m, v = y.mean(dims, keepdim=True), y.var(dims, unbiased=False, keepdim=True)
            return (y - m) / torch.sqrt(v + BN_EPS) * g + b
        m, inv = run[key + ".running_mean"].view(1, -1, 1, 1, 1), 1 / torch.sqrt(run[key + ".running_var"].view(1, -1, 1, 1, 1) + BN_EPS)
        if mutant == "eval_c12":
            return _EvalNormC12.apply(y, m, inv) * g + b
        return (y - m) * inv * g + b

    def cell(inp, d):
        p, lay = block_prefix(d), block_layout(f, d)
        li = d if mutant == "layer_index_outside" else nd - 1 - d
        sm = torch.softmax(arch[li], -1)
        ws = [P[f"{p}{lay['cell']}._ops._ops.{j}.op.weight"] for j in range(3)]
        y = F.conv3d(st(inp) if d == 0 else inp, st(c3.merged_weight(ws, sm)), None, stride=2, padding=3)
        if inst:                                        # in front of a norm the bias cancels: gradient exact zeros
            bs = [P[f"{p}{lay['cell']}._ops._ops.{j}.op.bias"] for j in range(3)]
            y = y + ((sm[0] * bs[0] + sm[1] * bs[1]) + sm[2] * bs[2]).view(1, -1, 1, 1, 1) * (1.0 if lay["downnorm"] is None else 0.0)
        return st(y)

    mask_i = [0]

    def block(a_in, d):
        """a_in: the block's input after the in-place LeakyReLU (the image for d = 0).  Returns what the parent's uprelu sees."""
        p, lay = block_prefix(d), block_layout(f, d)
        y = cell(a_in, d)
        if d == nd - 1:
            if mutant == "innermost_norm":
                y = norm(y, None)
            inner = y if mutant == "no_up_relu" else st(torch.relu(y))
        else:
            z = norm(y, None if inst else f"{p}{lay['downnorm']}") if lay["downnorm"] is not None else y
            leaky = st(F.leaky_relu(z, 0.2))
            sub = block(leaky, d + 1)                          # [relu'd or not]: the second half, pre-ReLU
            skip = leaky if mutant in ("skip_leaky", "no_up_relu") else st(torch.relu(z))
            up = sub if mutant == "no_up_relu" else st(torch.relu(sub))
            inner = torch.cat([up, skip], 1) if mutant == "halves_swapped" else torch.cat([skip, up], 1)
        v = st(_up(inner, mutant))
        w, b = P[f"{p}{lay['upconv']}.weight"], P[f"{p}{lay['upconv']}.bias"]
        if d == 0:
            tm = mutant if mutant in ("tail_sample_leak",) else None
            pre = tail_conv(v, w, None if mutant == "tail_no_bias" else b, tm)
            return _TanhNoGrad.apply(pre) if mutant == "no_tanh_grad" else torch.tanh(pre)
        u = _Conv3Unflipped.apply(v, st(w)) if mutant == "up_unflipped" else F.conv3d(v, st(w), None, padding=1)
        # in front of batch / instance statistics the bias cancels (gradient exact zeros); on running statistics it does not
        u = st(u) + b.view(1, -1, 1, 1, 1) * (1.0 if (not inst and not train) else 0.0)
        z = norm(u, None if inst else f"{p}{lay['upnorm']}")
        if lay["drop"] is not None and train:
            keep = masks[mask_i[0]].to(dtype)
            mask_i[0] += 1
            z = z * keep * (1.0 if mutant == "keep_factor" else 2.0)
        return z

    y = block(x, 0)
    r = {"y": y.detach()}
    if dense is None:
        return r
    keys = list(P)
    grads = torch.autograd.grad((y * dense.to(dtype)).sum(), [x, arch] + [P[k] for k in keys], allow_unused=True)
    r["dx"] = grads[0]
    r["darch"] = grads[1] if grads[1] is not None else torch.zeros_like(arch)
    r["grads"] = {k: (g if g is not None else torch.zeros_like(P[k])) for k, g in zip(keys, grads[2:])}
    return r


def flat(r):
    """{y, dx, darch, g/<key>...}: what the comparers walk"""
    out = {"y": r["y"], "dx": r["dx"], "darch": r["darch"]}
    out.update({"g/" + k: v for k, v in r["grads"].items()})
    return out


# ------------------------------------------------------------------------------------------------ network cases (the project's bound)
# The three fixture networks (four parts: BatchNorm3d in train and eval mode), one bf16 case, one train-mode dropout case with given
# keep masks.  Seeds: the fixtures' own; d_U is taken as 0 in the bound (no slack is claimed for undecided ReLU signs).
def _fixture(tag):
    from golden_util_gen3d import FIXTURES
    return next(f for f in FIXTURES["pix2pix3d_gen"] if f["tag"] == tag)


def net_cases():
    c = {t: dict(_fixture(t), dtype="f16") for t in ("bn5_train", "bn5_eval", "in5_rgb", "bn6_drop_eval")}
    c["in5_bf16"] = dict(_fixture("in5_rgb"), tag="in5_bf16", dtype="bf16", H=32, input_nc=1, output_nc=2, seed=94)
    c["bn6_drop_train"] = dict(_fixture("bn6_drop_eval"), tag="bn6_drop_train", dtype="f16", train=True, seed=95)
    return c


NET_CASE_IDS = ("bn5_train", "bn5_eval", "in5_rgb", "bn6_drop_eval", "in5_bf16", "bn6_drop_train")


def case_inputs(cid):
    """(f, state dict, conv_arch, x, dense, keep masks [N,C,D,H,W] innermost first or None)"""
    from golden_util_gen3d import channels, fixture_arch, fixture_dense, fixture_input, fixture_state_dict
    f = net_cases()[cid]
    masks = None
    if f["use_dropout"] and f["train"]:
        g = torch.Generator().manual_seed(f["seed"] + 4)
        c, nd = channels(f), f["num_downs"]
        masks = [(torch.rand((f["N"], c[d], f["D"] >> d, f["H"] >> d, f["W"] >> d), generator=g) >= 0.5).to(torch.uint8)
                 for d in range(nd - 2, 3, -1)]
    return f, fixture_state_dict(f), fixture_arch(f), fixture_input(f), fixture_dense(f), masks


_REF = {}


def case_reference(cid, store=None, mutant=None, dtype=torch.float64):
    """the flat statement of a case, computed once per (case, store, mutant, dtype) and shared (never modified)"""
    key = (cid, store, mutant, dtype)
    if key not in _REF:
        f, sd, arch, x, dense, masks = case_inputs(cid)
        # fp32: ATen's own conv kernels (the oneDNN fp32 Conv3d weight gradient returned NaNs for one channel pair of a k8 cell)
        with torch.backends.mkldnn.flags(enabled=dtype != torch.float32):
            r = flat(generator_statement(f, sd, arch, x, dense, masks, store=store, mutant=mutant, dtype=dtype))
        assert all(bool(torch.isfinite(v).all()) for v in r.values()), "the statement must be finite"
        _REF[key] = {k: v.double() for k, v in r.items()}
    return _REF[key]


def gen_hold(got, r64, r16):
    """cell3d_reference.hold over the tensors whose reference is not identically zero (the image held to 4 max(e16, FLOOR32), every
    gradient per tensor and per output-channel row to 4 max(e16, FLOOR32 / 4), d_U = 0); the others -- a bias cancelled by the norm
    behind it -- must be exact zeros.  Returns (report, failures)."""
    live = [k for k in r64 if float(r64[k].abs().max()) > 0.0]
    rep, bad = c3.hold({k: got[k] for k in live}, {k: r64[k] for k in live}, {k: r16[k] for k in live})
    for k in r64:
        if k not in live and float(got[k].double().abs().max()) != 0.0:
            bad.append(k + " (must be exact zeros)")
    return rep, bad


def worst(rep):
    k = max(rep, key=lambda n: max(rep[n]["ratio"] / 4, rep[n].get("row_worst", 0.0)))
    return k, rep[k]
