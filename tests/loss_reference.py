"""fp64 statements of the loss heads of csrc/loss.hip, the case lists of their tests, and the comparer.  Shared by
tests/test_loss_reference_cpu.py (the statements agree with the oracle, with torch's own criteria and with the recorded reference
values; the comparer rejects planted errors) and tests/test_loss_kernels_gpu.py (every kernel against these statements).  Plain
torch on the CPU; no GPU, no native library.

The statements follow the contract of include/gsseg.h and the reference lines cited there (running_files/train_end2end_jsrt.py:
136-138,181-183; util/dice_score.py:5-28; running_files/train_end2end_isic.py:40-56,247-249; models_pix2pix/networks.py:263-281):
whole-tensor expressions in float64 and the analytic derivative of each, written down from the mathematics -- d BCE / dx =
sigmoid(x) - t also AT x == 0, where autograd through max(x, 0) and |x| gives a one-sided value; d|x - t|/dx = sign(x - t), 0 at a
tie.  Mask values >= C (C > 1), or > 1 (C == 1), are outside the contract: the statements raise.

Every statement takes `fault=`: a named, deliberate error (FAULTS) used only by the CPU test, which proves that the comparer
rejects each of them.

Bounds.  Counts, sums of integer-valued operands and the L1 gradient are compared exactly.  Every other figure is allowed
4 * e32 + 2^-22, where e32 is the error of an fp32 evaluation of the same operation on the CPU (`*_fp32` below: the oracle's
expressions under fp32 autograd) against the fp64 statement, on the same scale: values relative to max(1, |ref|), gradients per
element relative to max |ref grad|.  Four times: the kernel's per-thread, wave and block fp32 partials, finished in double, are no
worse than torch's fp32 sums, and the device's expf / logf / log1pf may each be an ulp or two wider than the host's.  No value
bound exceeds 2e-6.  The fp32 evaluation takes BCE from torch's binary_cross_entropy_with_logits, not from the oracle's
max(x, 0) - x t + log1p(exp(-|x|)): the two agree in value, but autograd gives the oracle's form the derivative 1 - t at x == 0,
and the planted logits hold exact zeros."""
import torch
import torch.nn.functional as F

from tests import exact_reference as E

EPS = 1e-6                                           # dice_score.py:5
FLOOR = 2.0 ** -22
VALUE_CAP = 2e-6                                     # what tests/test_gpu_kernels.py::test_seg_loss_matches_oracle asserts
FACTOR = 4.0
FAULTS = ("no_eps", "drop_pixel", "swap_class", "gscale_twice", "l1_tie_plus")

# ---------------------------------------------------------------------------------------------------------------- case lists
# forward: min(1024, ceil(pixels / 1024)) blocks of 256 threads -- capped above 1 048 576 pixels; backward: min(4096, ceil(pixels /
# 256)) -- capped above the same count.  Per-sample heads: min(16, ceil(HW / 2048)) blocks -- capped above 32 768; the Jaccard
# backward min(256, ceil(HW / 1024)) -- capped above 262 144.
SEG_SHAPES = {"one": (1, 1, 1), "ragged": (3, 37, 29), "capped": (1, 1031, 1021)}            # (N, H, W)
SEG_CLASSES = {"one": (1, 2, 3, 4, 5, 9), "ragged": (1, 2, 3, 4, 5, 9, 64), "capped": (1, 3)}
FAMILIES = ("n2", "n30", "planted")
MASKS = ("random", "background", "one_class")
SEG_CASES = [(s, C, f, m) for s in SEG_SHAPES for C in SEG_CLASSES[s] for f in FAMILIES for m in MASKS]
EPS_CASES = [(1, 1, 1), (1, 1, 3), (1, 2, 2)]                                                # (N, H, W): at most 4 pixels, C = 1
SCALARS = [(gout, gscale, world) for world in (1, 4) for gout in (None, 3.0) for gscale in (1.0, 1.0 / 1024)]
SCALARS_CAPPED = [(None, 1.0, 1), (3.0, 1.0 / 1024, 1), (None, 1.0 / 1024, 4), (3.0, 1.0, 4)]  # every value of each, in four runs
WORLD_SHAPE = (3, 37, 29)                            # the three other ranks of the world-of-four cases hold batches of this shape

JACCARD_SHAPES = {"one": (1, 1, 1), "ragged": (3, 37, 29), "item_cap": (3, 191, 173), "bwd_cap": (1, 521, 509)}
JACCARD_CASES = [(s, f, m) for s in JACCARD_SHAPES for f in FAMILIES for m in MASKS]
JACCARD_SCALARS = [(None, 1.0), (3.0, 1.0), (None, 1.0 / 1024), (3.0, 1.0 / 1024)]

MEAN_N = (1, 255, 257, 4099, 1052651)
MEAN_CVAL = (0.0, 1.0, 0.9, -1.0)
MEAN_MODES = (0, 1, 2, 3, 4)                         # BCE vs constant, MSE vs constant, mean(x) * cval, L1, BCE vs tensor
MEAN_FAMILIES = ("n2", "planted")
MEAN_SCALARS = JACCARD_SCALARS
TIE_SHARE = 0.10                                     # L1: share of elements with x == t

DICE_N = MEAN_N
DICE_KINDS = ("prob", "integer", "zero", "opposite")  # sigmoid outputs vs {0,1}; integers in [-8, 8]; p = t = 0; p = -t (sets == 0)
DICE_BATCHED_SHAPE = (3, 191 * 173)


def case_id(case):
    return "-".join(str(c) for c in case)


def draw_logits(g, shape, family):
    x = 2.0 * torch.randn(shape, generator=g)
    if family == "n30":
        x = 15.0 * x
    elif family == "planted":
        f = x.view(-1)
        f[0::7] = 100.0
        f[1::11] = -100.0
        f[2::13] = 0.0
    elif family != "n2":
        raise ValueError(family)
    return x


def draw_mask(g, N, C, H, W, kind):
    if kind == "random":
        return torch.randint(0, max(C, 2), (N, H, W), generator=g).to(torch.uint8)
    if kind == "background":
        return torch.zeros(N, H, W, dtype=torch.uint8)
    if kind == "one_class":
        return torch.full((N, H, W), 1 if C <= 2 else C - 1, dtype=torch.uint8)
    raise ValueError(kind)


def seg_case(case):
    """logits fp32 [N,C,H,W], mask uint8 [N,H,W], others: the summed (2 sum p t, sum p, sum t) of the three other ranks, fp64 [3]"""
    shape, C, family, mkind = case
    N, H, W = SEG_SHAPES[shape]
    g = E.generator(("seg_loss",) + tuple(case))
    x = draw_logits(g, (N, C, H, W), family)
    m = draw_mask(g, N, C, H, W, mkind)
    others = torch.zeros(3, dtype=torch.float64)
    for _ in range(3):
        xo = draw_logits(g, (WORLD_SHAPE[0], C) + WORLD_SHAPE[1:], "n2")
        mo = draw_mask(g, WORLD_SHAPE[0], C, WORLD_SHAPE[1], WORLD_SHAPE[2], "random")
        others += seg_loss(xo, mo)["out"][3:6]
    return x, m, others


def eps_case(shape):
    """the eps-dominated case: one class, all background, logits about -14: sum p is a few 1e-6 and EPS decides the Dice value"""
    N, H, W = shape
    g = E.generator(("seg_loss_eps",) + tuple(shape))
    x = -14.0 + 0.25 * torch.randn(N, 1, H, W, generator=g)
    return x, torch.zeros(N, H, W, dtype=torch.uint8)


def jaccard_case(case):
    shape, family, mkind = case
    N, H, W = JACCARD_SHAPES[shape]
    g = E.generator(("jaccard",) + tuple(case))
    return draw_logits(g, (N, 1, H, W), family), draw_mask(g, N, 1, H, W, mkind)


def mean_case(mode, n, family):
    """x, t fp32 [n] (t None for the constant-label modes).  L1: t is another draw with x copied over TIE_SHARE of it."""
    g = E.generator(("mean_loss", mode, n, family))
    x = draw_logits(g, (n,), family)
    t = None
    if mode == 3:
        t = draw_logits(g, (n,), "n2")                # nothing planted: the only ties are the deliberate ones
        tie = torch.rand(n, generator=g) < TIE_SHARE
        tie[0] = n > 1                                # at least one tie, except where the single element has to carry a sign
        t = torch.where(tie, x, t)
    elif mode == 4:
        t = (torch.rand(n, generator=g) > 0.5).float()
    return x, t


def mean_case_integer(mode, n):
    """integer-valued operands in [-8, 8]: every fp32 partial sum of modes 1, 2, 3 is exact (cval an integer too)"""
    g = E.generator(("mean_loss_int", mode, n))
    x = torch.randint(-8, 9, (n,), generator=g).float()
    t = torch.randint(-8, 9, (n,), generator=g).float() if mode == 3 else None
    return x, t


def dice_case(kind, n):
    g = E.generator(("dice_loss", kind, n))
    if kind == "prob":
        return torch.sigmoid(2.0 * torch.randn(n, generator=g)), (torch.rand(n, generator=g) > 0.5).float()
    if kind == "integer":
        return torch.randint(-8, 9, (n,), generator=g).float(), torch.randint(-8, 9, (n,), generator=g).float()
    if kind == "zero":
        return torch.zeros(n), torch.zeros(n)
    if kind == "opposite":                            # sum p + sum t == 0 exactly with nonzero operands: dice_score.py:14
        t = torch.randint(1, 9, (n,), generator=g).float()
        return -t, t
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------- fp64 statements
def _g(gout, gscale, fault):
    g = (1.0 if gout is None else float(gout)) * float(gscale)
    return g * float(gscale) if fault == "gscale_twice" else g


def _sigmoid(v):
    return 1.0 / (1.0 + torch.exp(-v))


def _bce_terms(v, t):
    return v.clamp(min=0) - v * t + torch.log1p(torch.exp(-v.abs()))


def _dice(inter, sets, eps):
    """dice_score.py:12-16 on the sums: returns (dice, degenerate)"""
    degenerate = bool(sets == 0)
    if degenerate:
        sets = inter
    return (inter + eps) / (sets + eps), degenerate


def _check_mask(m, C):
    hi = 1 if C == 1 else C - 1
    if int(m.max()) > hi:
        raise ValueError(f"mask value {int(m.max())} is outside the contract of {C} classes")


def _last_foreground(m):
    """flat index of the pixel the "drop_pixel" fault omits: the last foreground pixel (the last pixel if there is none)"""
    fg = m.reshape(-1).nonzero()
    return int(fg[-1]) if fg.numel() else m.numel() - 1


def seg_loss(logits, mask, gout=None, gscale=1.0, others=None, world=1, fault=None):
    """gs_seg_loss_fwd / _bwd: {"out": fp64 [8], "grad": fp64 [N,C,H,W]}.  `others`: (2 sum p t, sum p, sum t) summed over the other
    ranks, with `world` the number of ranks: out[3..5] are then the global sums, out[2] and out[0] use the global Dice and the Dice part
    of the gradient is multiplied by `world` (losses.apply_global_dice; the gradient AVERAGE over the ranks is then that of the global
    loss)."""
    x = logits.double()
    N, C, H, W = x.shape
    m = mask.reshape(N, H, W).long()
    _check_mask(m, C)
    npix = N * H * W
    keep = torch.ones(N, 1, H, W, dtype=torch.float64)
    if fault == "drop_pixel":
        keep.view(-1)[_last_foreground(m)] = 0.0
    if fault == "swap_class":
        m = m.clone()
        k = npix // 2
        m.view(-1)[k] = (m.view(-1)[k] + 1) % max(C, 2)
    if C == 1:
        T = m.double().unsqueeze(1)
        P = _sigmoid(x)
        crit_terms = _bce_terms(x, T)                                            # BCEWithLogitsLoss, train_end2end_jsrt.py:136
    else:
        T = F.one_hot(m, C).permute(0, 3, 1, 2).double()
        z = x - x.max(dim=1, keepdim=True).values
        den = torch.exp(z).sum(dim=1, keepdim=True)
        P = torch.exp(z) / den
        crit_terms = torch.log(den) - (z * T).sum(dim=1, keepdim=True)           # CrossEntropyLoss: lse(x) - x_t
    crit = (crit_terms * keep).sum() / npix
    sums = torch.stack([2.0 * (P * T * keep).sum(), (P * keep).sum(), (T * keep).sum()])
    if others is not None:
        sums = sums + others.double()
    inter, sp, st = sums[0], sums[1], sums[2]
    eps = 0.0 if fault == "no_eps" else EPS
    dice, degenerate = _dice(inter, sp + st, eps)
    out = torch.stack([crit + (1.0 - dice), crit, 1.0 - dice, inter, sp, st,
                       torch.tensor(float(world), dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)])
    # d(1 - dice)/dP = -(2 T (S + eps) - (I + eps)) / (S + eps)^2; with sets == 0 the coefficient is (I + eps)/(I + eps): constant
    S = sp + st
    gP = torch.zeros_like(P) if degenerate else -(2.0 * T * (S + eps) - (inter + eps)) / (S + eps) ** 2
    if C == 1:
        dd = gP * P * (1.0 - P)
    else:
        dd = P * (gP - (P * gP).sum(dim=1, keepdim=True))
    grad = _g(gout, gscale, fault) * ((P - T) / npix + float(world) * dd) * keep
    return {"out": out, "grad": grad}


def dice_loss(p, t, gout=None, fault=None):
    """gs_dice_loss_fwd / _bwd (dice_score.py:25-28, one global sum): {"out": [loss, 2 sum p t, sum p, sum t], "grad": d loss / dp}"""
    a, b = p.double().reshape(-1), t.double().reshape(-1)
    inter, sp, st = 2.0 * (a * b).sum(), a.sum(), b.sum()
    eps = 0.0 if fault == "no_eps" else EPS
    dice, degenerate = _dice(inter, sp + st, eps)
    S = sp + st
    g = 1.0 if gout is None else float(gout)
    grad = torch.zeros_like(a) if degenerate else -g * (2.0 * b * (S + eps) - (inter + eps)) / (S + eps) ** 2
    return {"out": torch.stack([1.0 - dice, inter, sp, st]), "grad": grad.reshape(p.shape)}


def dice_coeff_batched(p, t, dtype=torch.float64):
    """gs_dice_coeff_batched (dice_score.py:5-17, reduce_batch_first=False): [1 + B] = mean, dice_b (dtype float32: the fp32 evaluation)"""
    a, b = p.to(dtype), t.to(dtype)
    inter, sets = 2.0 * (a * b).sum(dim=1), a.sum(dim=1) + b.sum(dim=1)
    sets = torch.where(sets == 0, inter, sets)
    d = (inter + EPS) / (sets + EPS)
    return torch.cat([d.mean().reshape(1), d])


def jaccard_seg_loss(logits, mask, gout=None, gscale=1.0, fault=None):
    """gs_jaccard_seg_loss_fwd / _bwd (train_end2end_isic.py:40-56,247-249): out fp64 [4 + 2N] = loss, bce, 1 - mean jac, 0, (I_i, S_i)"""
    x = logits.double()
    N, C, H, W = x.shape
    if C != 1:
        raise ValueError("the Jaccard loss is the one-class form")
    m = mask.reshape(N, 1, H, W).long()
    _check_mask(m, 1)
    T = m.double()
    keep = torch.ones_like(x)
    if fault == "drop_pixel":
        keep.view(-1)[_last_foreground(m)] = 0.0
    if fault == "swap_class":
        T = T.clone()
        k = x.numel() // 2
        T.view(-1)[k] = 1.0 - T.view(-1)[k]
    P = _sigmoid(x)
    bce = (_bce_terms(x, T) * keep).sum() / x.numel()
    I = (P * T * keep).sum(dim=(1, 2, 3))                                        # |t p| = t p: both are non-negative
    S = ((P + T) * keep).sum(dim=(1, 2, 3))
    D = S - I + 1.0                                                              # smooth = 1
    jac = (I + 1.0) / D
    ljac = 1.0 - jac.mean()
    out = torch.cat([torch.stack([bce + ljac, bce, ljac, torch.tensor(0.0, dtype=torch.float64)]),
                     torch.stack([I, S], dim=1).reshape(-1)])
    # jac_n = (I + 1) / (S - I + 1): d/dp = [t D - (I + 1)(1 - t)] / D^2
    Dn, In = D.view(N, 1, 1, 1), I.view(N, 1, 1, 1)
    djac = (T * Dn - (In + 1.0) * (1.0 - T)) / Dn ** 2
    grad = _g(gout, gscale, fault) * ((P - T) / x.numel() - P * (1.0 - P) * djac / N) * keep
    return {"out": out, "grad": grad}


def mean_loss(x, t, cval, mode, gout=None, gscale=1.0, fault=None):
    """gs_mean_loss_fwd / _bwd: {"out": fp64 [1], "grad": fp64 like x}"""
    v = x.double()
    c = float(torch.tensor(cval, dtype=torch.float32))                           # the entry point takes cval as a float
    tt = None if t is None else t.double()
    if mode in (3, 4) and tt is None:
        raise ValueError(f"mode {mode} needs a target tensor")
    if mode == 0:                                                                # GANLoss vanilla, networks.py:263-281
        terms, d = _bce_terms(v, torch.full_like(v, c)), _sigmoid(v) - c
    elif mode == 1:                                                              # lsgan
        terms, d = (v - c) ** 2, 2.0 * (v - c)
    elif mode == 2:                                                              # wgangp: mean(x) * (+-1)
        terms, d = v * c, torch.full_like(v, c)
    elif mode == 3:                                                              # L1Loss, train_end2end_jsrt.py:138
        terms, d = (v - tt).abs(), torch.sign(v - tt)
        if fault == "l1_tie_plus":
            d = torch.where(v == tt, torch.ones_like(d), d)
    elif mode == 4:                                                              # BCEWithLogitsLoss vs a tensor
        terms, d = _bce_terms(v, tt), _sigmoid(v) - tt
    else:
        raise ValueError(mode)
    n = v.numel()
    return {"out": (terms.sum() / n).reshape(1), "grad": _g(gout, gscale, fault) * d / n}


def l1_grad_exact(x, t, gout, gscale):
    """the L1 gradient as the contract states it, in fp32: +-float32(float32(gout * gscale) / float32(n)), 0 at a tie"""
    g = torch.tensor(1.0 if gout is None else gout, dtype=torch.float32) * torch.tensor(gscale, dtype=torch.float32)
    g = g / torch.tensor(float(x.numel()), dtype=torch.float32)
    return g * torch.sign(x.float() - t.float())


# ---------------------------------------------------------------------------------------------------------------- fp32 evaluations
def _leaf32(x):
    return x.detach().clone().float().requires_grad_(True)


def _g32(gout, gscale):
    return (1.0 if gout is None else float(gout)) * float(gscale)


def seg_loss_fp32(logits, mask, gout=None, gscale=1.0, others=None, world=1):
    """The oracle's seg_loss (oracle.cross_entropy, the lines of oracle.dice_coeff) in fp32 with autograd; BCE from torch (module
    docstring).  The other ranks enter the Dice sums as constants."""
    from oracle import oracle
    x = _leaf32(logits)
    N, C, H, W = x.shape
    m = mask.reshape(N, H, W).long()
    if C == 1:
        t = m.float()
        crit = F.binary_cross_entropy_with_logits(x[:, 0], t)
        p = torch.sigmoid(x[:, 0])
    else:
        crit = oracle.cross_entropy(x, m)
        t = F.one_hot(m, C).permute(0, 3, 1, 2).float()
        p = torch.softmax(x, dim=1)
    o = torch.zeros(3) if others is None else others.float()
    inter = 2 * (p * t).sum() + o[0]
    sp, st = p.sum() + o[1], t.sum() + o[2]
    sets = sp + st
    sets = torch.where(sets == 0, inter, sets)
    dl = 1 - (inter + EPS) / (sets + EPS)
    ((crit + float(world) * dl) * _g32(gout, gscale)).backward()
    out = torch.stack([crit + dl, crit, dl, inter, sp, st, torch.tensor(float(world)), torch.tensor(0.0)]).detach()
    return {"out": out, "grad": x.grad}


def dice_loss_fp32(p, t, gout=None):
    from oracle import oracle
    a = _leaf32(p.reshape(1, 1, -1))
    b = t.float().reshape(1, 1, -1)
    loss = oracle.dice_loss(a, b)
    (loss * (1.0 if gout is None else float(gout))).backward()
    out = torch.stack([loss.detach(), 2 * (a.detach() * b).sum(), a.detach().sum(), b.sum()])
    return {"out": out, "grad": a.grad.reshape(p.shape)}


def jaccard_seg_loss_fp32(logits, mask, gout=None, gscale=1.0):
    from oracle import oracle
    x = _leaf32(logits)
    N = x.shape[0]
    t = mask.reshape(x.shape).float()
    bce = F.binary_cross_entropy_with_logits(x, t)
    p = torch.sigmoid(x[:, 0])
    ljac = 1.0 - oracle.jaccard_index(t[:, 0], p)
    ((bce + ljac) * _g32(gout, gscale)).backward()
    I = (t[:, 0] * p).sum(dim=(-1, -2)).detach()
    S = (t[:, 0] + p).sum(dim=(-1, -2)).detach()
    out = torch.cat([torch.stack([bce + ljac, bce, ljac, torch.tensor(0.0)]).detach(), torch.stack([I, S], dim=1).reshape(-1)])
    return {"out": out, "grad": x.grad}


def mean_loss_fp32(x, t, cval, mode, gout=None, gscale=1.0):
    v = _leaf32(x)
    c = float(cval)
    if mode == 0:
        loss = F.binary_cross_entropy_with_logits(v, torch.full_like(v, c))
    elif mode == 1:
        loss = ((v - c) ** 2).mean()                                             # oracle.gan_loss "lsgan" with a free label
    elif mode == 2:
        loss = v.mean() * c                                                      # oracle.gan_loss "wgangp"
    elif mode == 3:
        loss = (v - t.float()).abs().mean()                                      # oracle.l1_loss
    else:
        loss = F.binary_cross_entropy_with_logits(v, t.float())
    (loss * _g32(gout, gscale)).backward()
    return {"out": loss.detach().reshape(1), "grad": v.grad}


# ---------------------------------------------------------------------------------------------------------------- comparer
def value_errors(got, ref):
    """per entry |got - ref| / max(1, |ref|), fp64"""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().reshape(-1)
    return (got - ref).abs() / ref.abs().clamp(min=1.0)


def grad_error(got, ref):
    """max over the elements of |got - ref|, relative to max |ref| (to 1 where the reference gradient is zero everywhere)"""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().reshape(-1)
    if got.shape != ref.shape:
        raise ValueError("gradient shapes differ")
    scale = float(ref.abs().max())
    return float((got - ref).abs().max()) / (scale if scale > 0.0 else 1.0)


def value_bounds(e32):
    return (FACTOR * e32 + FLOOR).clamp(max=VALUE_CAP)


def grad_bound(e32):
    return FACTOR * e32 + FLOOR


def compare(got, ref, o32, exact=(), skip=(), what=""):
    """got / ref / o32: {"out", "grad"} of the kernel, the fp64 statement and the fp32 evaluation (either key may be missing from
    `got`: that part is not compared).  `exact`: indices of out that must equal float32(ref) exactly; `skip`: indices not compared.
    Returns (failures, report): failures is a list of strings, empty when everything holds; report the measured figures."""
    fails, rep = [], {}
    if got.get("out") is not None:
        err = value_errors(got["out"], ref["out"])
        bnd = value_bounds(value_errors(o32["out"], ref["out"]))
        g32 = got["out"].detach().float().cpu().reshape(-1)
        want32 = ref["out"].float().reshape(-1)
        worst = 0.0
        for i in range(err.numel()):
            if i in skip:
                continue
            if i in exact:
                if float(g32[i]) != float(want32[i]):
                    fails.append(f"{what} out[{i}] = {float(g32[i])!r}, exactly {float(want32[i])!r} expected")
                continue
            worst = max(worst, float(err[i]) / float(bnd[i]))
            if not float(err[i]) <= float(bnd[i]):
                fails.append(f"{what} out[{i}] = {float(g32[i])!r} vs {float(ref['out'].reshape(-1)[i])!r}: error {float(err[i]):.3e} > "
                             f"bound {float(bnd[i]):.3e}")
        rep["value_err"] = float(max([float(err[i]) for i in range(err.numel()) if i not in skip and i not in exact], default=0.0))
        rep["value_of_bound"] = worst
    if got.get("grad") is not None:
        e = grad_error(got["grad"], ref["grad"])
        b = grad_bound(grad_error(o32["grad"], ref["grad"]))
        rep["grad_err"], rep["grad_bound"] = e, b
        if not e <= b:
            fails.append(f"{what} gradient: max-norm error {e:.3e} of max |grad| > bound {b:.3e}")
    return fails, rep


def fmt(rep):
    return " ".join(f"{k}={v:.3e}" for k, v in rep.items())
