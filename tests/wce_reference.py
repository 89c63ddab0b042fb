"""fp64 statement of the class-weighted cross-entropy of csrc/loss.hip (gs_wce_fwd / gs_wce_bwd), an fp32 evaluation of the same
operation, and the case lists of its tests.  Shared by tests/test_wce_reference_cpu.py (the statement agrees with torch's
F.cross_entropy(weight=) in fp64; the comparer rejects every planted error) and tests/test_wce_kernels_gpu.py (both entry points
against the statement).  Plain torch on the CPU; no GPU, no native library.

The operation is the criterion of both 3-D scripts of the reference (GenSeg-3D/train_unet.py:135,155,170 and train_end2end.py:139:
CrossEntropyLoss(weight=torch.Tensor(BCE_WEIGHTS)); UNet3D/config.py:35: BCE_WEIGHTS = [0.004, 0.996]), as include/gsseg.h states
it: logits fp32 [N][C][S], target uint8 [N][S], weight fp32 [C] or None,
    out = [sum_i w[t_i] (lse_i - x_{i,t_i}) / W, the numerator, W = sum_i w[t_i], gradient multiplier, 0, 0, 0, 0]
    grad[i, c] = gout * gscale * out[3] * w[t_i] * (p_{i,c} - [c == t_i]) / out[2]
    labels[i] = the first maximum over c (replaced only on a strict v > best)
With the numerator and W of the other ranks added (`others`, `world`): out[1], out[2] are the global sums, out[0] their quotient
and out[3] = world (losses.apply_global_mean), so that the gradient AVERAGE over the ranks is that of the global weighted mean.
The weights enter as the fp32 values the entry point receives.  Target values >= C are outside the contract: the statement raises.

Comparer and bound: loss_reference.compare unchanged -- every figure within 4 * e32 + 2^-22 of the fp64 statement, e32 the error of
the fp32 evaluation below on the same scale, no value bound above 2e-6; out[3..7] exact; out[2] exact where the weights are None
or multiples of 1/4 (fp32 sums of such values are exact in any order: W * 4 stays below 2^24 at every shape here).

Shapes (N, S), the smallest at which each path of the kernel runs.  The grid formula of the header comment of the kernels: items =
N * S / 4 on the vector path (S % 4 == 0, aligned pointers), N * S on the scalar path; forward min(1024, ceil(items / 256)) blocks,
backward min(2048, ceil(items / 256)).
    one      (1, 1)            a single voxel (scalar path, one thread)
    ragged   (3, 5 * 7 * 9)    S odd: every class plane starts at another offset within 16 bytes: the scalar path, four blocks
    aligned  (2, 16^3)         the vector path, eight blocks, two samples
    fwd_cap  (1, 1025 * 1024)  1025 > 1024 forward blocks on the vector path (the scalar path, 4100 > 1024, is reached through a
                               pointer that is not 16-byte aligned: tests/test_wce_kernels_gpu.py)
    bwd_cap  (1, 2049 * 1024)  2049 > 2048 backward blocks on the vector path
The capped shapes do not interact with the logit family, the mask or the weights beyond what the small shapes show: each capped
(shape, C, family, mask) runs with ONE weight kind and ONE scalar triple, rotated so that every kind and every scalar value occurs
at both caps.  The small shapes run every weight kind; "ragged" with all eight scalar triples, the others with four that hold
every value of each scalar."""
import torch
import torch.nn.functional as F

from tests import exact_reference as E
from tests import loss_reference as LR

FAULTS = ("div_voxels", "weight_argmax", "grad_no_weight", "drop_voxel", "gscale_twice", "last_max")
REFERENCE_WEIGHTS = (0.004, 0.996)                          # UNet3D/config.py:35
DYADIC = (0.25, 1.0, 0.5, 0.75)

SHAPES = {"one": (1, 1), "ragged": (3, 5 * 7 * 9), "aligned": (2, 16 ** 3), "fwd_cap": (1, 1025 * 1024), "bwd_cap": (1, 2049 * 1024)}
SPATIAL = {"one": (1,), "ragged": (5, 7, 9), "aligned": (16, 16, 16), "fwd_cap": (1025, 1024), "bwd_cap": (2049, 1024)}
SMALL, CAPPED = ("one", "ragged", "aligned"), ("fwd_cap", "bwd_cap")
CLASSES = {"one": (2, 3, 4, 5, 9, 64), "ragged": (2, 3, 4, 5, 9, 64), "aligned": (2, 3, 4, 5, 9, 64), "fwd_cap": (2, 3), "bwd_cap": (2, 3)}
FAMILIES, MASKS = LR.FAMILIES, LR.MASKS
WEIGHTS = ("none", "reference", "dyadic", "one_zero", "present_zero")
CASES = [(s, C, f, m) for s in SHAPES for C in CLASSES[s] for f in FAMILIES for m in MASKS]
SCALARS, SCALARS_FOUR = LR.SCALARS, LR.SCALARS_CAPPED      # (gout, gscale, world)
WORLD_SHAPE = (3, 5 * 7 * 9)                                # the three other ranks of the world-of-four cases hold batches of this shape
FWD_MAX_BLOCKS, BWD_MAX_BLOCKS = 1024, 2048


def case_id(case):
    return "-".join(str(c) for c in case)


def runs_of(case):
    """[(weight kind, [scalar triples])] of one (shape, C, family, mask) case (module docstring)"""
    shape = case[0]
    if shape in CAPPED:
        k = CASES.index(case)
        return [(WEIGHTS[k % len(WEIGHTS)], [SCALARS_FOUR[k % len(SCALARS_FOUR)]])]
    return [(w, SCALARS if shape == "ragged" else SCALARS_FOUR) for w in WEIGHTS]


def class_weights(kind, C, target=None):
    """the weight vector of a kind as fp32 [C], or None"""
    if kind == "none":
        return None
    if kind == "dyadic":
        return torch.tensor([DYADIC[c % 4] for c in range(C)], dtype=torch.float32)
    w = torch.tensor([REFERENCE_WEIGHTS[c % 2] for c in range(C)], dtype=torch.float32)
    if kind == "one_zero":
        w[0] = 0.0
    elif kind == "present_zero":
        w[torch.unique(target.long())] = 0.0
    elif kind != "reference":
        raise ValueError(kind)
    return w


def wce_case(case):
    """logits fp32 [N,C,S], target uint8 [N,S] of a (shape, C, family, mask) case"""
    shape, C, family, mkind = case
    N, S = SHAPES[shape]
    g = E.generator(("wce",) + tuple(case))
    x = LR.draw_logits(g, (N, C, S), family)
    t = LR.draw_mask(g, N, C, 1, S, mkind).reshape(N, S)
    return x, t


def other_ranks(case, weight):
    """(numerator, W) summed over the three other ranks of a world of four, fp64 [2]: batches of WORLD_SHAPE, same weights"""
    C = case[1]
    g = E.generator(("wce_world",) + tuple(case))
    tot = torch.zeros(2, dtype=torch.float64)
    for _ in range(3):
        xo = LR.draw_logits(g, (WORLD_SHAPE[0], C, WORLD_SHAPE[1]), "n2")
        to = LR.draw_mask(g, WORLD_SHAPE[0], C, 1, WORLD_SHAPE[1], "random").reshape(WORLD_SHAPE)
        tot += wce(xo, to, weight)["out"][1:3]
    return tot


# ---------------------------------------------------------------------------------------------------------------- fp64 statement
def first_maximum(x, last=False):
    """arg-max over dim 1 of [N,C,S], the first maximum (last=True: the last one -- the "last_max" fault); uint8 [N,S]"""
    best = x[:, 0].clone()
    pred = torch.zeros(best.shape, dtype=torch.uint8)
    for c in range(1, x.shape[1]):
        v = x[:, c]
        hit = (v >= best) if last else (v > best)
        best = torch.where(hit, v, best)
        pred = torch.where(hit, torch.full_like(pred, c), pred)
    return pred


def wce(logits, target, weight=None, gout=None, gscale=1.0, others=None, world=1, fault=None):
    """gs_wce_fwd / _bwd: {"out": fp64 [8], "grad": fp64 like logits, "labels": uint8 [N,S]}.  logits [N,C,S] (or any [N,C,*spatial]),
    target [N,S]; weight fp32 [C] or None; others: fp64 (numerator, W) of the other ranks, world their number plus one."""
    N, C = logits.shape[0], logits.shape[1]
    x = logits.double().reshape(N, C, -1)
    S = x.shape[2]
    t = target.reshape(N, S).long()
    if int(t.max()) >= C:
        raise ValueError(f"target value {int(t.max())} is outside the contract of {C} classes")
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.float().double()
    labels = first_maximum(logits.float().reshape(N, C, S), last=(fault == "last_max"))
    onehot = F.one_hot(t, C).permute(0, 2, 1).double()
    mx = x.max(dim=1, keepdim=True).values
    z = x - mx
    den = torch.exp(z).sum(dim=1, keepdim=True)
    P = torch.exp(z) / den
    terms = torch.log(den)[:, 0] - (z * onehot).sum(dim=1)                       # lse - x_t, [N,S]
    wt = w[labels.long()] if fault == "weight_argmax" else w[t]
    keep = torch.ones(N, S, dtype=torch.float64)
    if fault == "drop_voxel":
        nz = (wt.reshape(-1) != 0).nonzero()
        keep.view(-1)[int(nz[-1]) if nz.numel() else N * S - 1] = 0.0
    num = (wt * terms * keep).sum()
    W = torch.tensor(float(N * S), dtype=torch.float64) if fault == "div_voxels" else (wt * keep).sum()
    if others is not None:
        num, W = num + others[0].double(), W + others[1].double()
    zero = torch.tensor(0.0, dtype=torch.float64)
    out = torch.stack([num / W, num, W, torch.tensor(float(world), dtype=torch.float64), zero, zero, zero, zero])
    gw = torch.ones_like(wt) if fault == "grad_no_weight" else wt
    g = LR._g(gout, gscale, "gscale_twice" if fault == "gscale_twice" else None)
    grad = g * float(world) * (gw * keep).unsqueeze(1) * (P - onehot) / W
    return {"out": out, "grad": grad.reshape(logits.shape), "labels": labels}


# ---------------------------------------------------------------------------------------------------------------- fp32 evaluation
def wce_fp32(logits, target, weight=None, gout=None, gscale=1.0, others=None, world=1):
    """F.cross_entropy(weight=) under fp32 autograd; in a world of four the weighted sum and W of the other ranks enter as constants"""
    N, C = logits.shape[0], logits.shape[1]
    x = LR._leaf32(logits.reshape(N, C, -1))
    t = target.reshape(N, -1).long()
    w = None if weight is None else weight.float()
    g = LR._g32(gout, gscale)
    if others is None:
        loss = F.cross_entropy(x, t, weight=w)
        num = F.cross_entropy(x.detach(), t, weight=w, reduction="sum")
        W = torch.tensor(float(t.numel())) if w is None else w[t].sum()
    else:
        num = F.cross_entropy(x, t, weight=w, reduction="sum") + others[0].float()
        W = (torch.tensor(float(t.numel())) if w is None else w[t].sum()) + others[1].float()
        loss = num / W
    (loss * float(world) * g).backward()
    z = torch.tensor(0.0)
    out = torch.stack([loss.detach(), num.detach(), W, torch.tensor(float(world)), z, z, z, z])
    return {"out": out, "grad": x.grad.reshape(logits.shape)}


def exact_indices(kind):
    """indices of out that must equal the fp64 statement exactly"""
    return (2, 3, 4, 5, 6, 7) if kind in ("none", "dyadic") else (3, 4, 5, 6, 7)
