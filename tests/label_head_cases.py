"""Exact cases of the label head (gs_head1x1_labels, gs_labels_from_logits): shared by tests/test_label_head_reference_cpu.py (every
case meets the conditions under which a byte-for-byte comparison is valid, and is not vacuous) and
tests/test_label_head_kernels_gpu.py (kernel against the expected labels, every byte equal).  Plain torch on the CPU; no GPU, no
native library.

A case is a dense pair x = hi + lo of [N, H, W, 64]: hi integer-valued, lo a small multiple of 2^-4 (|lo| <= 3/16: both f16 and
bf16 hold hi and lo exactly), integer weights [ncls, 64] and biases.  Every product and every partial sum of a class is then a
multiple of 2^-4 far below 2^24 * 2^-4: exact in fp32 in any order, with or without fused multiply-add.  The BatchNorm-on-load
variant applies power-of-two scales (1/4, 1/2, 1), integer shifts and ReLU in front: multiples of 2^-6, the same argument.

Ties and coverage are PLANTED, because a random draw does not give them (with 64 classes a class wins 1.6 % of the pixels):
  several classes  one weight row and its bias are copied into a HIGHER class index (src < dst): the two logits are equal at every
                   pixel.  At 6 % of the pixels the input is chosen so that this pair is the maximum (z_i = a random 1..8 where
                   w[src][i] > 0, else 0): the label there must be src, never dst.  One further pixel per class c != dst is
                   chosen the same way for row c, so that every class that can win does win somewhere.
  one class        at 6 % of the pixels the logit is exactly 0 (z = 0 except channel 0, w[0][0] * z_0 = -bias): the label is 0.
Planted pixels have lo = 0; all other pixels are random.  The CPU test asserts these properties on the fp64 logits."""
import math

import torch

from tests import exact_reference as E
from tests import wide_head_cases as WH

SHAPES = WH.SHAPES                                   # "small" 2 x 11 x 9, "ragged" 3 x 37 x 29, "partial" 1 x 19 x 21
NCLS = (1, 2, 3, 4, 5, 8, 9, 33, 64)                 # 1..4: the 8-lanes-per-pixel kernel; 5..64: the thread-per-pixel kernel
CASES = [(shape, ncls) for shape in SHAPES for ncls in NCLS]
TIE_SHARE = 0.05                                     # asserted share of pixels with the tie at the maximum / the logit at 0
PLANT_SHARE = 0.06
LO_UNIT = 2.0 ** -4
SEEDS = {}                                           # (shape, ncls, bn) -> seed, where seed 0 does not meet the CPU test's conditions
WIDE_LOGITS_C = 70                                   # gs_labels_from_logits beyond the pair head's 64 classes


def case_id(case):
    return f"{case[0]}-{case[1]}"


def predicate(logits: torch.Tensor) -> torch.Tensor:
    """labels uint8 [M] of logits [M, C] (any float dtype): C == 1: 1 / (1 + exp(-x)) > 0.5; else the running best from class 0,
    replaced only on a strict v > best -- ties go to the lowest class index (eval_dice_kernel, csrc/loss.hip)"""
    if logits.shape[1] == 1:
        return (1.0 / (1.0 + torch.exp(-logits[:, 0])) > 0.5).to(torch.uint8)
    best = logits[:, 0].clone()
    pred = torch.zeros(logits.shape[0], dtype=torch.uint8)
    for c in range(1, logits.shape[1]):
        m = logits[:, c] > best
        pred[m] = c
        best = torch.where(m, logits[:, c], best)
    return pred


def activation(c, dtype=torch.float64) -> torch.Tensor:
    """what the head multiplies with its weights, [M, 64]: hi + lo, in the BatchNorm variant relu((hi + lo) * scale + shift)"""
    v = c["hi"].reshape(-1, 64).to(dtype) + c["lo"].reshape(-1, 64).to(dtype)
    if c["bn"]:
        v = torch.relu(v * c["scale"].to(dtype) + c["shift"].to(dtype))
    return v


def build(case, bn: bool):
    """hi, lo fp32 [N,H,W,64]; w fp32 [ncls,64]; b fp32 [ncls]; scale, shift fp32 [64] (bn: the load-path BatchNorm + ReLU);
    logits fp64 [M, ncls]; labels uint8 [N,H,W]; src, dst: the duplicated row pair (None for one class); tie / zero: planted pixels"""
    shape, ncls = case
    N, H, W = SHAPES[shape]
    M = N * H * W
    g = E.generator(("label_head", shape, ncls, bool(bn), SEEDS.get((shape, ncls, bool(bn)), 0)))
    ri = lambda lo, hi, size: torch.randint(lo, hi + 1, size, generator=g).float()
    hi = ri(-8, 8, (M, 64))
    lo = ri(-3, 3, (M, 64)) * LO_UNIT
    w = ri(-4, 4, (ncls, 64))
    b = ri(-8, 8, (ncls,))
    scale = 2.0 ** ri(-2, 0, (64,)) if bn else torch.ones(64)
    shift = ri(-4, 4, (64,)) if bn else torch.zeros(64)
    perm = torch.randperm(M, generator=g)
    nplant = int(math.ceil(PLANT_SHARE * M))
    out = {"bn": bool(bn), "ncls": ncls, "src": None, "dst": None}

    def put(p, z):                                   # the input whose load path yields z >= 0: an integer, (z - shift) / scale
        hi[p] = (z - shift) / scale
        lo[p] = 0.0

    def favour(row):                                 # z that makes class `row` large: a random 1..8 where its weight is positive
        return torch.where(w[row] > 0, ri(1, 8, (64,)), torch.zeros(64))

    if ncls == 1:
        if float(b[0]) == 0.0:
            b[0] = 3.0
        w[0, 0] = -torch.sign(b[0])
        z = torch.zeros(64)
        z[0] = b[0].abs()
        for p in perm[:nplant].tolist():
            put(p, z)
        out["planted"] = perm[:nplant]
    else:
        src = int(torch.randint(0, ncls - 1, (1,), generator=g))
        dst = int(torch.randint(src + 1, ncls, (1,), generator=g))
        w[dst] = w[src]
        b[dst] = b[src]
        out["src"], out["dst"] = src, dst
        assert M >= nplant + ncls
        for p in perm[:nplant].tolist():
            put(p, favour(src))
        k = nplant
        for c in range(ncls):
            if c != dst:
                put(int(perm[k]), favour(c))
                k += 1
        out["planted"] = perm[:k]
    out.update(hi=hi.view(N, H, W, 64), lo=lo.view(N, H, W, 64), w=w, b=b, scale=scale, shift=shift)
    out["logits"] = activation(out) @ w.double().t() + b.double()
    out["labels"] = predicate(out["logits"]).view(N, H, W)
    return out


def logits_nchw(c) -> torch.Tensor:
    """the case's exact logits as the logit kernels store them: fp32 [N, ncls, H, W]"""
    N, H, W = c["labels"].shape
    return E.expect32(c["logits"].view(N, H, W, c["ncls"]).permute(0, 3, 1, 2).contiguous())


def build_wide_logits():
    """integer logits [2, 70, 11, 9] in -8..8 (ties at the maximum at most pixels) for gs_labels_from_logits, and their labels"""
    g = E.generator(("labels_from_logits", WIDE_LOGITS_C))
    N, H, W = SHAPES["small"]
    x = torch.randint(-8, 9, (N, WIDE_LOGITS_C, H, W), generator=g).float()
    lab = predicate(x.permute(0, 2, 3, 1).reshape(-1, WIDE_LOGITS_C).double()).view(N, H, W)
    return x, lab
