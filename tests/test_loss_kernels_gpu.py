"""The loss kernels of csrc/loss.hip on the GPU (`-m gpu`), entry point by entry point, against the fp64 statements of
tests/loss_reference.py at the cases listed there: one pixel, a ragged four-block shape, shapes just over every block cap, 1..64
classes, logits of N(0, 2^2), N(0, 30^2) and with +100 / -100 / exact 0 planted, random / all-background / all-one-class masks, a
Dice denominator of the order of eps, an upstream gradient (absent or 3.0), a gradient scale (1 or 1/1024) and the world-of-four
multiplier written by losses.apply_global_dice.

Exact (zero tolerance): the pixel counts, out[6], out[7] and out[3] of the Jaccard output; mean_loss modes 1, 2, 3 and the dice_loss
sums on integer operands in [-8, 8]; the L1 gradient, 0 at every tie.  Everything else: values relative to max(1, |ref|), gradients
per element relative to max |ref grad|, each within 4 * e32 + 2^-22 (e32: the error of an fp32 evaluation of the same operation on
the CPU; no value bound above 2e-6) -- loss_reference.py gives the reasoning.  Every gradient is written into a buffer with guard
rows on both sides, which must keep their bytes; forward and backward launched twice at the capped shapes give the same bits.

Measured on an MI355X (worst case of each family; error / bound, gradients in units of max |ref grad|):
  family (runs)                         value error  of its bound   gradient error  of its bound
  seg_loss N(0, 2^2)          (312)       1.1e-07         0.39          2.7e-06         0.67
  seg_loss N(0, 30^2)         (312)       1.1e-07         0.31          5.6e-07         0.35
  seg_loss planted            (312)       1.2e-07         0.39          see below       0.25
  seg_loss capped, N(0, 2^2)   (24)       8.2e-08         0.22          5.0e-07         0.21
  seg_loss capped, N(0, 30^2)  (24)       4.9e-08         0.11          5.1e-07         0.21
  seg_loss capped, planted     (24)       8.6e-08         0.34          5.0e-07         0.22
  seg_loss eps-dominated       (12)       7.2e-08         0.25          2.4e-07         0.45
  jaccard N(0, 2^2)            (48)       1.1e-07         0.22          7.1e-07         0.23
  jaccard N(0, 30^2)           (48)       9.4e-08         0.29          see below       0.25
  jaccard planted              (48)       1.0e-07         0.30          2.1e-07         0.21
  dice_loss prob / integer     (20)       5.5e-08         0.14          1.4e-07         0.29
  dice_coeff_batched            (1)       5.9e-08         0.25          -               -
  mean_loss modes 0, 4        (200)       8.3e-08         0.27          1.5e-07         0.25
  mean_loss modes 1, 2, 3     (360)       9.4e-08         0.25          1.1e-07         0.27
"see below": in one-pixel cases with a saturated logit (|x| = 100, or x = 33 with t = 1) the whole gradient is of the order of 4e-44 or
p - 1 with p = 1 in fp32: the fp32 evaluation and the kernel both return 0 or a denormal, errors of 0.15 to 1.0 of max |grad| against
bounds of four times the fp32 evaluation's (up to 4.0).  With more than one pixel the gradient error of these two families stays
below 6e-07.  The largest bound of the N(0, 2^2) family (3.3e-05) is a one-pixel case as well: the
gradient of the true class is p_t - 1 with p_t close to 1.

Two defects these cases found, both fixed in csrc/loss.hip:
  - the multi-class forward formed lse = max + log(sum) and took lse - x_t and exp(x_t - lse): at logits of +-100 the rounding of lse
    (4e-6) biased the cross-entropy term and p_t with one sign at every such pixel -- out[3] off by 3.1e-06 of its value at
    ragged-64-planted-background (bound 3.7e-07), eight cases in all.  Now (max - x_t) + log(sum) and exp(x_t - max) / sum.
  - the library is built with -ffp-contract=fast, under which the compiler fuses its own expf expansion and loses its low-order
    term: expf off by |x| * 4e-8.  The one-pixel gradients of jaccard one-n30-background (1.3e-06, bound 4.6e-07), seg_loss
    one-1-n30-background and eps 1-2-2 went over their bounds.  sigmoid and softplus now take exp from a reduced argument written
    as one explicit fma (exp_tail in loss.hip), which leaves nothing to fuse.  The softmax path keeps expf: its arguments are
    x - max <= 0, and a term large enough to matter has a small argument.
"""
import pytest
import torch

from tests import exact_reference as E
from tests import loss_reference as LR

pytestmark = pytest.mark.gpu

GUARD = 1024                                                 # floats on either side of every gradient buffer
SENT = -7.25e11                                              # no gradient of these cases has this value


def dev():
    return torch.device("cuda:0")


class Guarded:
    """a contiguous fp32 tensor of `shape` inside a larger buffer whose other elements must not change"""

    def __init__(self, shape):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=dev())
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        assert self.t.is_contiguous()

    def check(self, what):
        torch.cuda.synchronize()
        n = self.t.numel()
        assert bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + n:] == SENT).all()), f"{what}: wrote beyond the tensor"
        assert not bool((self.t == SENT).any()), f"{what}: an element was not written"
        return self.t.cpu()


def scalar(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device=dev())


def report(what, rep, fails):
    print(f"{what}: {LR.fmt(rep)}")
    assert not fails, "\n".join(fails)


def ws():
    from semantic_segmentation_amd import ops
    return torch.empty(ops.LOSS_WS, dtype=torch.float32, device=dev())


# ---------------------------------------------------------------------------------------------------------------- seg_loss
def seg_fwd(xd, md, global_sums=None, world=1):
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd.losses import apply_global_dice
    out = torch.full((8,), SENT, dtype=torch.float32, device=dev())
    ops.seg_loss_fwd(xd, md, ws(), out)
    if world > 1:
        apply_global_dice(out, global_sums.to(dev()), world)
    return out


def seg_bwd(xd, md, out, gout, gscale, what):
    from semantic_segmentation_amd import ops
    d = Guarded(tuple(xd.shape))
    ops.seg_loss_bwd(xd, md, out, scalar(gout), gscale, d.t)              # gout None: a NULL pointer at the entry point
    return d.check(what)


def run_seg_case(x, m, others, scalars, what):
    xd, md = x.to(dev()), m.to(dev())
    C, npix = x.shape[1], m.numel()
    for gout, gscale, world in scalars:
        kw = dict(gout=gout, gscale=gscale, others=others if world > 1 else None, world=world)
        ref, o32 = LR.seg_loss(x, m, **kw), LR.seg_loss_fp32(x, m, **kw)
        out = seg_fwd(xd, md, ref["out"][3:6].float(), world)
        got = {"out": out.cpu(), "grad": seg_bwd(xd, md, out, gout, gscale, what)}
        exact = (5, 6, 7) if C == 1 else (4, 5, 6, 7)
        if world > 1:
            exact = (3, 4, 5, 6, 7)                                      # written by apply_global_dice from the CPU's sums
        elif C > 1:
            assert float(got["out"][4]) == float(got["out"][5]) == float(npix)
        fails, rep = LR.compare(got, ref, o32, exact=exact, what=what)
        report(f"{what} gout={gout} gscale={gscale:g} world={world}", rep, fails)


@pytest.mark.parametrize("case", LR.SEG_CASES, ids=LR.case_id)
def test_seg_loss_against_fp64(case):
    x, m, others = LR.seg_case(case)
    run_seg_case(x, m, others, LR.SCALARS_CAPPED if case[0] == "capped" else LR.SCALARS, "seg_loss " + LR.case_id(case))


@pytest.mark.parametrize("shape", LR.EPS_CASES, ids=LR.case_id)
def test_seg_loss_eps_dominated(shape):
    """sum p is a few 1e-6 and the mask is empty: DICE_EPS decides the Dice value and its gradient"""
    x, m = LR.eps_case(shape)
    run_seg_case(x, m, None, [s for s in LR.SCALARS if s[2] == 1], "seg_loss eps " + LR.case_id(shape))


@pytest.mark.parametrize("C", [1, 3])
def test_seg_loss_is_deterministic_at_the_capped_shape(C):
    x, m, _ = LR.seg_case(("capped", C, "n2", "random"))
    xd, md = x.to(dev()), m.to(dev())
    outs = [seg_fwd(xd, md) for _ in range(2)]
    grads = [seg_bwd(xd, md, outs[0], 3.0, 1.0 / 1024, f"seg_loss capped C={C}") for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- dice_loss
@pytest.mark.parametrize("n", LR.DICE_N)
@pytest.mark.parametrize("kind", LR.DICE_KINDS)
def test_dice_loss_against_fp64(kind, n):
    from semantic_segmentation_amd import ops
    p, t = LR.dice_case(kind, n)
    pd, td = p.to(dev()), t.to(dev())
    out = torch.full((4,), SENT, dtype=torch.float32, device=dev())
    ops.dice_loss_fwd(pd, td, ws(), out)
    exact = {"prob": (3,), "integer": (1, 2, 3), "zero": (0, 1, 2, 3), "opposite": (0, 1, 2, 3)}[kind]   # sum t of {0,1}: a count
    for gout in (None, 3.0):
        what = f"dice_loss {kind} n={n} gout={gout}"
        d = Guarded((n,))
        ops.dice_loss_bwd(td, out, scalar(gout), d.t)
        got = {"out": out.cpu(), "grad": d.check(what)}
        ref, o32 = LR.dice_loss(p, t, gout), LR.dice_loss_fp32(p, t, gout)
        fails, rep = LR.compare(got, ref, o32, exact=exact, what=what)
        report(what, rep, fails)
        if kind in ("zero", "opposite"):                                  # dice_score.py:14: the degenerate branch, gradient exactly 0
            assert float(got["grad"].abs().max()) == 0.0
    if n == max(LR.DICE_N):
        out2 = torch.full((4,), SENT, dtype=torch.float32, device=dev())
        ops.dice_loss_fwd(pd, td, ws(), out2)
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32))


def test_dice_coeff_batched_over_the_block_cap():
    """more than 16 x 2048 elements per item: every block of an item makes more than one trip"""
    from semantic_segmentation_amd import ops
    B, n = LR.DICE_BATCHED_SHAPE
    g = E.generator(("dice_batched", B, n))
    p = torch.sigmoid(2.0 * torch.randn(B, n, generator=g))
    t = (torch.rand(B, n, generator=g) > 0.5).float()
    p[2], t[2] = 0.0, 0.0                                                 # sets == 0: the coefficient is 1
    out = torch.full((1 + B,), SENT, dtype=torch.float32, device=dev())
    ops.dice_coeff_batched(p.to(dev()), t.to(dev()), out)
    ref = {"out": LR.dice_coeff_batched(p, t)}
    o32 = {"out": LR.dice_coeff_batched(p, t, torch.float32)}
    fails, rep = LR.compare({"out": out.cpu()}, ref, o32, exact=(3,), what="dice_coeff_batched")
    report("dice_coeff_batched", rep, fails)


# ---------------------------------------------------------------------------------------------------------------- Jaccard
@pytest.mark.parametrize("case", LR.JACCARD_CASES, ids=LR.case_id)
def test_jaccard_seg_loss_against_fp64(case):
    from semantic_segmentation_amd import ops
    x, m = LR.jaccard_case(case)
    xd, md = x.to(dev()), m.to(dev())
    N = x.shape[0]
    outs = []
    for _ in range(2):
        out = torch.full((4 + 2 * N,), SENT, dtype=torch.float32, device=dev())
        ops.jaccard_seg_loss_fwd(xd, md, out)
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    grads = []
    for gout, gscale in LR.JACCARD_SCALARS:
        what = f"jaccard {LR.case_id(case)} gout={gout} gscale={gscale:g}"
        d = Guarded(tuple(x.shape))
        ops.jaccard_seg_loss_bwd(xd, md, outs[0], scalar(gout), gscale, d.t)
        got = {"out": outs[0].cpu(), "grad": d.check(what)}
        grads.append(got["grad"])
        ref, o32 = LR.jaccard_seg_loss(x, m, gout, gscale), LR.jaccard_seg_loss_fp32(x, m, gout, gscale)
        fails, rep = LR.compare(got, ref, o32, exact=(3,), what=what)
        report(what, rep, fails)
    d = Guarded(tuple(x.shape))
    ops.jaccard_seg_loss_bwd(xd, md, outs[0], scalar(3.0), 1.0 / 1024, d.t)
    assert torch.equal(d.check("jaccard again").view(torch.int32), grads[-1].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- mean_loss
def mean_fwd(xd, td, cval, mode):
    from semantic_segmentation_amd import ops
    out = torch.full((1,), SENT, dtype=torch.float32, device=dev())
    ops.mean_loss_fwd(xd, td, cval, mode, ws(), out)
    return out


@pytest.mark.parametrize("n", LR.MEAN_N)
@pytest.mark.parametrize("family", LR.MEAN_FAMILIES)
@pytest.mark.parametrize("mode", LR.MEAN_MODES)
def test_mean_loss_against_fp64(mode, family, n):
    from semantic_segmentation_amd import ops
    x, t = LR.mean_case(mode, n, family)
    xd, td = x.to(dev()), None if t is None else t.to(dev())
    for cval in (LR.MEAN_CVAL if mode < 3 else (0.0,)):
        out = mean_fwd(xd, td, cval, mode)
        for gout, gscale in LR.MEAN_SCALARS:
            what = f"mean_loss mode={mode} {family} n={n} cval={cval} gout={gout} gscale={gscale:g}"
            d = Guarded((n,))
            ops.mean_loss_bwd(xd, td, cval, mode, scalar(gout), gscale, d.t)
            got = {"out": out.cpu(), "grad": d.check(what)}
            ref, o32 = LR.mean_loss(x, t, cval, mode, gout, gscale), LR.mean_loss_fp32(x, t, cval, mode, gout, gscale)
            fails, rep = LR.compare(got, ref, o32, what=what)
            report(what, rep, fails)
            if mode == 3:                                                 # +-float32(float32(gout * gscale) / float32(n)), 0 at every tie
                E.assert_exact(got["grad"], LR.l1_grad_exact(x, t, gout, gscale), what + " exact")
                assert float(got["grad"][x == t].abs().max() if bool((x == t).any()) else 0.0) == 0.0
        if n == max(LR.MEAN_N):
            assert torch.equal(out.view(torch.int32), mean_fwd(xd, td, cval, mode).view(torch.int32))


@pytest.mark.parametrize("n", LR.MEAN_N)
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_mean_loss_integer_operands_exact(mode, n):
    """operands in [-8, 8] and an integer label: every fp32 partial sum is exact, the double finalise divides the exact sum by n"""
    x, t = LR.mean_case_integer(mode, n)
    xd, td = x.to(dev()), None if t is None else t.to(dev())
    for cval in ((0.0, 1.0, -1.0) if mode < 3 else (0.0,)):
        got = mean_fwd(xd, td, cval, mode).cpu()
        want = LR.mean_loss(x, t, cval, mode)["out"].float()
        assert float(got) == float(want), (mode, n, cval, float(got), float(want))
