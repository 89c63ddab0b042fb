"""tests/loss_reference.py proven on the CPU (no GPU, no native library): the fp64 statements agree with the oracle's losses and
with torch's own criteria run in fp64 (values and autograd gradients), and with the values recorded from the reference in
tests/golden/{dice_cases,jaccard_cases,ops_micro}.npz; the case lists cross the block caps they are meant to cross; and the comparer
the GPU test uses rejects every planted error of loss_reference.FAULTS while it accepts an fp32 evaluation of the same operation."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import exact_reference as E
from tests import loss_reference as LR

TIGHT = 1e-12


def close(a, b, tol=TIGHT):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def grad_close(a, b, tol=TIGHT):
    return LR.grad_error(a, b) <= tol


def oracle64(fn, x, *args):
    v = x.detach().clone().double().requires_grad_(True)
    y = fn(v, *args)
    y.backward()
    return y.detach(), v.grad


# ---------------------------------------------------------------------------------------------------------------- case lists
def test_case_lists_cross_the_block_caps():
    N, H, W = LR.SEG_SHAPES["capped"]
    assert 1024 * 1024 < N * H * W < 1024 * 1024 + 8192 and (N * H * W) % 256 != 0       # forward 1024 x 1024, backward 4096 x 256
    assert N * H * W < E.LIMIT                                                           # the counts are exact in fp32
    N, H, W = LR.JACCARD_SHAPES["item_cap"]
    assert N == 3 and 16 * 2048 < H * W < 16 * 2048 + 2048 and (H * W) % 256 != 0
    N, H, W = LR.JACCARD_SHAPES["bwd_cap"]
    assert 256 * 1024 < H * W < 256 * 1024 + 4096 and (H * W) % 256 != 0
    assert LR.DICE_BATCHED_SHAPE[1] > 16 * 2048
    assert max(LR.MEAN_N) > 1024 * 1024 and max(LR.MEAN_N) % 256 != 0
    assert set(LR.MEAN_N) == {1, 255, 257, 4099, 1052651}
    assert {c[1] for c in LR.SEG_CASES} == {1, 2, 3, 4, 5, 9, 64}
    assert {c[0] for c in LR.SEG_CASES if c[1] == 64} == {"ragged"}
    assert {c[1] for c in LR.SEG_CASES if c[0] == "capped"} == {1, 3}
    for s in (LR.SCALARS, LR.SCALARS_CAPPED):
        assert {a for a, _, _ in s} == {None, 3.0} and {b for _, b, _ in s} == {1.0, 1.0 / 1024} and {c for _, _, c in s} == {1, 4}


def test_case_inputs_have_the_planted_values():
    x, m, others = LR.seg_case(("ragged", 3, "planted", "random"))
    assert int((x == 100).sum()) > 100 and int((x == -100).sum()) > 100 and int((x == 0).sum()) > 100
    assert float(others[1]) == pytest.approx(9 * 37 * 29, rel=1e-12) and float(others[2]) == 9 * 37 * 29
    x, m, _ = LR.seg_case(("ragged", 64, "n30", "one_class"))
    assert float(x.abs().max()) > 90 and bool((m == 63).all())
    x, m, _ = LR.seg_case(("ragged", 2, "n2", "one_class"))
    assert bool((m == 1).all())
    for shape in LR.EPS_CASES:
        x, m = LR.eps_case(shape)
        r = LR.seg_loss(x, m)["out"]
        assert x.numel() <= 4 and float(r[5]) == 0 and float(r[3]) == 0 and 1e-7 < float(r[4]) < 1e-5     # sum p ~ EPS
        assert 0.1 < float(r[2]) < 0.95
    x, t = LR.mean_case(3, 4099, "planted")
    assert 0.08 < float((x == t).float().mean()) < 0.13
    for mode in (1, 2, 3):                                          # integer operands: |term| <= 256, a block's partial sum far below 2^24
        x, t = LR.mean_case_integer(mode, 4099)
        E.require_integers(x, *([t] if t is not None else []))
        assert float(x.abs().max()) <= 8
    p, t = LR.dice_case("opposite", 257)
    assert float(p.sum() + t.sum()) == 0.0 and float((p * t).sum()) < 0


# ---------------------------------------------------------------------------------------------------------------- seg_loss
@pytest.mark.parametrize("C", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("family", LR.FAMILIES)
@pytest.mark.parametrize("mkind", LR.MASKS)
def test_seg_loss_matches_oracle_fp64(C, family, mkind):
    from oracle import oracle
    x, m, _ = LR.seg_case(("ragged", C, family, mkind))
    r = LR.seg_loss(x, m)
    if C == 1 and family == "planted":          # autograd through the oracle's BCE gives 1 - t at the exact zeros: torch's criterion instead
        def fn(v, mm):
            t = mm.double()
            return F.binary_cross_entropy_with_logits(v[:, 0], t) + oracle.dice_loss(torch.sigmoid(v[:, 0]), t)
        # the oracle's value is still the same number
        assert close(r["out"][0], oracle.seg_loss(x.double(), m.long()))
    else:
        fn = oracle.seg_loss
    y, g = oracle64(fn, x, m.long())
    assert close(r["out"][0], y) and grad_close(r["grad"], g)
    crit = (F.binary_cross_entropy_with_logits(x.double()[:, 0], m.double()) if C == 1
            else F.cross_entropy(x.double(), m.long()))
    assert close(r["out"][1], crit) and close(r["out"][2], y - crit, 1e-11)
    assert float(r["out"][6]) == 1.0 and float(r["out"][7]) == 0.0
    assert float(r["out"][5]) == (float(m.sum()) if C == 1 else m.numel())
    if C > 1:
        assert close(r["out"][4], m.numel())
    # upstream gradient and scale are plain factors
    r2 = LR.seg_loss(x, m, gout=3.0, gscale=1.0 / 1024)
    assert grad_close(r2["grad"], g * 3.0 / 1024) and torch.equal(r2["out"], r["out"])


@pytest.mark.parametrize("C", [1, 3])
def test_seg_loss_world_of_four_is_the_full_batch(C):
    """Rank 0 of four with the other ranks' summed triples: global sums, the global Dice, and world x the full-batch gradient of the
    rank's slice (the data-parallel exchange averages over the ranks); losses.apply_global_dice writes the same numbers."""
    from oracle import oracle
    from semantic_segmentation_amd.losses import apply_global_dice
    g = E.generator(("world", C))
    N, H, W = 3, 37, 29
    xs = [LR.draw_logits(g, (N, C, H, W), "n2") for _ in range(4)]
    ms = [LR.draw_mask(g, N, C, H, W, "random") for _ in range(4)]
    others = sum(LR.seg_loss(xs[k], ms[k])["out"][3:6] for k in (1, 2, 3))
    r = LR.seg_loss(xs[0], ms[0], others=others, world=4)
    y, gfull = oracle64(oracle.seg_loss, torch.cat(xs), torch.cat(ms).long())
    crit_full = sum(LR.seg_loss(xs[k], ms[k])["out"][1] for k in range(4)) / 4
    assert close(r["out"][2], y - crit_full, 1e-11)
    assert close(r["out"][0], r["out"][1] + r["out"][2]) and float(r["out"][6]) == 4.0
    assert grad_close(r["grad"], 4.0 * gfull[:N])
    local = LR.seg_loss(xs[0], ms[0])["out"].clone()
    apply_global_dice(local, local[3:6] + others, 4)
    assert close(local, r["out"], 1e-14)


def test_mask_values_outside_the_contract_raise():
    x = torch.zeros(1, 3, 2, 2)
    with pytest.raises(ValueError):
        LR.seg_loss(x, torch.full((1, 2, 2), 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        LR.seg_loss(x[:, :1], torch.full((1, 2, 2), 2, dtype=torch.uint8))
    with pytest.raises(ValueError):
        LR.jaccard_seg_loss(x[:, :1], torch.full((1, 2, 2), 2, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- dice_loss
@pytest.mark.parametrize("kind", LR.DICE_KINDS)
def test_dice_loss_matches_oracle_fp64(kind):
    from oracle import oracle
    p, t = LR.dice_case(kind, 4099)
    r = LR.dice_loss(p, t, gout=3.0)
    y, g = oracle64(lambda v: oracle.dice_loss(v.reshape(1, 1, -1), t.double().reshape(1, 1, -1)), p)
    assert close(r["out"][0], y)
    assert float((r["grad"] - 3.0 * g).abs().max()) <= 1e-12 * max(1e-30, float(g.abs().max()), 1.0)
    if kind in ("zero", "opposite"):            # dice_score.py:14: sets == 0 -> the coefficient is (I + eps) / (I + eps) = 1
        assert float(r["out"][0]) == 0.0 and float(r["grad"].abs().max()) == 0.0


def test_dice_matches_recorded_reference_values(golden_dir):
    z = np.load(os.path.join(golden_dir, "dice_cases.npz"))
    p, t = torch.from_numpy(z["p"]), torch.from_numpy(z["t"])
    r = LR.dice_loss(p, t)
    assert close(r["out"][0], float(z["loss"]), 2e-7)                            # recorded in fp32
    assert LR.grad_error(r["grad"], torch.from_numpy(z["loss_grad_p"])) < 1e-6
    assert close(1.0 - r["out"][0], float(z["coeff_rbf_true"]), 2e-7)
    assert close(LR.dice_loss(torch.zeros_like(p), torch.zeros_like(p))["out"][0], float(z["all_zero_loss"]), 0.0)
    assert close(LR.dice_loss(p, torch.zeros_like(p))["out"][0], float(z["zero_target_loss"]), 2e-7)
    assert close(LR.dice_loss(torch.from_numpy(z["pm"]), torch.from_numpy(z["tm"]))["out"][0], float(z["mc_loss"]), 2e-7)
    b = LR.dice_coeff_batched(p.reshape(3, -1), t.reshape(3, -1))
    assert close(b[0], float(z["coeff_rbf_false"]), 2e-7) and close(b[1], float(z["coeff_2d"]), 2e-7)


# ---------------------------------------------------------------------------------------------------------------- Jaccard
@pytest.mark.parametrize("family", LR.FAMILIES)
@pytest.mark.parametrize("mkind", LR.MASKS)
def test_jaccard_matches_oracle_fp64(family, mkind):
    from oracle import oracle
    x, m = LR.jaccard_case(("ragged", family, mkind))
    r = LR.jaccard_seg_loss(x, m, gout=3.0, gscale=1.0 / 1024)
    assert close(r["out"][0], oracle.seg_loss_jaccard(x.double(), m.long()))
    t = m.double().unsqueeze(1)
    y, g = oracle64(lambda v: F.binary_cross_entropy_with_logits(v, t) + 1.0 - oracle.jaccard_index(t[:, 0], torch.sigmoid(v[:, 0])), x)
    assert close(r["out"][0], y) and grad_close(r["grad"], g * 3.0 / 1024)
    assert close(r["out"][1], F.binary_cross_entropy_with_logits(x.double(), t)) and float(r["out"][3]) == 0.0
    p = torch.sigmoid(x.double())
    assert close(r["out"][4::2], (p * t).sum(dim=(1, 2, 3))) and close(r["out"][5::2], (p + t).sum(dim=(1, 2, 3)))


def test_jaccard_matches_recorded_reference_values(golden_dir):
    z = np.load(os.path.join(golden_dir, "jaccard_cases.npz"))
    x, m = torch.from_numpy(z["logits"]), torch.from_numpy(z["mask"])
    r = LR.jaccard_seg_loss(x, m.to(torch.uint8)[:, 0])
    assert close(r["out"][0], float(z["loss"]), 2e-7) and close(r["out"][1], float(z["bce"]), 2e-7)
    assert close(1.0 - r["out"][2], float(z["jaccard"]), 2e-7)
    assert LR.grad_error(r["grad"], torch.from_numpy(z["grad"])) < 2e-6
    assert close(LR.jaccard_seg_loss(x[:1], m.to(torch.uint8)[:1, 0])["out"][0], float(z["loss_b1"]), 2e-7)


# ---------------------------------------------------------------------------------------------------------------- mean_loss
@pytest.mark.parametrize("mode", LR.MEAN_MODES)
@pytest.mark.parametrize("family", LR.MEAN_FAMILIES)
def test_mean_loss_matches_torch_fp64(mode, family):
    x, t = LR.mean_case(mode, 4099, family)
    for cval in LR.MEAN_CVAL:
        c = float(torch.tensor(cval, dtype=torch.float32))
        fn = {0: lambda v: F.binary_cross_entropy_with_logits(v, torch.full_like(v, c)),
              1: lambda v: F.mse_loss(v, torch.full_like(v, c)),
              2: lambda v: v.mean() * c,
              3: lambda v: F.l1_loss(v, t.double()),
              4: lambda v: F.binary_cross_entropy_with_logits(v, t.double())}[mode]
        y, g = oracle64(fn, x)
        r = LR.mean_loss(x, t, cval, mode, gout=3.0, gscale=1.0 / 1024)
        assert close(r["out"], y)
        assert float((r["grad"] - g * 3.0 / 1024).abs().max()) <= 1e-12 * max(float(g.abs().max()), 1e-30)
    if mode == 3:
        tie = x == t
        assert int(tie.sum()) > 300 and float(r["grad"][tie].abs().max()) == 0.0
        assert torch.equal(LR.l1_grad_exact(x, t, 3.0, 1.0 / 1024).double(),
                           (torch.tensor(3.0 / 1024) / torch.tensor(4099.0)).double() * torch.sign(x - t).double())


def test_mean_loss_matches_recorded_reference_values(golden_dir):
    from oracle import oracle
    z = np.load(os.path.join(golden_dir, "ops_micro.npz"))
    pred = torch.from_numpy(z["gan/pred"])
    for name, mode in (("vanilla", 0), ("lsgan", 1)):
        assert close(LR.mean_loss(pred, None, 1.0, mode)["out"], float(z[f"gan/{name}/real"]), 2e-7)
        assert close(LR.mean_loss(pred, None, 0.0, mode)["out"], float(z[f"gan/{name}/fake"]), 2e-7)
        assert close(LR.mean_loss(pred, None, 1.0, mode)["out"], oracle.gan_loss(pred.double(), True, name))
    assert close(LR.mean_loss(pred, None, -1.0, 2)["out"], float(z["gan/wgangp/real"]), 2e-7)
    assert close(LR.mean_loss(pred, None, 1.0, 2)["out"], float(z["gan/wgangp/fake"]), 2e-7)
    a, b = torch.from_numpy(z["l1/a"]), torch.from_numpy(z["l1/b"])
    assert close(LR.mean_loss(a, b, 0.0, 3)["out"], float(z["l1/y"]), 2e-7)
    x, t = torch.from_numpy(z["bce/x"]), torch.from_numpy(z["bce/t"])
    assert close(LR.mean_loss(x, t, 0.0, 4)["out"], float(z["bce/y"]), 2e-7)


# ---------------------------------------------------------------------------------------------------------------- the comparer
def as_kernel(r):
    """an fp64 result as a perfect fp32 kernel would return it"""
    return {k: v.float() for k, v in r.items()}


SEG_EXACT = (5, 6, 7)


def test_comparer_accepts_fp32_evaluations_and_the_rounded_reference():
    worst = {"value": 0.0, "grad": 0.0}
    for case in [("ragged", 1, "n2", "random"), ("ragged", 3, "n30", "random"), ("ragged", 9, "planted", "one_class"),
                 ("one", 2, "n30", "random"), ("ragged", 1, "planted", "background")]:
        x, m, others = LR.seg_case(case)
        for gout, gscale, world in LR.SCALARS:
            kw = dict(gout=gout, gscale=gscale, others=others if world > 1 else None, world=world)
            ref, o32 = LR.seg_loss(x, m, **kw), LR.seg_loss_fp32(x, m, **kw)
            for got in (o32, as_kernel(ref)):
                fails, rep = LR.compare(got, ref, o32, exact=SEG_EXACT, what=LR.case_id(case))
                assert not fails, fails
            worst["value"] = max(worst["value"], float(LR.value_errors(o32["out"], ref["out"]).max()))
            worst["grad"] = max(worst["grad"], LR.grad_error(o32["grad"], ref["grad"]))
    print("fp32 evaluation of seg_loss: value error %.3e, gradient error %.3e of max |grad|" % (worst["value"], worst["grad"]))
    assert worst["value"] < 1e-5 and worst["grad"] < 1e-4            # the fp32 evaluation is itself a sane yardstick


def rejected(got, ref, o32, **kw):
    fails, _ = LR.compare(got, ref, o32, **kw)
    return len(fails) > 0


@pytest.mark.parametrize("shape", LR.EPS_CASES, ids=LR.case_id)
def test_comparer_rejects_a_dice_without_eps(shape):
    x, m = LR.eps_case(shape)
    ref, o32 = LR.seg_loss(x, m), LR.seg_loss_fp32(x, m)
    bad = as_kernel(LR.seg_loss(x, m, fault="no_eps"))
    assert rejected({"out": bad["out"]}, ref, o32, exact=SEG_EXACT) and rejected({"grad": bad["grad"]}, ref, o32)
    assert not rejected(as_kernel(ref), ref, o32, exact=SEG_EXACT)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("fault", ["drop_pixel", "swap_class"])
def test_comparer_rejects_one_wrong_pixel_at_the_capped_shape(C, fault):
    """one pixel of 1 052 651: the count is off by one (exact items) and its gradient element is wrong (max norm; the L2 ratio of
    the older test, about 1e-3 for one element of a million, is what let such an error through)"""
    x, m, _ = LR.seg_case(("capped", C, "n2", "random"))
    ref, o32 = LR.seg_loss(x, m), LR.seg_loss_fp32(x, m)
    bad = as_kernel(LR.seg_loss(x, m, fault=fault))
    assert rejected({"grad": bad["grad"]}, ref, o32)
    if fault == "drop_pixel" or C == 1:
        exact = SEG_EXACT if C == 1 else (4,) + SEG_EXACT
        fails, _ = LR.compare({"out": bad["out"]}, ref, o32, exact=exact)
        assert any("exactly" in f for f in fails), fails
    assert not rejected(as_kernel(ref), ref, o32, exact=SEG_EXACT)


def test_comparer_rejects_gscale_applied_twice():
    x, m, _ = LR.seg_case(("ragged", 3, "n2", "random"))
    kw = dict(gout=3.0, gscale=1.0 / 1024)
    ref, o32 = LR.seg_loss(x, m, **kw), LR.seg_loss_fp32(x, m, **kw)
    assert rejected({"grad": as_kernel(LR.seg_loss(x, m, fault="gscale_twice", **kw))["grad"]}, ref, o32)
    xj, mj = LR.jaccard_case(("ragged", "n2", "random"))
    ref, o32 = LR.jaccard_seg_loss(xj, mj, **kw), LR.jaccard_seg_loss_fp32(xj, mj, **kw)
    assert rejected({"grad": as_kernel(LR.jaccard_seg_loss(xj, mj, fault="gscale_twice", **kw))["grad"]}, ref, o32)
    assert not rejected(as_kernel(ref), ref, o32, exact=(3,))
    xm, tm = LR.mean_case(0, 257, "planted")
    ref, o32 = LR.mean_loss(xm, tm, 0.9, 0, **kw), LR.mean_loss_fp32(xm, tm, 0.9, 0, **kw)
    assert rejected({"grad": as_kernel(LR.mean_loss(xm, tm, 0.9, 0, fault="gscale_twice", **kw))["grad"]}, ref, o32)


def test_l1_sign_at_ties_is_checked_exactly():
    x, t = LR.mean_case(3, 4099, "planted")
    want = LR.l1_grad_exact(x, t, 3.0, 1.0 / 1024)
    good = as_kernel(LR.mean_loss(x, t, 0.0, 3, gout=3.0, gscale=1.0 / 1024))["grad"]
    bad = as_kernel(LR.mean_loss(x, t, 0.0, 3, gout=3.0, gscale=1.0 / 1024, fault="l1_tie_plus"))["grad"]
    assert E.mismatches(good, want).numel() == 0
    assert E.mismatches(bad, want).numel() == int((x == t).sum()) > 300
