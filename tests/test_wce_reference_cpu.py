"""tests/wce_reference.py proven on the CPU (no GPU, no native library): the fp64 statement of the class-weighted cross-entropy
agrees with torch's F.cross_entropy(weight=) run in fp64, in value and in autograd gradient, on every case with W != 0; the case
lists cross the block caps they are meant to cross; the comparer the GPU test uses rejects every planted error of
wce_reference.FAULTS while it accepts an fp32 evaluation; header and binding declare the three entry points at ABI 54; and
losses.weighted_cross_entropy refuses what it has to refuse before it touches a device."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import loss_reference as LR
from tests import wce_reference as WR

TIGHT = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b, tol=TIGHT):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_case_lists_cross_the_block_caps():
    N, S = WR.SHAPES["fwd_cap"]
    assert S % 4 == 0 and WR.FWD_MAX_BLOCKS < math.ceil(N * S / 4 / 256) <= WR.FWD_MAX_BLOCKS + 1       # vector path, one block over
    assert math.ceil(N * S / 256) > WR.FWD_MAX_BLOCKS                                                    # and the scalar path
    N, S = WR.SHAPES["bwd_cap"]
    assert S % 4 == 0 and WR.BWD_MAX_BLOCKS < math.ceil(N * S / 4 / 256) <= WR.BWD_MAX_BLOCKS + 1
    assert 4 * N * S < 2 ** 24                                      # sums of multiples of 1/4 up to 1 stay exact in fp32
    assert max(WR.DYADIC) <= 1.0 and all(float(4 * v).is_integer() for v in WR.DYADIC)
    N, S = WR.SHAPES["ragged"]
    assert S % 2 == 1 and math.ceil(N * S / 256) > 1               # odd: the scalar path, more than one block
    N, S = WR.SHAPES["aligned"]
    assert S % 4 == 0 and N > 1 and math.ceil(N * S / 4 / 256) > 1
    assert WR.SHAPES["one"] == (1, 1)
    for s in WR.SMALL:
        assert WR.CLASSES[s] == (2, 3, 4, 5, 9, 64)
    for s in WR.CAPPED:
        assert WR.CLASSES[s] == (2, 3)
        runs = [WR.runs_of(c)[0] for c in WR.CASES if c[0] == s]
        assert {k for k, _ in runs} == set(WR.WEIGHTS)
        sc = [t[0] for _, t in runs]
        assert {a for a, _, _ in sc} == {None, 3.0} and {b for _, b, _ in sc} == {1.0, 1.0 / 1024} and {c for _, _, c in sc} == {1, 4}
    assert all(n * s <= 1 << 20 for k, (n, s) in WR.SHAPES.items() if k in WR.SMALL)
    assert {c[0] for c in WR.CASES} == set(WR.SHAPES) and {c[2] for c in WR.CASES} == set(LR.FAMILIES) and {c[3] for c in WR.CASES} == set(LR.MASKS)


@pytest.mark.parametrize("case", [c for c in WR.CASES if c[0] in WR.SMALL], ids=WR.case_id)
def test_statement_is_torch_cross_entropy_in_fp64(case):
    x, t = WR.wce_case(case)
    for kind in WR.WEIGHTS:
        w = WR.class_weights(kind, case[1], t)
        r = WR.wce(x, t, w)
        if float(r["out"][2]) == 0.0:
            assert kind in ("one_zero", "present_zero") and math.isnan(float(r["out"][0]))
            continue
        v = x.double().requires_grad_(True)
        y = F.cross_entropy(v, t.long(), weight=None if w is None else w.double())
        y.backward()
        assert close(r["out"][0], y.detach()), (kind, float(r["out"][0]), float(y))
        assert LR.grad_error(r["grad"], v.grad) <= TIGHT, kind
        assert close(r["out"][0], r["out"][1] / r["out"][2])
        assert float(r["out"][3]) == 1.0 and not r["out"][4:].any()
        r2 = WR.wce(x, t, w, gout=3.0, gscale=1.0 / 1024)                  # upstream gradient and scale are plain factors
        assert LR.grad_error(r2["grad"], v.grad * 3.0 / 1024) <= TIGHT and torch.equal(r2["out"], r["out"])
    assert bool((WR.class_weights("present_zero", case[1], t)[t.long()] == 0).all())


@pytest.mark.parametrize("case", [c for c in WR.CASES if c[0] in WR.CAPPED and c[2] == "n2" and c[3] == "random"], ids=WR.case_id)
def test_statement_is_torch_cross_entropy_in_fp64_at_the_caps(case):
    x, t = WR.wce_case(case)
    w = WR.class_weights("reference", case[1], t)
    r = WR.wce(x, t, w)
    v = x.double().requires_grad_(True)
    y = F.cross_entropy(v, t.long(), weight=w.double())
    y.backward()
    assert close(r["out"][0], y.detach()) and LR.grad_error(r["grad"], v.grad) <= TIGHT


@pytest.mark.parametrize("C", [2, 3])
def test_world_of_four_is_the_global_weighted_mean(C):
    """rank 0 of four with the other ranks' (numerator, W): the global quotient, and world x the full-batch gradient of the rank's
    slice (the data-parallel exchange averages over the ranks); a per-rank mean is NOT the global mean"""
    case = ("ragged", C, "n2", "random")
    x, t = WR.wce_case(case)
    w = WR.class_weights("reference", C)
    from tests import exact_reference as E
    g = E.generator(("wce_world_full", C))
    xs = [x] + [LR.draw_logits(g, (3, C, 315), "n2") for _ in range(3)]
    ts = [t] + [LR.draw_mask(g, 3, C, 1, 315, "random").reshape(3, 315) for _ in range(3)]
    others = sum(WR.wce(xs[k], ts[k], w)["out"][1:3] for k in (1, 2, 3))
    r = WR.wce(x, t, w, others=others, world=4)
    v = torch.cat(xs).double().requires_grad_(True)
    y = F.cross_entropy(v, torch.cat(ts).long(), weight=w.double())
    y.backward()
    assert close(r["out"][0], y.detach()) and float(r["out"][3]) == 4.0
    assert LR.grad_error(r["grad"], 4.0 * v.grad[:3]) <= TIGHT
    means = torch.stack([WR.wce(xs[k], ts[k], w)["out"][0] for k in range(4)])
    assert abs(float(means.mean()) - float(y.detach())) > 1e-6
    # losses.apply_global_mean writes the same numbers
    from semantic_segmentation_amd.losses import apply_global_mean
    local = WR.wce(x, t, w)["out"].clone()
    apply_global_mean(local, local[1:3] + others, 4)
    assert close(local, r["out"])


FAULT_CASE = ("ragged", 3, "planted", "random")


@pytest.mark.parametrize("fault", WR.FAULTS)
def test_comparer_rejects_each_fault(fault):
    x, t = WR.wce_case(FAULT_CASE)
    w = WR.class_weights("reference", FAULT_CASE[1], t)
    kw = dict(gout=3.0, gscale=1.0 / 1024)
    ref, o32 = WR.wce(x, t, w, **kw), WR.wce_fp32(x, t, w, **kw)
    bad = WR.wce(x, t, w, fault=fault, **kw)
    if fault == "last_max":                                          # the label map is compared byte for byte
        assert int((x[:, 0] == x[:, 1]).sum()) > 0                   # planted ties
        assert not torch.equal(bad["labels"], ref["labels"])
        assert torch.equal(bad["out"], ref["out"])
        return
    assert torch.equal(bad["labels"], ref["labels"])
    fails, _ = LR.compare({"out": bad["out"].float(), "grad": bad["grad"].float()}, ref, o32, exact=WR.exact_indices("reference"),
                          what=fault)
    assert fails, fault


@pytest.mark.parametrize("case", [c for c in WR.CASES if c[0] in WR.SMALL and c[1] in (2, 5, 64)], ids=WR.case_id)
def test_comparer_accepts_a_correct_fp32_evaluation(case):
    """a second fp32 evaluation (the statement's own expressions rounded to fp32 at the end is too good; this one is torch's
    log_softmax + nll_loss in fp32) passes the comparer at every weight kind with W != 0"""
    x, t = WR.wce_case(case)
    for kind in WR.WEIGHTS:
        w = WR.class_weights(kind, case[1], t)
        ref = WR.wce(x, t, w, gout=3.0, gscale=1.0 / 1024)
        if float(ref["out"][2]) == 0.0:
            continue
        o32 = WR.wce_fp32(x, t, w, gout=3.0, gscale=1.0 / 1024)
        v = x.clone().requires_grad_(True)
        ls = F.log_softmax(v, dim=1)
        wt = torch.ones(t.shape) if w is None else w[t.long()]
        num = -(wt * ls.gather(1, t.long().unsqueeze(1))[:, 0]).sum()
        W = wt.sum()
        (num / W * (3.0 / 1024)).backward()
        z = torch.tensor(0.0)
        got = {"out": torch.stack([(num / W).detach(), num.detach(), W, torch.tensor(1.0), z, z, z, z]), "grad": v.grad}
        fails, _ = LR.compare(got, ref, o32, exact=WR.exact_indices(kind), what=kind)
        assert not fails, fails


def test_header_and_binding_declare_the_entry_points():
    from semantic_segmentation_amd import _lib
    with open(os.path.join(ROOT, "include", "gsseg.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+GS_ABI_VERSION\s+54\b", h) and _lib.ABI_VERSION == 54
    for name in ("gs_wce_fwd", "gs_wce_bwd", "gs_wce_ws_floats"):
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    for line in ("train_unet.py:135,155,170", "config.py:35", "train_end2end.py:139,189,203,215"):
        assert line in h, line
    assert len(_lib.PROTOTYPES["gs_wce_fwd"][1]) == 10 and len(_lib.PROTOTYPES["gs_wce_bwd"][1]) == 11
    assert _lib.PROTOTYPES["gs_wce_ws_floats"][1] == []
    with open(os.path.join(ROOT, "semantic_segmentation_amd", "csrc", "loss.hip")) as f:
        src = f.read()
    assert "WCE_FWD_MAX_BLOCKS = LOSS_MAX_BLOCKS" in src and "LOSS_MAX_BLOCKS = %d" % WR.FWD_MAX_BLOCKS in src
    assert "WCE_BWD_MAX_BLOCKS = %d" % WR.BWD_MAX_BLOCKS in src


def test_weighted_cross_entropy_refuses_bad_arguments():
    from semantic_segmentation_amd.losses import WeightedCrossEntropyLoss, weighted_cross_entropy
    x = torch.zeros(1, 2, 4, 4, 4)
    t = torch.zeros(1, 4, 4, 4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU path"):
        weighted_cross_entropy(x, t, (0.004, 0.996))
    with pytest.raises(RuntimeError, match="no CPU path"):
        WeightedCrossEntropyLoss((0.004, 0.996))(x, t)
    with pytest.raises(ValueError):
        weighted_cross_entropy(torch.zeros(1, 1, 4, 4, 4), t)                      # C == 1
    with pytest.raises(ValueError):
        weighted_cross_entropy(x, t, (-0.1, 1.0))
    with pytest.raises(ValueError):
        weighted_cross_entropy(x, t, (float("nan"), 1.0))
    with pytest.raises(ValueError):
        weighted_cross_entropy(x, t, (float("inf"), 1.0))
    with pytest.raises(ValueError):
        weighted_cross_entropy(x, t, (0.1, 0.2, 0.7))                              # wrong length
    with pytest.raises(ValueError):
        weighted_cross_entropy(x, t, torch.tensor([0.1, 0.2, 0.7]))
    with pytest.raises(ValueError):
        weighted_cross_entropy(torch.zeros(1, 2), torch.zeros(1, dtype=torch.long))   # no spatial dim
