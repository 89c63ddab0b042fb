"""CPU checks for the label head: every case of tests/label_head_cases.py meets the conditions under which the GPU test may compare
every byte (exact operands, exact sums in any order), the planted ties and zero logits are there so that the GPU test cannot pass
vacuously, and the two entry points are declared, bound and exported with ABI 54.  No GPU."""
import os
import re

import pytest
import torch

from tests import exact_reference as E
from tests import label_head_cases as LH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gs_head1x1_labels", "gs_labels_from_logits")


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("case", LH.CASES, ids=LH.case_id)
def test_label_head_cases_are_exact_and_not_vacuous(case, bn):
    c = LH.build(case, bn)
    shape, ncls = case
    N, H, W = LH.SHAPES[shape]
    M = N * H * W
    hi, lo = c["hi"], c["lo"]
    assert tuple(hi.shape) == (N, H, W, 64) == tuple(lo.shape) and tuple(c["w"].shape) == (ncls, 64) and tuple(c["b"].shape) == (ncls,)
    # operands: integer hi / weights / biases / shifts, dyadic lo, power-of-two scales; both 16-bit types hold hi and lo exactly
    E.require_integers(hi, c["w"], c["b"], c["shift"])
    assert torch.equal(lo / LH.LO_UNIT, (lo / LH.LO_UNIT).round()) and float(lo.abs().max()) <= 3 * LH.LO_UNIT
    for s in c["scale"].tolist():
        E.require_pow2(s)
    assert float(c["scale"].min()) >= 0.25 and float(c["scale"].max()) <= 1.0
    if not bn:
        assert torch.equal(c["scale"], torch.ones(64)) and torch.equal(c["shift"], torch.zeros(64))
    for _, dt in E.DTS:
        assert torch.equal(hi.to(dt).float(), hi) and torch.equal(lo.to(dt).float(), lo)
    # every term is a multiple of u = 2^-4 (plain) / 2^-6 (scales down to 1/4), and the sum of the absolute terms of a class stays
    # below 2^24 u: every partial sum is exact in fp32, in any order, fused or not
    u = LH.LO_UNIT * (0.25 if bn else 1.0)
    z = LH.activation(c)
    assert torch.equal(z / u, (z / u).round())
    assert (64 * float(z.abs().max()) * float(c["w"].abs().max()) + float(c["b"].abs().max())) / u < E.LIMIT
    z32 = LH.activation(c, torch.float32)
    assert torch.equal(z32.double(), z)                                   # the load path itself is exact in fp32
    order = torch.randperm(64, generator=E.generator(("order", case, bn)))
    for idx in (torch.arange(63, -1, -1), order):
        acc = torch.zeros(M, ncls)
        for i in idx.tolist():                                            # one channel at a time, fp32
            acc = acc + z32[:, i:i + 1] * c["w"][:, i].view(1, -1)
        assert torch.equal((acc + c["b"]).double(), c["logits"])
    assert torch.equal(LH.logits_nchw(c).permute(0, 2, 3, 1).reshape(M, ncls).double(), c["logits"])
    # expected labels: the predicate on the fp64 logits; the fp32 evaluation of it agrees (the logits are the same numbers)
    lab = c["labels"].view(-1)
    assert lab.dtype == torch.uint8 and torch.equal(LH.predicate(c["logits"].float()), lab)
    lg = c["logits"]
    if ncls == 1:
        zero = lg[:, 0] == 0
        assert float(zero.float().mean()) >= LH.TIE_SHARE, float(zero.float().mean())
        assert int(lab[zero].max()) == 0                                 # sigmoid(0) = 0.5 is not > 0.5
        assert torch.equal(lab, (lg[:, 0] > 0).to(torch.uint8))
        assert set(lab.unique().tolist()) == {0, 1}
        assert bool(zero[c["planted"]].all())
    else:
        src, dst = c["src"], c["dst"]
        assert 0 <= src < dst < ncls
        assert torch.equal(lg[:, src], lg[:, dst])                        # an exact tie at every pixel
        at_max = lg[:, src] == lg.max(1).values
        assert float(at_max.float().mean()) >= LH.TIE_SHARE, float(at_max.float().mean())
        first = lg[:, :src].max(1).values < lg[:, src] if src > 0 else torch.ones(M, dtype=torch.bool)
        assert torch.equal(lab[at_max & first], torch.full((int((at_max & first).sum()),), src, dtype=torch.uint8))
        assert float((at_max & first).float().mean()) >= LH.TIE_SHARE
        # every class index that can win does win somewhere; dst, the copy behind src, never does
        assert set(lab.unique().tolist()) == set(range(ncls)) - {dst}
        # arg-max with ties to the lowest index, restated
        want = torch.tensor([min(j for j in range(ncls) if row[j] == max(row)) for row in lg.tolist()], dtype=torch.uint8)
        assert torch.equal(lab, want)


def test_wide_logits_case_has_ties_and_every_byte_is_a_class():
    x, lab = LH.build_wide_logits()
    C = LH.WIDE_LOGITS_C
    assert x.shape[1] == C > 64 and lab.dtype == torch.uint8 and int(lab.max()) < C
    flat = x.permute(0, 2, 3, 1).reshape(-1, C)
    ties = (flat == flat.max(1, keepdim=True).values).sum(1) > 1
    assert float(ties.float().mean()) >= 0.5
    want = torch.tensor([row.index(max(row)) for row in flat.tolist()], dtype=torch.uint8)
    assert torch.equal(lab.view(-1), want)
    assert int(lab.max()) > 64                                            # a label beyond the pair head's class range occurs


def test_label_head_symbols_are_declared_bound_and_exported_with_abi_54():
    from semantic_segmentation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gsseg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in gsseg.h"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype in _lib.py"
    assert int(re.search(r"#define GS_ABI_VERSION (\d+)", hdr).group(1)) == 54 == _lib.ABI_VERSION
    for cite in ("GenSeg-3D/train_unet.py:39", "unet/evaluate.py:29-40"):
        assert cite in hdr, cite
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.gs_abi_version() == 54
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by the library"


def test_label_head_refuses_bad_arguments_before_any_device_work():
    """NULL pointers: a launch would fault, a refusal returns GS_EINVAL with the entry point's name in the message"""
    from semantic_segmentation_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    for ncls, dtype in ((0, 0), (65, 0), (9, 7)):
        assert lib.gs_head1x1_labels(None, None, None, None, 0, None, None, None, 64, ncls, dtype, None) == -1
        assert b"gs_head1x1_labels" in lib.gs_last_error()
    for C in (0, 257):
        assert lib.gs_labels_from_logits(None, None, 1, C, 64, None) == -1
        assert b"gs_labels_from_logits" in lib.gs_last_error()
