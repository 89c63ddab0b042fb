"""gs_head1x1_labels and gs_labels_from_logits on the GPU (`-m gpu`): the exact cases of tests/label_head_cases.py, every byte equal
to the labels the predicate gives on the fp64 logits -- planted ties go to the lower class index, a logit of exactly 0 gives label 0.
Rejected arguments return an error and leave the output untouched."""
import pytest
import torch

from tests import exact_reference as E
from tests import label_head_cases as LH

pytestmark = pytest.mark.gpu

SENT = 255                                                   # no case has 256 classes: a byte the kernel did not write
_CACHE = {}


def dev():
    return torch.device("cuda:0")


def cached(case, bn):
    if (case, bn) not in _CACHE:
        _CACHE[(case, bn)] = LH.build(case, bn)
    return _CACHE[(case, bn)]


def sentinel(*shape):
    return torch.full(shape, SENT, dtype=torch.uint8, device=dev())


@pytest.mark.parametrize("dtn,dt", E.DTS)
@pytest.mark.parametrize("case", LH.CASES, ids=LH.case_id)
def test_head1x1_labels_exact(case, dtn, dt):
    """the pair head with the label epilogue, on an activation pair and on a conv-output pair with BatchNorm + ReLU on the load path"""
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd._lib import ACT_RELU
    N, H, W = LH.SHAPES[case[0]]
    for bn in (False, True):
        c = cached(case, bn)
        what = f"labels {LH.case_id(case)} {'bn' if bn else 'plain'} {dtn} [n][y][x]"
        hi, lo = c["hi"].to(dt).to(dev()), c["lo"].to(dt).to(dev())
        lab = sentinel(N, H, W)
        if bn:
            ops.head1x1_labels(hi, lo, c["w"].to(dev()), c["b"].to(dev()), lab, c["scale"].to(dev()), c["shift"].to(dev()), ACT_RELU)
        else:
            ops.head1x1_labels(hi, lo, c["w"].to(dev()), c["b"].to(dev()), lab)
        torch.cuda.synchronize()
        E.assert_exact(lab, c["labels"], what)
        # without a bias: the labels of the logits without it
        if not bn:
            lab0 = sentinel(N, H, W)
            ops.head1x1_labels(hi, lo, c["w"].to(dev()), None, lab0)
            torch.cuda.synchronize()
            E.assert_exact(lab0, LH.predicate(c["logits"] - c["b"].double()).view(N, H, W), what + " no bias")


@pytest.mark.parametrize("case", LH.CASES, ids=LH.case_id)
def test_labels_from_logits_exact(case):
    """the same predicate on the stored fp32 logits of the same cases (the plain and the BatchNorm variant's)"""
    from semantic_segmentation_amd import ops
    N, H, W = LH.SHAPES[case[0]]
    for bn in (False, True):
        c = cached(case, bn)
        lab = sentinel(N, H, W)
        ops.labels_from_logits(LH.logits_nchw(c).to(dev()), lab)
        torch.cuda.synchronize()
        E.assert_exact(lab, c["labels"], f"labels_from_logits {LH.case_id(case)} {'bn' if bn else 'plain'} [n][y][x]")


def test_labels_from_logits_70_classes():
    from semantic_segmentation_amd import ops
    x, want = LH.build_wide_logits()
    lab = sentinel(*want.shape)
    ops.labels_from_logits(x.to(dev()), lab)
    torch.cuda.synchronize()
    E.assert_exact(lab, want, "labels_from_logits C=70 [n][y][x]")
    # a volume's logits [NB*D, C, H, W] give the labels of [NB, D, H, W] in place: the flat order is the same
    lab5 = sentinel(1, *want.shape)
    ops.labels_from_logits(x.to(dev()), lab5)
    torch.cuda.synchronize()
    assert torch.equal(lab5.view(-1).cpu(), want.view(-1))


def test_label_entry_points_refuse_bad_arguments():
    """65 classes, 257 logit planes, an x pointer 8 bytes off a 16-byte boundary: GS_EINVAL with a message, nothing launched, the
    output bytes untouched"""
    from semantic_segmentation_amd import _lib
    lib = _lib.load()
    M = 256
    x = torch.zeros(2, M + 1, 64, dtype=torch.float16, device=dev())
    w = torch.zeros(65, 64, dtype=torch.float32, device=dev())
    lab = sentinel(M)
    assert x[0].data_ptr() % 16 == 0
    rc = lib.gs_head1x1_labels(x[0].data_ptr(), x[1].data_ptr(), None, None, 0, w.data_ptr(), None, lab.data_ptr(), M, 65, 0, None)
    assert rc == -1 and b"gs_head1x1_labels" in lib.gs_last_error() and b"65" in lib.gs_last_error()
    rc = lib.gs_head1x1_labels(x[0].data_ptr() + 8, x[1].data_ptr(), None, None, 0, w.data_ptr(), None, lab.data_ptr(), M, 2, 0, None)
    assert rc == -1 and b"aligned" in lib.gs_last_error()
    rc = lib.gs_head1x1_labels(x[0].data_ptr(), x[1].data_ptr() + 8, None, None, 0, w.data_ptr(), None, lab.data_ptr(), M, 9, 0, None)
    assert rc == -1 and b"aligned" in lib.gs_last_error()
    lg = torch.zeros(1, 257, 8, dtype=torch.float32, device=dev())
    rc = lib.gs_labels_from_logits(lg.data_ptr(), lab.data_ptr(), 1, 257, 8, None)
    assert rc == -1 and b"gs_labels_from_logits" in lib.gs_last_error() and b"257" in lib.gs_last_error()
    torch.cuda.synchronize()
    assert bool((lab == SENT).all())
