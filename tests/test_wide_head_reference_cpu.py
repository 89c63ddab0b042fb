"""CPU checks for the wide pointwise head (5..64 classes): the exact-integer case list meets the conditions under which a
zero-tolerance comparison is valid, and the new entry points are declared, bound and exported.  No GPU."""
import os
import re

import pytest
import torch

from tests import exact_reference as E
from tests import wide_head_cases as WH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gs_head1x1_wide_bwd", "gs_head1x1_wide_bwd_ws_floats", "gs_head1x1_wide_fwd")


@pytest.mark.parametrize("vset", WH.VSETS)
@pytest.mark.parametrize("case", WH.CASES, ids=WH.case_id)
def test_wide_head_cases_meet_the_exactness_conditions(case, vset):
    """build() asserts require_integers / require_products for y, dx and dw; here also: the bias gradient and every gradient stay
    below 2^24 in absolute-value form, the scaled expectations are fp32 numbers, and both 16-bit roundings of dx exist"""
    r = WH.build(case, vset)
    N, H, W = WH.SHAPES[case[0]]
    cout = case[1]
    assert tuple(r["x"].shape) == (N, 64, H, W) and tuple(r["dy"].shape) == (N, cout, H, W) and tuple(r["w"].shape) == (cout, 64, 1, 1)
    E.require_integers(r["x"], r["w"], r["dy"], r["b"])
    px = N * H * W
    assert px * float(r["dy"].abs().max()) < E.LIMIT                                     # db
    assert px * float(r["dy"].abs().max()) * float(r["x"].abs().max()) < E.LIMIT         # dw
    assert cout * float(r["dy"].abs().max()) * float(r["w"].abs().max()) < E.LIMIT       # dx
    assert max(float(r["dw"].abs().max()), float(r["db"].abs().max()), float(r["dx"].abs().max())) < E.LIMIT
    assert float(r["dx"].abs().max()) <= 2048                                            # an integer every fp16 value holds exactly
    E.expect32(r["dw"], 0.5)
    E.expect32(r["db"], 0.5)
    E.expect32(r["y"].double() + r["b"].double().view(1, -1, 1, 1))
    for _, dt in E.DTS:
        assert torch.isfinite(E.expect16(E.channels_last(r["dx"]), dt).float()).all()
    # the reference does not depend on the order of the class sum: the same dx from the classes in reverse
    dx_rev = torch.einsum("nchw,ck->nkhw", r["dy"].flip(1).double(), r["w"][:, :, 0, 0].flip(0).double())
    assert torch.equal(dx_rev, r["dx"].double())


def test_wide_head_symbols_are_declared_bound_and_exported():
    from semantic_segmentation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gsseg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in gsseg.h"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert int(re.search(r"#define GS_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == lib.gs_abi_version()
    # the reference lines the new entry points serve are cited next to them
    for cite in ("unet/unet_parts.py:71-77", "GenSeg-3D/UNet3D/unet3d.py", "unet/evaluate.py:34-40"):
        assert cite in hdr, cite


def test_wide_head_workspace_query_and_synchronous_argument_checks():
    """the workspace grows with the class count and covers one slab; bad class counts / dtypes are refused before any device work
    (NULL pointers here: a launch would fault, a refusal returns GS_EINVAL)"""
    from semantic_segmentation_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    q = lib.gs_head1x1_wide_bwd_ws_floats
    assert q(2, 37, 29, 9) >= 9 * 64 + 64 and q(2, 37, 29, 64) > q(2, 37, 29, 9)
    assert q(8, 256, 256, 64) >= q(2, 37, 29, 64)
    assert q(1, 8, 8, 0) == 0 and q(1, 8, 8, 65) == 0
    for ncls, dtype in ((0, 0), (65, 0), (9, 7)):
        assert lib.gs_head1x1_wide_bwd(None, None, None, None, None, None, None, 1, 8, 8, ncls, 1.0, dtype, None) == -1
        assert b"gs_head1x1_wide_bwd" in lib.gs_last_error()
        assert lib.gs_head1x1_wide_fwd(None, None, None, None, 1, 8, 8, ncls, dtype, None) == -1
        assert b"gs_head1x1_wide_fwd" in lib.gs_last_error()
