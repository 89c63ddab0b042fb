"""Exact-integer cases of the wide pointwise head (Cin == 64, 5..64 classes): shared by tests/test_wide_head_reference_cpu.py (every
case meets the conditions of tests/exact_reference.py) and tests/test_wide_head_kernels_gpu.py (kernel against reference at zero
tolerance).  Plain torch on the CPU; no GPU, no native library."""
import torch.nn.functional as F

from tests import exact_reference as E

COUTS = (5, 8, 9, 33, 64)
VSETS = ("S", "P")
# "small": E.smallcout_build's 2 x 11 x 9 = 198 pixels, less than one block of any of the kernels.
# "ragged": 3 x 37 x 29 = 3219 pixels -- no multiple of 32, 64, 128 or 256, several blocks of the forward / data-gradient kernels
#           and several slabs (64-pixel stages, a partial last one) of the weight gradient.
# "partial": 1 x 19 x 21 = 399 pixels -- the data gradient's second pixel per thread (256 further on) exists for 143 threads only.
SHAPES = {"small": (2, 11, 9), "ragged": (3, 37, 29), "partial": (1, 19, 21)}
CASES = [(shape, cout) for shape in SHAPES for cout in COUTS]


def case_id(case):
    return f"{case[0]}-{case[1]}"


def build(case, vset):
    """x [N,64,H,W], w [Cout,64,1,1], b [Cout], dy [N,Cout,H,W] integers; y, dx, dw, db their exact fp64 results"""
    shape, cout = case
    if shape == "small":
        return E.smallcout_build((64, cout, 1, 0), vset)
    N, H, W = SHAPES[shape]
    c = E.conv_case(("wide_head", N, H, W, cout), vset, (N, 64, H, W), (cout, 64, 1, 1), lambda x, w: F.conv2d(x, w, None),
                    64, cout, N * H * W, bias=True)
    c["db"] = c["dy"].double().sum((0, 2, 3))
    return c
