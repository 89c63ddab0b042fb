"""The yardsticks of tests/test_wide_ends_kernels_gpu.py, proved on the CPU (no GPU, no native library).

Wide stem (gs_conv_widecin_fwd_split): an fp32 convolution of the UNROUNDED image followed by the hi/lo split stays inside
pair_tol of the fp64 convolution, while a kernel that rounded the image to 16 bits first, or lost one input channel, lies at
least ten times outside it -- so pair_tol can tell the fp32 stem from the 16-bit engine's model of a wide image.

Wide head (gs_head1x1_fwd_split, 5..64 classes): 64 fp32 terms, added as the kernel adds them, stay inside 1e-6 * scale + 1e-6 at
any class count, while a dropped bias or a dropped input channel exceeds ten times that."""
import pytest
import torch
import torch.nn.functional as F

from tests import pair_reference as pr

# (N, Cin, H, W, Cout): the stem cases of tests/test_wide_ends_kernels_gpu.py
STEM_CASES = [(2, 5, 45, 53, 64), (2, 8, 45, 53, 64), (1, 13, 17, 19, 64), (2, 6, 16, 40, 32), (1, 64, 20, 36, 64), (3, 3, 33, 64, 64)]
HEAD_CASES = [(2, 18, 22, 5), (2, 18, 22, 9), (2, 18, 22, 21), (2, 18, 22, 64), (1, 33, 64, 5), (1, 33, 64, 64), (3, 45, 53, 9),
              (2, 18, 22, 1), (2, 18, 22, 4)]


def stem_inputs(N, Cin, H, W, Cout):
    g = torch.Generator().manual_seed(Cin * 100 + Cout)
    x = torch.rand(N, Cin, H, W, generator=g)
    w = (torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) / (9 * Cin) ** 0.5
    return x, w


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("case", STEM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fp32_stem_is_inside_pair_tol_and_its_defects_are_not(dtn, dt, case):
    N, Cin, H, W, Cout = case
    x, w = stem_inputs(*case)
    ref = F.conv2d(x.double(), w.double(), padding=1)
    scale = float(ref.abs().max())
    tol = pr.pair_tol(dt, scale)
    hi, lo = pr.split(F.conv2d(x, w, padding=1), dt)
    err = float((hi.double() + lo.double() - ref).abs().max())
    rounded = float((F.conv2d(x.to(dt).double(), w.double(), padding=1) - ref).abs().max())
    worst_drop = None
    for c in sorted({0, Cin // 2, Cin - 1}):
        xd = x.clone()
        xd[:, c] = 0
        dropped = float((F.conv2d(xd.double(), w.double(), padding=1) - ref).abs().max())
        worst_drop = dropped if worst_drop is None else min(worst_drop, dropped)
    print(f"stem {case} {dtn}: fp32+split {err:.2e}  tol {tol:.2e}  16-bit image {rounded:.2e}  dropped channel {worst_drop:.2e}")
    assert err < tol, (err, tol)
    assert rounded > 10 * tol, (rounded, tol)
    assert worst_drop > 10 * tol, (worst_drop, tol)


def head_kernel_order_fp32(v, w, b):
    """logits as the head kernels add them: eight 8-term fp32 chains per class, joined as a tree, then the bias"""
    p = v.float()[..., None, :] * w.float()                      # [..., ncls, 64] fp32 products
    p = p.reshape(*p.shape[:-1], 8, 8)
    t = torch.zeros_like(p[..., 0])
    for i in range(8):
        t = t + p[..., i]
    s = ((t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])) + ((t[..., 4] + t[..., 5]) + (t[..., 6] + t[..., 7]))
    return s + b.float()


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("N,H,W,ncls", HEAD_CASES)
def test_fp32_head_is_inside_its_tolerance_and_its_defects_are_not(dtn, dt, N, H, W, ncls):
    g = torch.Generator().manual_seed(ncls + H)
    v = torch.randn(N, H, W, 64, generator=g)
    x_hi, x_lo = pr.split(v, dt)
    w = (torch.rand(ncls, 64, generator=g) * 2 - 1) / 8
    b = torch.randn(ncls, generator=g) * 0.1
    val = x_hi.double() + x_lo.double()
    ref = val @ w.double().t() + b.double()
    scale = float(ref.abs().max())
    tol = 1e-6 * scale + 1e-6
    got = head_kernel_order_fp32((x_hi.float() + x_lo.float()), w, b)
    err = float((got.double() - ref).abs().max())
    print(f"head ncls={ncls} {dtn}: fp32 {err:.2e} tol {tol:.2e}")
    assert err < tol, (err, tol)
    for c in range(ncls):                                        # one class without its bias: every logit of it moves by |b[c]|
        assert abs(float(b[c])) > 10 * tol, (c, float(b[c]), tol)
    for ci in (0, 31, 63):                                       # one input channel lost
        wd = w.double().clone()
        wd[:, ci] = 0
        assert float((val @ wd.t() + b.double() - ref).abs().max()) > 10 * tol
