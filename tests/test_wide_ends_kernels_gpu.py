"""The end kernels of the pair forward for any channel / class count, each against fp64 (GPU only, `-m gpu`):
gs_conv_widecin_fwd_split (fp32 image of 1..64 channels -> conv-output pair + BatchNorm partial rows, csrc/stem_wide.hip) and the
5..64-class form of gs_head1x1_fwd_split / gs_head1x1_bn_fwd_split.  tests/test_wide_ends_reference_cpu.py proves that the
tolerances used here separate the kernels' arithmetic from a 16-bit image, a lost channel or a lost bias."""
import pytest
import torch
import torch.nn.functional as F

from tests import pair_reference as pr

pytestmark = pytest.mark.gpu

SENT = 7.0                                                   # finite sentinel in output buffers
ACT_RELU = 1
# (N, Cin, H, W, Cout): ragged with K odd before padding; Cin a multiple of 8; an image smaller than a patch both ways; the 3-D
# stem's Cout with Cin = 2 * 3; the channel-chunk loop at its full length; the overlap with the narrow kernel
STEM_CASES = [(2, 5, 45, 53, 64), (2, 8, 45, 53, 64), (1, 13, 17, 19, 64), (2, 6, 16, 40, 32), (1, 64, 20, 36, 64), (3, 3, 33, 64, 64)]


def dev():
    return torch.device("cuda:0")


def check_pair(y_hi, y_lo, ref, dt, what=""):
    got = y_hi.double().cpu() + y_lo.double().cpu()
    assert torch.isfinite(got).all(), what
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"{what}: max err {err:.3e} tol {pr.pair_tol(dt, scale):.3e} scale {scale:.3f}")
    assert err < pr.pair_tol(dt, scale), (what, err, pr.pair_tol(dt, scale))
    return got


def check_stat_rows(part, nt, cout, got):
    """BatchNorm partial rows [nt][2][Cout]: slot 0 sums to the column sums of y = y_hi + y_lo, slot 1 to those of y^2"""
    p = part[:nt * 2 * cout].view(nt, 2, cout).double().sum(0).cpu()
    y = got.reshape(-1, cout)
    s1, s2 = y.sum(0), (y * y).sum(0)
    assert float((p[0] - s1).abs().max()) < 1e-5 * float(y.abs().sum(0).max()), float((p[0] - s1).abs().max())
    assert float((p[1] - s2).abs().max()) < 1e-3 * float(s2.max()), float((p[1] - s2).abs().max())


def _bn_ref(val, sc, sh):
    return torch.relu(val * sc.double() + sh.double())


def stem_inputs(N, Cin, H, W, Cout):
    g = torch.Generator().manual_seed(Cin * 100 + Cout)
    x = torch.rand(N, Cin, H, W, generator=g)
    w = (torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) / (9 * Cin) ** 0.5
    return x, w


def run_stem(x, w, dt, with_stats=True):
    from semantic_segmentation_amd import ops
    N, _, H, W = x.shape
    Cout = w.shape[0]
    y_hi = torch.full((N, H, W, Cout), SENT, dtype=dt, device=dev())
    y_lo = torch.full((N, H, W, Cout), SENT, dtype=dt, device=dev())
    nt = ops.conv_widecin_mtiles(N, H, W)
    part = torch.full((ops.bn_partials_numel(nt, Cout),), float("nan"), dtype=torch.float32, device=dev()) if with_stats else None
    ops.conv_widecin_fwd_split(x.to(dev()), w.to(dev()), y_hi, y_lo, part)
    torch.cuda.synchronize()
    return y_hi, y_lo, part, nt


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("case", STEM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_wide_stem_pair_vs_fp64(dtn, dt, case):
    """conv_widecin_fwd_split against the fp64 convolution to pair_tol; its partial rows against the column sums; every output
    element written (the buffers start as a sentinel whose pair value no output takes); two runs bit-identical"""
    N, Cin, H, W, Cout = case
    x, w = stem_inputs(*case)
    y_hi, y_lo, part, nt = run_stem(x, w, dt)
    assert nt == N * ((H + 7) // 8) * ((W + 31) // 32)
    ref = F.conv2d(x.double(), w.double(), padding=1).permute(0, 2, 3, 1)
    got = check_pair(y_hi, y_lo, ref, dt, f"conv_widecin_fwd_split {case} {dtn}")
    assert float(ref.abs().max()) < 2 * SENT - 1 and not bool(((y_hi == SENT) & (y_lo == SENT)).any()), "an output element was left unwritten"
    assert torch.isfinite(part[:nt * 2 * Cout]).all()
    check_stat_rows(part, nt, Cout, got)
    z_hi, z_lo, part2, _ = run_stem(x, w, dt)
    assert torch.equal(y_hi.view(torch.int16), z_hi.view(torch.int16)) and torch.equal(y_lo.view(torch.int16), z_lo.view(torch.int16))
    assert torch.equal(part[:nt * 2 * Cout], part2[:nt * 2 * Cout])


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
def test_wide_stem_without_statistics(dtn, dt):
    """bn_partials = None: the same pair, nothing else written"""
    case = STEM_CASES[0]
    x, w = stem_inputs(*case)
    y_hi, y_lo, part, _ = run_stem(x, w, dt, with_stats=False)
    assert part is None
    w_hi, w_lo, _, _ = run_stem(x, w, dt)
    assert torch.equal(y_hi.view(torch.int16), w_hi.view(torch.int16)) and torch.equal(y_lo.view(torch.int16), w_lo.view(torch.int16))
    check_pair(y_hi, y_lo, F.conv2d(x.double(), w.double(), padding=1).permute(0, 2, 3, 1), dt, "conv_widecin_fwd_split, no statistics")


def test_wide_stem_matches_the_narrow_kernel():
    """Cin = 3: both stems are fp32 products of the same operands; their pairs agree to the fp32 accumulation order (pair_tol)"""
    from semantic_segmentation_amd import ops
    case = STEM_CASES[-1]
    N, Cin, H, W, Cout = case
    x, w = stem_inputs(*case)
    dt = torch.float16
    y_hi, y_lo, _, _ = run_stem(x, w, dt)
    n_hi, n_lo = torch.empty_like(y_hi), torch.empty_like(y_lo)
    part = torch.zeros(ops.bn_partials_numel(ops.conv_smallcin_mtiles(N, H, W), Cout), dtype=torch.float32, device=dev())
    ops.conv_smallcin_fwd_split(x.to(dev()), w.to(dev()), n_hi, n_lo, part, 3, 1)
    torch.cuda.synchronize()
    a, b = y_hi.double() + y_lo.double(), n_hi.double() + n_lo.double()
    assert float((a - b).abs().max()) < pr.pair_tol(dt, float(b.abs().max()))


@pytest.mark.parametrize("Cin,Cout", [(65, 64), (8, 48), (8, 160)])
def test_wide_stem_rejects_shapes_outside_its_range(Cin, Cout):
    """Cin above 64 / Cout not a multiple of 32 in 32..128: unsupported, nothing launched (the outputs keep their sentinel)"""
    from semantic_segmentation_amd import _lib, ops
    N, H, W = 1, 16, 32
    x = torch.zeros(N, Cin, H, W, device=dev())
    w = torch.zeros(Cout, Cin, 3, 3, device=dev())
    y_hi = torch.full((N, H, W, Cout), SENT, dtype=torch.float16, device=dev())
    y_lo = torch.full((N, H, W, Cout), SENT, dtype=torch.float16, device=dev())
    rc = _lib.load().gs_conv_widecin_fwd_split(x.data_ptr(), w.data_ptr(), y_hi.data_ptr(), y_lo.data_ptr(), None, N, Cin, H, W, Cout,
                                               ops.dt_code(y_hi), None)
    assert rc == _lib.GS_EUNSUPPORTED
    with pytest.raises(NotImplementedError):
        ops.conv_widecin_fwd_split(x, w, y_hi, y_lo, None)
    torch.cuda.synchronize()
    assert bool((y_hi == SENT).all()) and bool((y_lo == SENT).all())


def test_wide_stem_rejects_misaligned_planes():
    """the epilogue stores 16-byte channel groups: a plane off a 16-byte boundary is an argument error, not a launch"""
    from semantic_segmentation_amd import _lib, ops
    N, Cin, H, W, Cout = 1, 8, 16, 32, 64
    x = torch.zeros(N, Cin, H, W, device=dev())
    w = torch.zeros(Cout, Cin, 3, 3, device=dev())
    buf = torch.zeros(N * H * W * Cout + 8, dtype=torch.float16, device=dev())
    good = torch.zeros(N, H, W, Cout, dtype=torch.float16, device=dev())
    rc = _lib.load().gs_conv_widecin_fwd_split(x.data_ptr(), w.data_ptr(), buf.data_ptr() + 2, good.data_ptr(), None, N, Cin, H, W, Cout,
                                               ops.dt_code(good), None)
    assert rc == -1                                              # GS_EINVAL


# ------------------------------------------------------------------------------------------------ head
HEAD_SHAPES = [(2, 18, 22, n) for n in (5, 9, 21, 64)] + [(1, 33, 64, n) for n in (5, 9, 21, 64)] + [(3, 45, 53, 9)] + \
              [(2, 18, 22, 1), (2, 18, 22, 4)]                    # 1 and 4 classes: the four-class instance, same formula


@pytest.mark.parametrize("dtn,dt", pr.DTYPES)
@pytest.mark.parametrize("N,H,W,ncls", HEAD_SHAPES)
def test_wide_head_vs_fp64(dtn, dt, N, H, W, ncls):
    """head1x1_fwd_split and head1x1_bn_fwd_split (BatchNorm + ReLU on the load path) for 5..64 classes: fp32 logits against fp64 to
    1e-6 * scale + 1e-6 (64 fp32 terms), every logit written (the buffer starts as NaN)"""
    from semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(ncls + H)
    v = torch.randn(N, H, W, 64, generator=g)
    x_hi, x_lo = pr.split(v, dt)
    w = (torch.rand(ncls, 64, generator=g) * 2 - 1) / 8
    b = torch.randn(ncls, generator=g) * 0.1
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3
    val = x_hi.double() + x_lo.double()
    for bn in (False, True):
        logits = torch.full((N, ncls, H, W), float("nan"), dtype=torch.float32, device=dev())
        if bn:
            ops.head1x1_bn_fwd_split(x_hi.to(dev()), x_lo.to(dev()), sc.to(dev()), sh.to(dev()), ACT_RELU, w.to(dev()), b.to(dev()), logits)
            src = _bn_ref(val, sc, sh)
        else:
            ops.head1x1_fwd_split(x_hi.to(dev()), x_lo.to(dev()), w.to(dev()), b.to(dev()), logits)
            src = val
        torch.cuda.synchronize()
        assert torch.isfinite(logits).all(), "a logit was left unwritten"
        ref = (src @ w.double().t() + b.double()).permute(0, 3, 1, 2)
        scale = float(ref.abs().max())
        err = float((logits.double().cpu() - ref).abs().max())
        print(f"head1x1 bn={bn} ncls={ncls} {dtn}: err {err:.3e} scale {scale:.3f}")
        assert err < 1e-6 * scale + 1e-6, (bn, err, scale)


def test_wide_head_rejects_more_than_64_classes():
    from semantic_segmentation_amd import _lib, ops
    x = torch.zeros(1, 16, 16, 64, dtype=torch.float16, device=dev())
    logits = torch.zeros(1, 65, 16, 16, device=dev())
    with pytest.raises(ValueError):
        ops.head1x1_fwd_split(x, x, torch.zeros(65, 64, device=dev()), torch.zeros(65, device=dev()), logits)
    rc = _lib.load().gs_head1x1_fwd_split(x.data_ptr(), x.data_ptr(), torch.zeros(65, 64, device=dev()).data_ptr(), None, logits.data_ptr(),
                                          1, 16, 16, 64, 65, ops.dt_code(x), None)
    assert rc == -1                                              # GS_EINVAL: nothing launched
