"""Exact-integer kernel tests: the 16-bit convolution, data-gradient, weight-gradient and reduction kernels and the
BatchNorm / activation family (section G: forward apply, backward reduce / coefficients / apply, the head-source entry points) on
integer operands against the fp64 references of tests/exact_reference.py, at ZERO tolerance.  Called through
semantic_segmentation_amd.ops the way tests/test_gpu_kernels.py calls each kernel (channel-sliced inputs with poison outside
the slice, output slices whose neighbours must stay untouched, NaN-filled outputs and workspaces where a kernel promises to
overwrite), in fp16 and bf16.  Every comparison is assert_exact / torch.equal; the one allowance is the documented unit in
the last place on NEGATIVE LeakyReLU(0.2) outputs (exact_reference.leaky_ok) of the convolution epilogues.  Section G draws its
LeakyReLU operands as multiples of 5, where the slope product is exact, and has three allowances of its own, each stated where
it is made: c1 / c2 = float32(s / count) may be the adjacent fp32 value where count is no power of two (_bn_chain); tanh outputs
may be the 16-bit neighbour of the correctly rounded fp64 value, on at most TANH_NEIGHBOUR_SHARE of the elements
(test_bn_act_tanh_per_element); gs_bn_finalize / gs_bn_eval_coeffs, which take 1 / sqrt, are bounded by their count of fp32
roundings, 2^-24 each of the magnitude of the terms (test_bn_finalize_against_fp64, test_bn_eval_coeffs_against_fp64).
No case is skipped or filtered at run time.  GPU only (`-m gpu`).
Outputs and workspaces created through guarded() (out_buffer, nan32, zeros32) sit between guard words that are checked when the
test ends; tensors allocated otherwise (weight packs, inputs) are not covered by that check."""
import collections

import pytest
import torch
import torch.nn.functional as F

from tests import exact_reference as E
from tests.exact_reference import DTS, assert_exact, channels_last, expect16, expect32

pytestmark = pytest.mark.gpu

POISON = 7.0          # outside an input slice: an integer, so a read of it is a wrong integer and not a NaN that 0 * x hides
SENTINEL = 3.0        # around an output slice: must still be there afterwards
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def sliced(t_cl: torch.Tensor, dt, stride=None, coff=0, fill=POISON) -> torch.Tensor:
    """channels-last CPU tensor -> device buffer [..., stride] of dtype dt holding it at channel coff, `fill` elsewhere"""
    C = t_cl.shape[-1]
    stride = C if stride is None else stride
    buf = torch.full(tuple(t_cl.shape[:-1]) + (stride,), fill, dtype=dt, device=dev())
    buf[..., coff:coff + C] = t_cl.to(dt).to(dev())
    return buf


GUARD = 8192         # elements in front of and behind every output / workspace of a launch
GUARD_VALUE = -512.0
_GUARDED = []


def guarded(shape, dtype, fill) -> torch.Tensor:
    """A tensor of `shape` filled with `fill`, inside a larger allocation whose GUARD elements on either side must still hold
    GUARD_VALUE when the test ends (check_guards): a kernel that writes past its output or workspace fails the test that
    launched it, not a later one."""
    n = 1
    for v in shape:
        n *= int(v)
    flat = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=dtype, device=dev())
    body = flat[GUARD:GUARD + n]
    body.fill_(fill)
    _GUARDED.append((flat, n))
    return body.view(*[int(v) for v in shape])


@pytest.fixture(autouse=True)
def check_guards():
    _GUARDED.clear()
    yield
    torch.cuda.synchronize()
    for flat, n in _GUARDED:
        ok = bool((flat[:GUARD] == GUARD_VALUE).all()) and bool((flat[GUARD + n:] == GUARD_VALUE).all())
        assert ok, f"a launch wrote outside a buffer of {n} {flat.dtype} elements (guard words overwritten)"
    _GUARDED.clear()


@pytest.fixture(scope="module", autouse=True)
def leave_the_process_as_found():
    """these tests share a process with the rest of the suite: hand back the cached references and the allocator's blocks
    (several GB after the multi-item shapes) and make sure the process-wide knobs are at their defaults"""
    yield
    from semantic_segmentation_amd import ops
    _CACHE.clear()
    _GUARDED.clear()
    ops.conv3x3_set_kernel_form(-1)
    ops.set_persistent_grid(0)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def out_buffer(shape_cl, dt, stride=None, coff=0) -> torch.Tensor:
    """NaN where the kernel must write, the sentinel in the neighbouring channels, guard words around the allocation"""
    C = shape_cl[-1]
    stride = C if stride is None else stride
    buf = guarded(tuple(shape_cl[:-1]) + (stride,), dt, SENTINEL)
    buf[..., coff:coff + C] = NAN
    return buf


def assert_slice(buf, coff, want_cl, what):
    """the slice equals want; every other channel still holds the sentinel"""
    C = want_cl.shape[-1]
    assert_exact(buf[..., coff:coff + C], want_cl, what)
    other = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    other[coff:coff + C] = False
    assert bool((buf[..., other] == SENTINEL).all()), f"{what}: channels outside the output slice were written"


def nan32(*shape):
    return guarded(shape, torch.float32, NAN)


def zeros32(*shape):
    return guarded(shape, torch.float32, 0.0)


_CACHE = collections.OrderedDict()


def cached(fn, *key):
    """references are the same integers for both dtypes and every kernel form: keep the last few cases"""
    k = (fn.__name__,) + key
    if k not in _CACHE:
        _CACHE[k] = fn(*key)
        while len(_CACHE) > 4:
            _CACHE.popitem(last=False)
    return _CACHE[k]


def _id(v):
    return "x".join(_id(i) for i in v) if isinstance(v, tuple) else str(v)


def stat_sums(part, rows, C):
    return part[: rows * 2 * C].view(rows, 2, C).double().sum(0).cpu()


# ================================================================================================ A: 2-D 3x3 halo kernels
def _conv3x3_prepare(ops, c, shape, dt):
    """device operands and expected values of one (case, value set, dtype): shared by every kernel form"""
    N, H, W, Cin, Cout = shape
    wf = torch.empty(9, Cout, Cin, dtype=dt, device=dev())
    wd = torch.empty(9, Cin, Cout, dtype=dt, device=dev())
    ops.pack_weight(c["w"].to(dev()), wf, wd, False)
    assert_exact(wf.float().cpu(), c["w"].permute(2, 3, 0, 1).reshape(9, Cout, Cin).contiguous(), "pack_weight [tap][co][ci]")
    assert_exact(wd.float().cpu(), c["w"].permute(2, 3, 1, 0).reshape(9, Cin, Cout).contiguous(), "pack_weight [tap][ci][co]")
    x_cl = channels_last(c["x"])
    y_cl = channels_last(c["y"]).to(dev())
    b = c["b"].to(dev())
    return {"wf": wf, "wd": wd, "b": b, "xin": sliced(x_cl, dt, Cin + 16, 16), "x": sliced(x_cl, dt),
            "dy": sliced(channels_last(c["dy"]), dt), "want_y": expect16(y_cl, dt), "want_y2": expect16(F.relu(y_cl.double() + b.double()), dt),
            "want_dx": expect16(channels_last(c["dx"]).to(dev()), dt),
            "sums": torch.stack([c["s1"], c["s2"]]) if "s1" in c else None}


def _forms(W, K, Cn):
    """forms worth pinning for a launch with K input and Cn output channels: without the LDS-DMA kernel every form is form 0"""
    return E.ALL_FORMS if E.conv3x3_dma_shape(W, K, Cn) else (-1, 0)


def _conv3x3_forward(ops, p, shape, dt, form, what):
    """forward + partials into a strided slice from a channel-sliced input, and bias + ReLU -- one kernel form"""
    from semantic_segmentation_amd._lib import ACT_RELU
    N, H, W, Cin, Cout = shape
    y = out_buffer((N, H, W, Cout), dt, Cout + 8, 8)
    y2 = out_buffer((N, H, W, Cout), dt, 2 * Cout, Cout)
    part = nan32(ops.bn_partials_numel(ops.conv3x3_mtiles(N, H, W, Cout), Cout))
    ops.conv3x3_set_kernel_form(form)
    try:
        rows = ops.conv3x3_stat_rows(N, H, W, Cin, Cout)
        ops.conv3x3(p["xin"], p["wf"], y, N, H, W, Cin, Cout, ops.TAPS3_FWD, None, part, in_stride=Cin + 16, in_coff=16,
                    out_stride=Cout + 8, out_coff=8)
        ops.conv3x3(p["x"], p["wf"], y2, N, H, W, Cin, Cout, ops.TAPS3_FWD, p["b"], None, act=ACT_RELU, out_stride=2 * Cout, out_coff=Cout)
        torch.cuda.synchronize()
    finally:
        ops.conv3x3_set_kernel_form(-1)
    assert_slice(y, 8, p["want_y"], what + " y")
    if p["sums"] is not None:
        assert_exact(stat_sums(part, rows, Cout), p["sums"], what + f" partial sums ({rows} rows)")
    assert_slice(y2, Cout, p["want_y2"], what + " bias+relu")


def _conv3x3_dgrad(ops, p, shape, dt, form, what):
    """the data gradient (flipped taps, the [9][Cin][Cout] pack: K = Cout) -- one kernel form"""
    N, H, W, Cin, Cout = shape
    dx = out_buffer((N, H, W, Cin), dt)
    ops.conv3x3_set_kernel_form(form)
    try:
        ops.conv3x3(p["dy"], p["wd"], dx, N, H, W, Cout, Cin, ops.TAPS3_DGRAD)
        torch.cuda.synchronize()
    finally:
        ops.conv3x3_set_kernel_form(-1)
    assert_exact(dx, p["want_dx"], what + " dgrad")


def _conv3x3_launches(ops, p, shape, dt, what, forms_fwd=None, forms_dgrad=None):
    """every form that applies, decided per launch direction (the data gradient swaps the channel roles)"""
    N, H, W, Cin, Cout = shape
    for form in (_forms(W, Cin, Cout) if forms_fwd is None else forms_fwd):
        _conv3x3_forward(ops, p, shape, dt, form, f"{what} form {form}")
    for form in (_forms(W, Cout, Cin) if forms_dgrad is None else forms_dgrad):
        _conv3x3_dgrad(ops, p, shape, dt, form, f"{what} form {form}")


def _conv3x3_wgrad_launches(ops, c, shape, dt, what):
    N, H, W, Cin, Cout = shape
    xb = sliced(channels_last(c["x"]), dt, Cin + 8, 8)
    db = sliced(channels_last(c["dy"]), dt, Cout + 16, 0)
    dwp = zeros32(9, Cout, Cin)
    ops.conv3x3_wgrad(xb, db, dwp, N, H, W, Cin, Cout, in_stride=Cin + 8, in_coff=8, out_stride=Cout + 16, out_coff=0)
    assert_exact(dwp, expect32(c["dw"].permute(2, 3, 0, 1).reshape(9, Cout, Cin).contiguous()), what + " wgrad (atomic) [tap][co][ci]")
    outs = []
    for _ in range(2):
        ws = nan32(ops.conv3x3_wgrad_ws_floats(N, H, W, Cin, Cout))
        g = nan32(Cout, Cin, 3, 3)
        ops.conv3x3_wgrad_det(xb, db, ws, g, N, H, W, Cin, Cout, 0.25, in_stride=Cin + 8, in_coff=8, out_stride=Cout + 16, out_coff=0)
        outs.append(g)
    assert_exact(outs[0], expect32(c["dw"], 0.25), what + " wgrad (deterministic) [co][ci][ky][kx]")
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("shape,wgrad", E.CONV3X3_CASES, ids=[_id(s) for s, _ in E.CONV3X3_CASES])
def test_conv3x3_exact(shape, wgrad, dtn, dt):
    """gs_conv3x3 (every kernel form), gs_conv3x3_wgrad, gs_conv3x3_wgrad_slabs + gs_wgrad_reduce_unpack: y, y + bias -> ReLU,
    dx, dw equal the integer reference under the dense sets S and P; y, dx, the BatchNorm partial sums and dw under T(d) --
    the only set under which the weight gradient of the multi-item shapes (up to 294 912 pixels) is exact."""
    from semantic_segmentation_amd import ops
    for vset, d in E.conv3x3_sets(shape, wgrad):
        c = cached(E.conv3x3_build, shape, wgrad, vset, d)
        p = _conv3x3_prepare(ops, c, shape, dt)
        _conv3x3_launches(ops, p, shape, dt, f"conv3x3 {_id(shape)} {vset} {dtn}")
        if E.conv3x3_wgrad_runs(wgrad, vset):
            _conv3x3_wgrad_launches(ops, c, shape, dt, f"conv3x3 {_id(shape)} {vset} {dtn}")


@pytest.mark.parametrize("dtn,dt", DTS)
def test_conv3x3_exact_small_persistent_grids(dtn, dt):
    """A block that walks many work items with a short last round, on a small tensor: gs_set_persistent_grid accepts 0 or
    8..1024 (include/gsseg.h), so 1, 2 and 3 are refused (error, setting unchanged) and the test runs at the documented lower
    limit 8 and at 9 and 11 blocks (54 / 90 items of the 8- / 4-wave form); the statistics rows are re-queried after each change."""
    from semantic_segmentation_amd import ops
    shape = E.GRID_SHAPE
    N, H, W, Cin, Cout = shape
    before = ops.get_persistent_grid()
    for blocks in E.GRID_BLOCKS_REFUSED:
        with pytest.raises(RuntimeError):
            ops.set_persistent_grid(blocks)
        assert ops.get_persistent_grid() == before
    try:
        for blocks in E.GRID_BLOCKS:
            ops.set_persistent_grid(blocks)
            assert ops.get_persistent_grid() == blocks
            for form in (8, 4, 44, 0):
                ops.conv3x3_set_kernel_form(form)
                try:
                    rows = ops.conv3x3_stat_rows(N, H, W, Cin, Cout)
                finally:
                    ops.conv3x3_set_kernel_form(-1)
                if form != 0:
                    assert rows * ((Cout + 63) // 64) <= blocks, (rows, blocks)      # one row per block and cout-tile group
                for vset, d in E.conv3x3_sets(shape, False):
                    p = _conv3x3_prepare(ops, cached(E.conv3x3_build, shape, False, vset, d), shape, dt)
                    _conv3x3_launches(ops, p, shape, dt, f"conv3x3 {_id(shape)} {vset} {dtn} grid {blocks}", (form,), (form,))
    finally:
        ops.set_persistent_grid(0)
    assert ops.get_persistent_grid() == before


# ================================================================================================ G: negative control
@pytest.mark.parametrize("dtn,dt", DTS)
def test_comparer_sees_one_misplaced_tap_on_the_gpu(dtn, dt):
    """An ordinary, legal launch of gs_conv3x3 with a tap table in which tap 0 reads (0, 0) instead of (-1, -1): the result
    equals the convolution whose centre weight is w[1][1] + w[0][0] and whose corner weight is 0 -- exactly -- and the
    comparer finds it different from the true convolution, whatever the norm-wise error is."""
    from semantic_segmentation_amd import ops
    from tests.test_gpu_kernels import rel_err, tol
    shape = (2, 37, 41, 64, 64)
    N, H, W, Cin, Cout = shape
    c = cached(E.conv3x3_build, shape, True, "S", None)
    taps = list(ops.TAPS3_FWD)
    taps[0] = (0, 0)
    wf = torch.empty(9, Cout, Cin, dtype=dt, device=dev())
    ops.pack_weight(c["w"].to(dev()), wf, None, False)
    y = out_buffer((N, H, W, Cout), dt)
    ops.conv3x3(sliced(channels_last(c["x"]), dt), wf, y, N, H, W, Cin, Cout, taps)
    torch.cuda.synchronize()
    w2 = c["w"].clone()
    w2[:, :, 1, 1] += w2[:, :, 0, 0]
    w2[:, :, 0, 0] = 0
    E.require_products(9 * Cin, c["x"], w2, "moved tap")
    moved, _ = E.autograd(lambda x, w: F.conv2d(x, w, None, padding=1), (c["x"], w2))
    assert_exact(y, expect16(channels_last(moved), dt), f"conv3x3 with tap 0 at (0, 0) {dtn}")
    true = expect16(channels_last(c["y"]), dt)
    n = E.mismatches(y, true).shape[0]
    err = rel_err(y.float(), true.float())
    assert n > 0, f"the comparer missed a misplaced tap (rel_err {err:.3e}, limit of the norm-wise tests {tol(dt):.1e})"
    print(f"misplaced tap {dtn}: {n} of {y.numel()} elements differ, rel_err {err:.3e} (norm-wise limit {tol(dt):.1e})")


# ================================================================================================ B: generic implicit GEMM
ACTS = {"none": 0, "relu": 1, "leaky": 2}


def _poison_splitk(ops):
    """the split-K workspaces need no initialisation between launches (test_igemm_split_k_skinny): fill them with NaN, so that a
    part a launch fails to write cannot be served by the stale, correct partial of the launch before it"""
    torch.cuda.synchronize()
    for ws in ops._SPLITK_WS.values():
        ws.fill_(NAN)


def _check_activated(buf, coff, ref, b, act, dt, what):
    """y = act(ref + b) in a slice of buf: exact for no activation / ReLU, the one-ulp rule on negative LeakyReLU outputs"""
    pre = channels_last(ref.double() + b.double().view(1, -1, *([1] * (ref.dim() - 2))))
    C = pre.shape[-1]
    if act == "leaky":
        E.assert_leaky_exact(buf[..., coff:coff + C], pre, what)
        other = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
        other[coff:coff + C] = False
        assert bool((buf[..., other] == SENTINEL).all()), f"{what}: channels outside the output slice were written"
    else:
        assert_slice(buf, coff, expect16(F.relu(pre) if act == "relu" else pre, dt), what)


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.IGEMM_FWD_CASES, ids=E.fwd_id)
def test_igemm_forward_exact(case, dtn, dt):
    """gs_conv_igemm forward (register-staged engine, split-K through the workspace, the weight-streaming form of
    csrc/skinny.hip): bias + activation + partials in one launch from / into channel slices, and the plain convolution with
    partials; the partial sums (of the accumulators, before bias) under T(d)."""
    from semantic_segmentation_amd import ops
    c = case
    N, IH, IW, Cin, Cout, k, s, p = (c[n] for n in ("N", "IH", "IW", "Cin", "Cout", "k", "s", "p"))
    OH, OW = E.out_size(IH, k, s, p), E.out_size(IW, k, s, p)
    for vset, d in E.igemm_fwd_sets(c, dtn):
        r = cached(E.igemm_fwd_build, tuple(c.items()), vset, d)
        what = f"igemm {E.fwd_id(c)} {vset} {dtn}"
        geom = ops.geom_conv(N, IH, IW, Cin, Cout, k, s, p, in_stride=Cin + c["in_extra"], in_coff=c["in_coff"],
                             out_stride=Cout + c["out_extra"], out_coff=c["out_coff"])
        wf = torch.empty(k * k, Cout, Cin, dtype=dt, device=dev())
        ops.pack_weight(r["w"].to(dev()), wf, None, False)
        xin = sliced(channels_last(r["x"]), dt, Cin + c["in_extra"], c["in_coff"])
        nt = ops.conv_igemm_mtiles(geom)
        want_sums = torch.stack([r["s1"], r["s2"]]) if vset == "T" else None
        y = out_buffer((N, OH, OW, Cout), dt, Cout + c["out_extra"], c["out_coff"])
        part = nan32(ops.bn_partials_numel(nt, Cout))
        _poison_splitk(ops)
        ops.conv_igemm(geom, xin, wf, y, r["b"].to(dev()), part, ACTS[c["act"]])
        torch.cuda.synchronize()
        _check_activated(y, c["out_coff"], r["y"], r["b"], c["act"], dt, what + " bias+act")
        if want_sums is not None:
            assert_exact(stat_sums(part, nt, Cout), want_sums, what + " partial sums (with bias + act)")
        y = out_buffer((N, OH, OW, Cout), dt, Cout + c["out_extra"], c["out_coff"])
        part = nan32(ops.bn_partials_numel(nt, Cout))
        _poison_splitk(ops)
        ops.conv_igemm(geom, xin, wf, y, None, part)
        torch.cuda.synchronize()
        assert_slice(y, c["out_coff"], expect16(channels_last(r["y"]), dt), what + " y")
        if want_sums is not None:
            assert_exact(stat_sums(part, nt, Cout), want_sums, what + " partial sums")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.IGEMM_GRAD_CASES, ids=_id)
def test_igemm_gradients_exact(case, dtn, dt):
    """data gradient on the generic engine (geom_conv_dgrad_s1; the four classes of geom_conv_s2_dgrad_class one by one and
    in one gs_conv_igemm_batch launch) and the MFMA weight gradient: atomic into zeros (+ gs_unpack_wgrad), assigned into NaN
    where gs_conv_wgrad_single_pass allows it (refused where not), deterministic slabs + gs_wgrad_reduce_unpack"""
    from semantic_segmentation_amd import ops
    N, h, w, Cin, Cout, k, s, p, single = case
    OH, OW = E.out_size(h, k, s, p), E.out_size(w, k, s, p)
    taps = k * k
    geom = ops.geom_conv(N, h, w, Cin, Cout, k, s, p)
    assert ops.conv_wgrad_single_pass(geom) == single
    for vset in ("S", "P"):
        r = cached(E.igemm_grad_build, case, vset)
        what = f"igemm {_id(case)} {vset} {dtn}"
        wd = torch.empty(taps, Cin, Cout, dtype=dt, device=dev())
        ops.pack_weight(r["w"].to(dev()), None, wd, False)
        assert_exact(wd.float().cpu(), r["w"].permute(2, 3, 1, 0).reshape(taps, Cin, Cout).contiguous(), what + " dgrad pack")
        xd, dyd = sliced(channels_last(r["x"]), dt), sliced(channels_last(r["dy"]), dt)
        want_dx = expect16(channels_last(r["dx"]), dt)
        if s == 1:
            dx = out_buffer((N, h, w, Cin), dt)
            ops.conv_igemm(ops.geom_conv_dgrad_s1(N, h, w, Cin, Cout, k, p), dyd, wd, dx)
            assert_exact(dx, want_dx, what + " dgrad s1")
        else:
            gds = [ops.geom_conv_s2_dgrad_class(N, h, w, Cin, Cout, k, p, cls >> 1, cls & 1) for cls in range(4)]
            dx = out_buffer((N, h, w, Cin), dt)
            for g in gds:
                ops.conv_igemm(g, dyd, wd, dx)
            assert_exact(dx, want_dx, what + " dgrad s2, four class launches")
            dx = out_buffer((N, h, w, Cin), dt)
            ops.conv_igemm_batch(gds, dyd, [wd] * 4, dx)
            assert_exact(dx, want_dx, what + " dgrad s2, batched")
        want_dw = r["dw"].permute(2, 3, 0, 1).reshape(taps, Cout, Cin).contiguous()
        dwp = zeros32(taps, Cout, Cin)
        ops.conv_wgrad(geom, xd, dyd, dwp)
        assert_exact(dwp, expect32(want_dw), what + " wgrad (atomic) [tap][co][ci]")
        dw = nan32(Cout, Cin, k, k)
        ops.unpack_wgrad(dwp, dw, Cout, Cin, taps, False, 0.5)
        assert_exact(dw, expect32(r["dw"], 0.5), what + " unpack_wgrad")
        dwa = nan32(taps, Cout, Cin)
        if single:
            ops.conv_wgrad(geom, xd, dyd, dwa, assign=True)
            assert_exact(dwa, expect32(want_dw), what + " wgrad (assigned into NaN)")
        else:
            with pytest.raises(RuntimeError):
                ops.conv_wgrad(geom, xd, dyd, dwa, assign=True)
            assert bool(torch.isnan(dwa).all()), what + ": a refused assign launch wrote"
        outs = []
        for _ in range(2):
            ws = nan32(max(ops.conv_wgrad_ws_floats(geom), 1))
            g_ = nan32(Cout, Cin, k, k)
            ops.conv_wgrad_det(geom, xd, dyd, ws, g_, Cout, Cin, taps, 0.25)
            outs.append(g_)
        assert_exact(outs[0], expect32(r["dw"], 0.25), what + " wgrad (deterministic)")
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.CONVT_CASES, ids=_id)
def test_convT_classes_exact(case, dtn, dt):
    """ConvTranspose2d(k, s2, pad) through its four sub-pixel classes (geom_convT_class on the full [k*k][Cout][Cin] pack):
    four gs_conv_igemm launches and one gs_conv_igemm_batch, with bias and per-class partials; and the batched deterministic
    weight gradient of the four classes (gs_conv_wgrad_slabs_batch + gs_wgrad_reduce_unpack) in its [class][tap][Cout][Cin] layout"""
    from semantic_segmentation_amd import ops
    N, h, Cin, Cout, k, pad = case
    geoms = [ops.geom_convT_class(N, h, h, Cin, Cout, k, pad, cls >> 1, cls & 1) for cls in range(4)]
    slots = [[g.tap_w[t] for t in range(g.ntaps)] for g in geoms]              # ky * k + kx of each class tap
    mt = ops.conv_igemm_mtiles(geoms[0])
    rowf = mt * 2 * Cout
    for vset, d in E.convt_sets(case, dtn):
        r = cached(E.convt_build, case, vset, d)
        what = f"convT {_id(case)} {vset} {dtn}"
        wf = torch.empty(k * k, Cout, Cin, dtype=dt, device=dev())
        ops.pack_weight(r["w"].to(dev()), wf, None, True)
        xd = sliced(channels_last(r["x"]), dt)
        want = expect16(channels_last(r["y"].double() + r["b"].double().view(1, -1, 1, 1)), dt)
        y1 = out_buffer((N, 2 * h, 2 * h, Cout), dt)
        p1 = nan32(ops.bn_partials_numel(4 * mt, Cout))
        _poison_splitk(ops)
        for cls in range(4):
            ops.conv_igemm(geoms[cls], xd, wf, y1, r["b"].to(dev()), p1[cls * rowf:])
        _poison_splitk(ops)
        y2 = out_buffer((N, 2 * h, 2 * h, Cout), dt)
        p2 = nan32(ops.bn_partials_numel(4 * mt, Cout))
        ops.conv_igemm_batch(geoms, xd, [wf] * 4, y2, r["b"].to(dev()), [p2[cls * rowf:] for cls in range(4)])
        torch.cuda.synchronize()
        assert_exact(y1, want, what + " four class launches")
        assert_exact(y2, want, what + " batched")
        if vset == "T":
            for cls in range(4):
                ws_ = torch.stack(list(r["cls_sums"][cls]))
                assert_exact(stat_sums(p1[cls * rowf:], mt, Cout), ws_, what + f" partial sums class {cls}")
                assert_exact(stat_sums(p2[cls * rowf:], mt, Cout), ws_, what + f" partial sums class {cls} (batched)")
        # weight gradient: x = the layer input, dy = d(output); identity slots -> dwm[class][t] = dW[:, :, ky, kx]^T
        gi = [ops.geom_convT_class(N, h, h, Cin, Cout, k, pad, cls >> 1, cls & 1) for cls in range(4)]
        for g in gi:
            for t in range(g.ntaps):
                g.tap_w[t] = t
        nt_ = gi[0].ntaps
        want_dwm = torch.stack([torch.stack([r["dw"][:, :, sl // k, sl % k].t() for sl in slots[cls]]) for cls in range(4)])
        parts = ops.conv_wgrad_parts(gi[0])
        dud = sliced(channels_last(r["dy"]), dt)
        outs = []
        for _ in range(2):
            ws = nan32(max(parts * 4 * nt_ * Cout * Cin, 1)) if parts > 1 else None
            dwm = nan32(4, nt_, Cout, Cin)
            assert ops.conv_wgrad_det_batch(gi, xd, dud, ws, dwm, 0.5) == parts
            outs.append(dwm)
        assert_exact(outs[0], expect32(want_dwm.contiguous(), 0.5), what + " batched wgrad [class][tap][co][ci]")
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("A,B,T,parts,transposed", [(128, 128, 9, 4, 0), (256, 128, 9, 32, 0), (160, 130, 9, 3, 0), (128, 128, 16, 5, 0),
                                                    (128, 256, 4, 2, 1), (512, 512, 9, 1, 0), (128, 128, 9, 40, 0), (64, 64, 9, 7, 0),
                                                    (64, 64, 27, 130, 0)])
def test_wgrad_reduce_unpack_exact(A, B, T, parts, transposed):
    """gs_wgrad_reduce_unpack on integer slabs (|v| <= 1000, up to 130 parts: every sum below 2^24): the ordered sum times a
    power-of-two scale, in both output layouts, into a NaN-filled gradient"""
    from semantic_segmentation_amd import _lib
    from semantic_segmentation_amd.ops import _p, _stream
    g = E.generator(("reduce", A, B, T, parts, transposed))
    ws = torch.randint(-1000, 1001, (parts, T, A, B), generator=g).float()
    assert parts * 1000 < E.LIMIT
    tot = ws.double().sum(0)
    want = tot.permute(2, 1, 0) if transposed else tot.permute(1, 2, 0)           # [B][A][T] / [A][B][T]
    grad = nan32(*want.shape)
    _lib.call("gs_wgrad_reduce_unpack", _p(ws.to(dev())), parts, _p(grad), A, B, T, transposed, 0.5, _stream())
    torch.cuda.synchronize()
    assert_exact(grad, expect32(want.contiguous(), 0.5), f"reduce_unpack {A}x{B}x{T} parts {parts} transposed {transposed}")


# ================================================================================================ C: ConvTranspose 2x2 / s2
def _pad_off(pad):
    return pad[0] // 2, pad[1] // 2


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.UPCONV_FWD_CASES, ids=_id)
def test_upconv2x2_fwd_exact(case, dtn, dt):
    """gs_upconv2x2_fwd (merged pointwise GEMM and the LDS-DMA GEMM of csrc/pwgemm.hip) + bias into the up half of a concat
    buffer at the F.pad offset, from a channel slice: inside equals the reference, pixels no input owns stay 0, the skip half
    keeps its sentinel"""
    from semantic_segmentation_amd import ops
    N, h, w, Cin, Cout, pad = case
    H2, W2 = 2 * h + pad[0], 2 * w + pad[1]
    pt, pl = _pad_off(pad)
    for vset in ("S", "P"):
        r = cached(E.upconv_build, case, vset, "")
        what = f"upconv2x2 fwd {_id(case)} {vset} {dtn}"
        wf = torch.empty(4, Cout, Cin, dtype=dt, device=dev())
        ops.pack_weight(r["w"].to(dev()), wf, None, True)
        assert_exact(wf.float().cpu(), r["w"].permute(2, 3, 1, 0).reshape(4, Cout, Cin).contiguous(), what + " pack")
        xin = sliced(channels_last(r["x"]), dt, Cin + 24, 8)
        cat = guarded((N, H2, W2, 2 * Cout), dt, 0.0)
        cat[..., :Cout] = SENTINEL
        cat[:, pt:pt + 2 * h, pl:pl + 2 * w, Cout:] = NAN
        for _ in range(2):
            ops.upconv2x2_fwd(xin, wf, r["b"].to(dev()), cat, N, 1, h, w, Cin, Cout, 1, H2, W2, in_stride=Cin + 24, in_coff=8,
                              out_stride=2 * Cout, out_coff=Cout, ooy=pt, oox=pl)
        torch.cuda.synchronize()
        want = torch.where(r["inner"], r["y"].double() + r["b"].double().view(1, -1, 1, 1), torch.zeros((), dtype=torch.float64))
        assert_slice(cat, Cout, expect16(channels_last(want), dt), what)


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.UPCONV_DGRAD_CASES, ids=_id)
def test_upconv2x2_dgrad_exact(case, dtn, dt):
    """gs_upconv2x2_dgrad on the shapes it covers, GS_EUNSUPPORTED (output untouched) and the generic engine on the others"""
    from semantic_segmentation_amd import _lib, ops
    from semantic_segmentation_amd.ops import _p, _stream, dt_code
    N, h, w, Cin, Cout, pad = case
    H2, W2 = 2 * h + pad[0], 2 * w + pad[1]
    pt, pl = _pad_off(pad)
    fast = E.upconv_dma_fwd_shape(N, h, w, Cin, Cout)
    for vset in ("S", "P"):
        r = cached(E.upconv_build, case, vset, "x")
        what = f"upconv2x2 dgrad {_id(case)} {vset} {dtn}"
        wd = torch.empty(4, Cin, Cout, dtype=dt, device=dev())
        ops.pack_weight(r["w"].to(dev()), None, wd, True)
        dcat = sliced(channels_last(r["dy"]), dt, 2 * Cout, Cout, fill=SENTINEL)        # the skip half must not be read
        want = expect16(channels_last(r["dx"]), dt)
        dz = out_buffer((N, h, w, Cin), dt)
        rc = _lib.load().gs_upconv2x2_dgrad(_p(dcat), _p(wd), _p(dz), N, h, w, Cin, Cout, H2, W2, 2 * Cout, Cout, pt, pl, Cin, 0,
                                            dt_code(dcat), _stream())
        torch.cuda.synchronize()
        assert rc == (0 if fast else _lib.GS_EUNSUPPORTED), (rc, fast)
        if fast:
            assert_exact(dz, want, what + " (LDS-DMA GEMM)")
        else:
            assert bool(torch.isnan(dz).all()), what + ": a declined launch wrote"
        taps = [(py + pt, px + pl) for py in range(2) for px in range(2)]
        geom = ops.make_geom(N, H2, W2, Cout, h, w, Cin, h, w, taps, isy=2, isx=2, in_stride=2 * Cout, in_coff=Cout)
        dz = out_buffer((N, h, w, Cin), dt)
        ops.upconv2x2_dgrad(geom, dcat, wd, dz, N, h, w, Cin, Cout, H2, W2, 2 * Cout, Cout, pt, pl)
        assert_exact(dz, want, what + " (ops.upconv2x2_dgrad)")
        dz = out_buffer((N, h, w, Cin), dt)
        ops.conv_igemm(geom, dcat, wd, dz)
        assert_exact(dz, want, what + " (generic engine)")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.UPCONV_WGRAD_CASES, ids=_id)
def test_upconv2x2_wgrad_exact(case, dtn, dt):
    """ops.upconv2x2_wgrad_det: the K = pixels LDS-DMA GEMM (csrc/upwgrad.hip) where upconv2x2_wgrad_ws_floats > 0, else the
    generic deterministic weight gradient; the layer input optionally the hi plane of a pair buffer"""
    from semantic_segmentation_amd import ops
    N, h, w, Cin, Cout, pad, pair = case
    H2, W2 = 2 * h + pad[0], 2 * w + pad[1]
    pt, pl = _pad_off(pad)
    fast = ops.upconv2x2_wgrad_ws_floats(N, h, w, Cin, Cout) > 0
    assert fast == E.upconv_dma_wgrad_shape(N, h, w, Cin, Cout)
    xs = 2 * Cin if pair else Cin
    taps = [(py + pt, px + pl) for py in range(2) for px in range(2)]
    geom = ops.make_geom(N, H2, W2, Cout, h, w, Cin, h, w, taps, isy=2, isx=2, in_stride=2 * Cout, in_coff=Cout, out_stride=xs)
    need = max(ops.conv_wgrad_ws_floats(geom), ops.upconv2x2_wgrad_ws_floats(N, h, w, Cin, Cout), 1)
    for vset in ("S", "P"):
        r = cached(E.upconv_build, case, vset, "w")
        what = f"upconv2x2 wgrad {_id(case)} {vset} {dtn}"
        dcat = sliced(channels_last(r["dy"]), dt, 2 * Cout, Cout, fill=SENTINEL)
        xin = sliced(channels_last(r["x"]), dt, xs, 0, fill=5.0)                          # pair: the lo plane must not be read
        res = []
        for _ in range(2):
            ws = nan32(need)
            dw = nan32(Cin, Cout, 2, 2)
            ops.upconv2x2_wgrad_det(geom, xin, dcat, ws, dw, N, h, w, Cin, Cout, H2, W2, xs, 2 * Cout, Cout, pt, pl, 0.5)
            res.append(dw)
        assert_exact(res[0], expect32(r["dw"], 0.5), what + (" (LDS-DMA GEMM)" if fast else " (generic engine)"))
        assert torch.equal(res[0], res[1])


# ================================================================================================ D: 3-D
def _slices(t):                         # [NB, C, D, H, W] -> [NB*D, H, W, C]
    cl = channels_last(t)
    return cl.reshape(cl.shape[0] * cl.shape[1], *cl.shape[2:])


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.CONV3D_CASES, ids=_id)
def test_conv3d3_exact(case, dtn, dt):
    """gs_conv3d_3x3x3 forward + partials and data gradient, gs_conv3d_3x3x3_wgrad (atomic, + gs_unpack_wgrad) and the
    deterministic slabs form: with dense values a depth tap that leaks across volumes or past D is a certain mismatch"""
    from semantic_segmentation_amd import ops
    NB, D, H, W, Cin, Cout = case
    for vset, d in E.conv3d_sets(case):
        r = cached(E.conv3d_build, case, vset, d)
        what = f"conv3d {_id(case)} {vset} {dtn}"
        wf = torch.empty(27, Cout, Cin, dtype=dt, device=dev())
        wd = torch.empty(27, Cin, Cout, dtype=dt, device=dev())
        ops.pack_weight(r["w"].reshape(Cout, Cin, 27, 1).to(dev()), wf, wd, False)
        xs, dys = sliced(_slices(r["x"]), dt), sliced(_slices(r["dy"]), dt)
        part = nan32(ops.bn_partials_numel(ops.conv3d3_mtiles(NB, D, H, W, Cout), Cout))
        rows = ops.conv3d3_stat_rows(NB, D, H, W, Cin, Cout)
        yo = out_buffer((NB * D, H, W, Cout), dt)
        ops.conv3d3(xs, wf, yo, NB, D, H, W, Cin, Cout, bn_partials=part)
        dxo = out_buffer((NB * D, H, W, Cin), dt)
        ops.conv3d3(dys, wd, dxo, NB, D, H, W, Cout, Cin, dgrad=True)
        torch.cuda.synchronize()
        assert_exact(yo, expect16(_slices(r["y"]), dt), what + " y [nb*D+d][y][x][c]")
        if vset == "T":
            assert_exact(stat_sums(part, rows, Cout), torch.stack([r["s1"], r["s2"]]), what + f" partial sums ({rows} rows)")
        assert_exact(dxo, expect16(_slices(r["dx"]), dt), what + " dgrad")
        if vset == "T":
            continue
        want_dw = r["dw"].reshape(Cout, Cin, 27)
        dwp = zeros32(27, Cout, Cin)
        ops.conv3d3_wgrad(xs, dys, dwp, NB, D, H, W, Cin, Cout)
        assert_exact(dwp, expect32(want_dw.permute(2, 0, 1).contiguous()), what + " wgrad (atomic) [tap][co][ci]")
        dw = nan32(Cout, Cin, 27)
        ops.unpack_wgrad(dwp, dw, Cout, Cin, 27, False, 1.0)
        assert_exact(dw, expect32(want_dw), what + " unpack_wgrad")
        outs = []
        for _ in range(2):
            ws = nan32(ops.conv3d3_wgrad_ws_floats(NB, D, H, W, Cin, Cout))
            g_ = nan32(Cout, Cin, 27)
            ops.conv3d3_wgrad_det(xs, dys, ws, g_, NB, D, H, W, Cin, Cout, 0.5)
            outs.append(g_)
        assert_exact(outs[0], expect32(want_dw, 0.5), what + " wgrad (deterministic)")
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.UPCONV3D_CASES, ids=_id)
def test_upconv2x2x2_fwd_exact(case, dtn, dt):
    """ConvTranspose3d(k2, s2) + bias: eight sub-voxel classes in one GEMM (merged kernel / LDS-DMA GEMM), from a channel slice
    into a channel slice of a wider buffer"""
    from semantic_segmentation_amd import ops
    N, D, h, w, Cin, Cout = case
    for vset in ("S", "P"):
        r = cached(E.upconv3d_build, case, vset)
        wf = r["w"].permute(2, 3, 4, 1, 0).reshape(8, Cout, Cin).contiguous().to(dt).to(dev())      # slot (kz*2+ky)*2+kx
        xin = sliced(_slices(r["x"]), dt, Cin + 64, 64)
        y = out_buffer((N * 2 * D, 2 * h, 2 * w, Cout), dt, Cout + 64, 0)
        ops.upconv2x2_fwd(xin, wf, r["b"].to(dev()), y, N, D, h, w, Cin, Cout, 2 * D, 2 * h, 2 * w, in_stride=Cin + 64, in_coff=64,
                          out_stride=Cout + 64, out_coff=0)
        torch.cuda.synchronize()
        want = r["y"].double() + r["b"].double().view(1, -1, 1, 1, 1)
        assert_slice(y, 0, expect16(_slices(want), dt), f"upconv2x2x2 {_id(case)} {vset} {dtn}")


# ================================================================================================ E: ends of the nets, reductions
@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.SMALLCIN_CASES, ids=_id)
def test_smallcin_exact(case, dtn, dt):
    """gs_conv_smallcin_fwd (+ bias, or + tile partials) / _wgrad / _dgrad on fp32 integer images and weights: a ragged tile,
    several tiles with a ragged last one; the fp32 gradients equal the reference times the power-of-two gscale"""
    from semantic_segmentation_amd import ops
    Cin, k, s, p, bias, H, W = case
    N, Cout = 2, 64
    OH, OW = E.out_size(H, k, s, p), E.out_size(W, k, s, p)
    for vset, d in E.smallcin_sets(case):
        r = cached(E.smallcin_build, case, vset, d)
        what = f"smallcin {_id(case)} {vset} {dtn}"
        xd, wd_ = r["x"].to(dev()), r["w"].to(dev())
        y = out_buffer((N, OH, OW, Cout), dt)
        mt = ops.conv_smallcin_mtiles(N, OH, OW)
        part = None if bias else nan32(ops.bn_partials_numel(mt, Cout))
        ops.conv_smallcin_fwd(xd, wd_, r["b"].to(dev()) if bias else None, y, part, k, s, p)
        torch.cuda.synchronize()
        want = r["y"].double() + (r["b"].double().view(1, -1, 1, 1) if bias else 0.0)
        assert_exact(y, expect16(channels_last(want), dt), what + " y")
        if part is not None and vset == "T":
            assert_exact(stat_sums(part, mt, Cout), torch.stack([r["s1"], r["s2"]]), what + " partial sums")
        dyd = sliced(channels_last(r["dy"]), dt)
        dw = zeros32(Cout, Cin, k, k)
        ops.conv_smallcin_wgrad(xd, dyd, dw, k, s, p, 0.5)
        dx = nan32(N, Cin, H, W)
        ops.conv_smallcin_dgrad(dyd, wd_, dx, k, s, p, 0.5)
        torch.cuda.synchronize()
        assert_exact(dw, expect32(r["dw"], 0.5), what + " wgrad [co][ci][ky][kx]")
        assert_exact(dx, expect32(r["dx"], 0.5), what + " dgrad [n][ci][y][x]")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.SMALLCOUT_CASES, ids=_id)
def test_smallcout_exact(case, dtn, dt):
    """gs_conv_smallcout_fwd (fp32 NCHW logits) and _bwd (dx 16-bit, dw and db fp32 times gscale)"""
    from semantic_segmentation_amd import ops
    Cin, Cout, k, p = case
    N, H, W = 2, 11, 9
    for vset in ("S", "P"):
        r = cached(E.smallcout_build, case, vset)
        what = f"smallcout {_id(case)} {vset} {dtn}"
        OH, OW = r["y"].shape[2], r["y"].shape[3]
        xd = sliced(channels_last(r["x"]), dt)
        wdev, bdev = r["w"].to(dev()), r["b"].to(dev())
        y = nan32(N, Cout, OH, OW)
        ops.conv_smallcout_fwd(xd, wdev, bdev, y, k, 1, p)
        torch.cuda.synchronize()
        assert_exact(y, expect32(r["y"].double() + r["b"].double().view(1, -1, 1, 1)), what + " logits [n][co][y][x]")
        dx = out_buffer((N, H, W, Cin), dt)
        dw = zeros32(Cout, Cin, k, k)
        db = zeros32(Cout)
        ops.conv_smallcout_bwd(xd, wdev, r["dy"].to(dev()), dx, dw, db, k, 1, p, 0.5)
        torch.cuda.synchronize()
        assert_exact(dx, expect16(channels_last(r["dx"]), dt), what + " dx")
        assert_exact(dw, expect32(r["dw"], 0.5), what + " dw")
        assert_exact(db, expect32(r["db"], 0.5), what + " db")


@pytest.mark.parametrize("case", E.STEM_CASES, ids=_id)
def test_stem_stats_exact(case):
    """gs_stem_stats: the tile partials equal the exact sums of y and y^2 of the one-channel convolution it never materialises"""
    from semantic_segmentation_amd import ops
    N, H, W = case
    r = cached(E.stem_build, case)
    mt = ops.conv_smallcin_mtiles(N, H, W)
    part = nan32(ops.bn_partials_numel(mt, 64))
    taps = nan32(mt * 54)
    ops.stem_stats(r["x"].to(dev()), r["w"].to(dev()), part, taps)
    torch.cuda.synchronize()
    assert_exact(stat_sums(part, mt, 64), torch.stack([r["s1"], r["s2"]]), f"stem_stats {_id(case)} ({mt} tiles) [sum y | sum y^2][c]")
    part2 = nan32(ops.bn_partials_numel(mt, 64))
    ops.stem_stats(r["x"].to(dev()), r["w"].to(dev()), part2, None)
    assert torch.equal(part2[: mt * 128], part[: mt * 128])


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.HEAD_CASES, ids=_id)
def test_head1x1_exact(case, dtn, dt):
    """gs_head1x1_bn_fwd / _wgrad on relu(y * scale + shift) with power-of-two scales and integer shifts: fp32 logits, weight
    and bias gradients equal the reference"""
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd._lib import ACT_RELU
    N, H, W, ncls = case
    r = cached(E.head_build, case)
    what = f"head1x1 {_id(case)} {dtn}"
    yd = sliced(channels_last(r["y"]), dt)
    sc, sh = r["scale"].to(dev()), r["shift"].to(dev())
    whd, bhd, dld = r["wh"].to(dev()), r["bh"].to(dev()), r["dl"].to(dev())
    logits = nan32(N, ncls, H, W)
    ops.head1x1_bn_fwd(yd, sc, sh, ACT_RELU, whd, bhd, logits)
    dw = zeros32(ncls, 64, 1, 1)
    db = zeros32(ncls)
    ops.head1x1_bn_wgrad(yd, sc, sh, ACT_RELU, whd, dld, dw, db, gscale=0.5)
    torch.cuda.synchronize()
    assert_exact(logits, expect32(r["logits"]), what + " logits [n][cls][y][x]")
    assert_exact(dw, expect32(r["dw"], 0.5), what + " dw")
    assert_exact(db, expect32(r["db"], 0.5), what + " db")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.COLSUM_CASES, ids=_id)
def test_colsum_exact(case, dtn, dt):
    from semantic_segmentation_amd import ops
    N, H, W, stride, coff, C, y0, x0, h, w, gscale = case
    t = E.draw(E.generator(("colsum",) + tuple(case)), "S", "a", (N, H, W, C))
    assert N * H * W * 8 < E.LIMIT
    buf = sliced(t, dt, stride, coff)
    ws, out = nan32(1024 * C), nan32(C)
    ops.colsum(buf, stride, coff, N, H, W, y0, x0, h, w, C, gscale, ws, out)
    torch.cuda.synchronize()
    assert_exact(out, expect32(t[:, y0:y0 + h, x0:x0 + w].double().sum((0, 1, 2)), gscale), f"colsum {_id(case)} {dtn}")


@pytest.mark.parametrize("case", E.PARTIALS_COLSUM_CASES, ids=_id)
def test_bn_partials_colsum_exact(case):
    from semantic_segmentation_amd import ops
    ntiles, Cfull, coff, C, gscale = case
    p = torch.randint(-1000, 1001, (ntiles, 2, Cfull), generator=E.generator(("pcolsum",) + tuple(case))).float()
    assert ntiles * 1000 < E.LIMIT
    part = nan32(ops.bn_partials_numel(ntiles, Cfull))
    part[: p.numel()] = p.reshape(-1).to(dev())
    out = nan32(C)
    ops.bn_partials_colsum(part, ntiles, Cfull, coff, C, gscale, out)
    torch.cuda.synchronize()
    assert_exact(out, expect32(p[:, 0, coff:coff + C].double().sum(0), gscale), f"bn_partials_colsum {_id(case)}")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.BIAS_FROM_DGRAD_CASES, ids=_id)
def test_upconv_bias_gradient_from_dgrad_partials_exact(case, dtn, dt):
    """the ConvTranspose2d bias gradient = column sums of the second half of d(concat), out of the tile partials of the
    data-gradient convolution that writes d(concat), and out of gs_colsum over the stored tensor: both exact under T(d)"""
    from semantic_segmentation_amd import ops
    N, H, W, Cin, Cout = case
    r = cached(E.bias_from_dgrad_build, case)
    what = f"bias from dgrad partials {_id(case)} T({r['d']}) {dtn}"
    wd = torch.empty(9, Cin, Cout, dtype=dt, device=dev())
    ops.pack_weight(r["w"].to(dev()), None, wd, False)
    rows = ops.conv3x3_stat_rows(N, H, W, Cout, Cin)
    part = nan32(ops.bn_partials_numel(ops.conv3x3_mtiles(N, H, W, Cin), Cin))
    dx = out_buffer((N, H, W, Cin), dt)
    ops.conv3x3(sliced(channels_last(r["dy"]), dt), wd, dx, N, H, W, Cout, Cin, ops.TAPS3_DGRAD, bn_partials=part)
    half = Cin // 2
    db = nan32(half)
    ops.bn_partials_colsum(part, rows, Cin, half, half, 0.5, db)
    ws, db2 = nan32(1024 * half), nan32(half)
    ops.colsum(dx, Cin, half, N, H, W, 0, 0, H, W, half, 0.5, ws, db2)
    torch.cuda.synchronize()
    assert_exact(dx, expect16(channels_last(r["dx"]), dt), what + " dx")
    assert_exact(stat_sums(part, rows, Cin), torch.stack([r["s1"], r["s2"]]), what + f" partial sums ({rows} rows)")
    assert_exact(db, expect32(r["s1"][half:], 0.5), what + " db from partials")
    assert_exact(db2, expect32(r["s1"][half:], 0.5), what + " db from gs_colsum")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.MAXPOOL2D_CASES, ids=_id)
def test_maxpool2x2_fwd_exact(case, dtn, dt):
    from semantic_segmentation_amd import ops
    N, H, W, C, extra = case
    z = E.tied_values(E.generator(("maxpool2d",) + tuple(case)), (N, C, H, W), (-1, 0, 1, 2))
    buf = sliced(channels_last(z), dt, C + extra, 0)
    zp = out_buffer((N, H // 2, W // 2, C), dt)
    ops.maxpool2x2_fwd(buf, zp, N, H, W, C, z_stride=C + extra, z_coff=0)
    torch.cuda.synchronize()
    assert_exact(zp, expect16(channels_last(F.max_pool2d(z.double(), 2)), dt), f"maxpool2x2 {_id(case)} {dtn}")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.MAXPOOL3D_CASES, ids=_id)
def test_maxpool3d_exact_with_ties(case, dtn, dt):
    """gs_maxpool3d_fwd / _bwd on values from {0, 1, 2}: most windows hold their maximum more than once, and the gradient must
    go to the FIRST maximum in ATen scan order (include/gsseg.h), plus the skip gradient -- exactly"""
    from semantic_segmentation_amd import ops
    NB, D, H, W, C = case
    r = cached(E.maxpool3d_build, case)
    what = f"maxpool3d {_id(case)} {dtn} ({100 * r['ties']:.0f} % of the windows tied)"
    zd = sliced(_slices(r["z"]), dt, C + 8, 8)
    out = out_buffer((NB * (D // 2), H // 2, W // 2, C), dt)
    ops.maxpool3d_fwd(zd, out, NB, D, H, W, C, C + 8, 8)
    dz = out_buffer((NB * D, H, W, C), dt)
    dr = sliced(_slices(r["dres"]), dt, C + 16, 16)
    ops.maxpool3d_bwd(zd, sliced(_slices(r["dzp"]), dt), dr, dz, NB, D, H, W, C, C + 8, 8, C + 16, 16)
    torch.cuda.synchronize()
    assert_exact(out, expect16(_slices(r["zp"]), dt), what + " fwd")
    assert_exact(dz, expect16(_slices(r["dz"]), dt), what + " bwd [nb*D+d][y][x][c]")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.POOL_ROUTE_CASES, ids=_id)
def test_pool_gradient_routing_2d_exact_with_ties(case, dtn, dt):
    """gs_bn_act_bwd_apply with bn = 0 (scale 1, shift 0, ReLU): dy = dz * act'(y) + dzp routed to the first maximum of each
    2x2 window, on integer y with ties among the positive values"""
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd._lib import ACT_RELU
    N, H, W, C = case
    r = cached(E.pool_route_build, case)
    yd = sliced(channels_last(r["y"]), dt)
    dbuf = sliced(channels_last(r["dz"]), dt, 2 * C, C)
    dzp = sliced(channels_last(r["dzp"]), dt)
    one, zero = torch.ones(C, device=dev()), torch.zeros(C, device=dev())
    dy = out_buffer((N, H, W, C), dt)
    ops.bn_act_bwd_apply(yd, dbuf, 2 * C, C, dzp, one, zero, zero, one, zero, zero, ACT_RELU, False, dy)
    torch.cuda.synchronize()
    assert_exact(dy, expect16(channels_last(r["dy"]), dt), f"pool routing {_id(case)} {dtn}")


# ================================================================================================ F: Pix2Pix packs
@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.MERGE_CASES, ids=_id)
def test_upconv_merge_pack_exact(case, dtn, dt):
    """gs_upconv_merge_pack with integer weights and softmax3 = (0.5, 0.25, 0.25): the merged 8x8 kernel is an exact multiple of
    0.25, and merged_f32, the class-major forward pack and the 64-slot data-gradient pack all equal it"""
    from semantic_segmentation_amd import ops
    Cin, Cout = case
    r = cached(E.merge_build, case)
    sm = torch.tensor(E.SOFTMAX3, device=dev())
    pf = torch.full((4, 16, Cout, Cin), NAN, dtype=dt, device=dev())
    pd = torch.full((64, Cin, Cout), NAN, dtype=dt, device=dev())
    merged = nan32(Cin, Cout, 8, 8)
    ops.upconv_merge_pack(r["w4"].to(dev()), r["w6"].to(dev()), r["w8"].to(dev()), sm, pf, pd, merged)
    torch.cuda.synchronize()
    what = f"merge_pack {_id(case)} {dtn}"
    assert_exact(merged, expect32(r["wm"]), what + " merged_f32 [ci][co][ky][kx]")
    assert_exact(pf, expect16(E.merged_to_classes(r["wm"]), dt), what + " pack_fwd [class][tap][co][ci]")
    assert_exact(pd, expect16(r["wm"].permute(2, 3, 0, 1).reshape(64, Cin, Cout).contiguous(), dt), what + " pack_dgrad [ky*8+kx][ci][co]")
    assert torch.equal(pf.float(), expect32(E.merged_to_classes(r["wm"])).to(dev()))          # the 16-bit store did not round


@pytest.mark.parametrize("case", E.SPLIT_CASES, ids=_id)
def test_upconv_split_wgrad_exact(case):
    """gs_upconv_split_wgrad_det (nparts = 1) / _parts (nparts > 1, the slabs summed on the way): dW4 / dW6 / dW8 =
    gscale * softmax3[j] * the window of the merged gradient, and the three dot products"""
    from semantic_segmentation_amd import ops
    Cin, Cout, nparts = case
    assert nparts == 1 or ops.upconv_split_wgrad_parts_ok(Cin, Cout)
    r = cached(E.split_build, case)
    sm = torch.tensor(E.SOFTMAX3, device=dev())
    dws = {k: nan32(Cin, Cout, k, k) for k in (4, 6, 8)}
    dots = zeros32(3)
    src = (r["slabs"] if nparts > 1 else E.expect32(r["dwm"])).to(dev()).contiguous()
    ops.upconv_split_wgrad(src, r["w4"].to(dev()), r["w6"].to(dev()), r["w8"].to(dev()), sm, 0.5, dws[4], dws[6], dws[8], dots, nparts=nparts)
    torch.cuda.synchronize()
    what = f"split_wgrad {_id(case)}"
    for j, k in enumerate((4, 6, 8)):
        assert_exact(dws[k], expect32(r["wins"][k].contiguous() * E.SOFTMAX3[j], 0.5), what + f" dW{k}")
    assert_exact(dots, expect32(r["dots"], 0.5), what + " dots3")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.IMAGE_FWD_CASES, ids=_id)
def test_upconv8_image_fwd_exact(case, dtn, dt):
    """gs_upconv8_image_fwd: merged 8x8 / s2 / p3 transposed conv + bias to a 1..4-channel fp32 NCHW image, from a channel slice"""
    from semantic_segmentation_amd import ops
    N, h, w, Cin, Cout = case
    assert ops.upconv8_image_fits(Cin, Cout)
    r = cached(E.image_fwd_build, case)
    xin = sliced(channels_last(r["x"]), dt, Cin + 16, 8)
    out = nan32(N, Cout, 2 * h, 2 * w)
    ops.upconv8_image_fwd(xin, r["pack"].to(dt).to(dev()), r["b"].to(dev()), out, None, N, h, w, Cin, Cout, 0, in_stride=Cin + 16, in_coff=8)
    torch.cuda.synchronize()
    assert_exact(out, expect32(r["y"]), f"upconv8_image_fwd {_id(case)} {dtn} [n][co][y][x]")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.IMAGE_WGRAD_CASES, ids=_id)
def test_upconv8_image_wgrad_exact(case, dtn, dt):
    from semantic_segmentation_amd import ops
    N, h, w, Cin = case
    assert ops.upconv8_image_wgrad_ok(Cin, 1) and not ops.upconv8_image_wgrad_ok(Cin, 3) and not ops.upconv8_image_wgrad_ok(64, 1)
    r = cached(E.image_wgrad_build, case)
    xd = sliced(channels_last(r["x"]), dt)
    du = sliced(channels_last(r["du"]), dt, 8, 0)                            # the padding channels must not be read
    outs = []
    for _ in range(2):
        dwm = nan32(4, 16, 1, Cin)
        ops.upconv8_image_wgrad(xd, du, dwm, N, h, w, Cin)
        outs.append(dwm)
    torch.cuda.synchronize()
    assert_exact(outs[0], expect32(r["dwm"]), f"upconv8_image_wgrad {_id(case)} {dtn} [class][tap][0][ci]")
    assert torch.equal(outs[0], outs[1])


# ================================================================================================ G: BatchNorm / activation
# gs_bn_act_apply, gs_bn_act_bwd_reduce -> gs_bn_bwd_coeffs -> gs_bn_act_bwd_apply and their head-source entry points on the
# operands of exact_reference.bn_build: every fp32 intermediate is exactly representable (proven on the CPU in
# tests/test_exact_reference_cpu.py), so z, zp, the tile sums, dgamma / dbeta and dy are compared at zero tolerance.
def _act_code(name):
    from semantic_segmentation_amd import _lib
    return {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "leaky": _lib.ACT_LEAKY02}[name]


def _vec(t):
    return None if t is None else t.float().to(dev()).contiguous()


def _bn_build_any(case):
    return E.bn_head_build(case) if len(case) == 5 else E.bn_build(*case)


def _bn_forward(ops, c, p, ref, dt, what):
    """z into channels [8, 8 + C) of a C + 16 wide buffer (sentinel intact around it) and the pooled zp, exact"""
    N, C, H, W = c["y"].shape
    z = out_buffer((N, H, W, C), dt, C + 16, 8)
    zp = out_buffer((N, H // 2, W // 2, C), dt) if c["pooled"] else None
    ops.bn_act_apply(p["y"], p["scale"], p["shift"], _act_code(c["act"]), z, C + 16, 8, zp, p["keep"], c["keep_scale"])
    torch.cuda.synchronize()
    assert_slice(z, 8, channels_last(ref["z"]), what + " z")
    if zp is not None:
        assert_exact(zp, channels_last(ref["zp"]), what + " zp")


def _bn_chain(ops, c, dt, what, forward=True, backward=True):
    """one case through the forward apply and the backward chain.  The only comparison that is not an equality: c1 / c2 =
    float32(s / count) may be the ADJACENT fp32 value where count is no power of two (the double quotient is rounded twice);
    with a power-of-two count it is exact too."""
    N, C, H, W = c["y"].shape
    head = c["dza_kind"] == "head"
    ref = E.bn_reference(c, dt)
    p = {"y": sliced(channels_last(c["y"]), dt), "dzp": None if c["dzp"] is None else sliced(channels_last(c["dzp"]), dt),
         "dzb": None if c["dzb"] is None else sliced(channels_last(c["dzb"]), dt),
         "keep": None if c["keep"] is None else channels_last(c["keep"]).to(dev())}
    p["sa"], p["ca"] = (2 * C, C) if c["dza_kind"] == "slice" else (C, 0)
    p["dza"] = sliced(channels_last(c["dza"]), dt, p["sa"], p["ca"]) if c["dza_kind"] in ("slice", "dense") else None
    for k in ("scale", "shift", "mean", "invstd", "c1", "c2"):
        p[k] = _vec(c[k])
    if forward and not head:
        _bn_forward(ops, c, p, ref, dt, what)
    if not backward:
        return
    act, act_b = _act_code(c["act"]), _act_code(c["act_b"])
    if head:
        dl, wh = c["dl"].to(dev()).contiguous(), c["w_head"].to(dev()).contiguous()
    # ---- reduce: NaN-filled partials; the used tiles finite, their fp64 sum exact, nothing behind them written
    used = ops.bn_bwd_tiles_used(N, H, W, c["pooled"])
    part = nan32(ops.bn_partials_numel(ops.bn_bwd_tiles(N, H, W), C))
    if head:
        ops.bn_act_bwd_reduce_head(p["y"], dl, wh, p["scale"], p["shift"], p["mean"], p["invstd"], act, part)
    else:
        ops.bn_act_bwd_reduce(p["y"], p["dza"], p["sa"], p["ca"], p["dzp"], p["scale"], p["shift"], p["mean"], p["invstd"], act, part,
                              p["dzb"], act_b, p["keep"], c["keep_scale"])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(part[: used * 2 * C]).all()), what + f": a partial of the {used} used tiles was not written"
    assert bool(torch.isnan(part[used * 2 * C:]).all()), what + f": written behind the {used} used tiles"
    sums = torch.stack([ref["s1"], ref["s2"]])
    assert_exact(stat_sums(part, used, C), sums, what + f" tile sums ({used} tiles)")
    # ---- coefficients out of those partials (direct up to 512 tiles, two-stage above)
    count = N * H * W
    dgamma, dbeta, c1, c2 = nan32(C), nan32(C), nan32(C), nan32(C)
    ops.bn_bwd_coeffs(part, used, C, count, 0.5, dgamma, dbeta, c1, c2)
    torch.cuda.synchronize()
    assert_exact(dbeta, expect32(ref["s1"], 0.5), what + " dbeta")
    assert_exact(dgamma, expect32(ref["s2"], 0.5), what + " dgamma")
    for got, s, name in ((c1, ref["s1"], "c1"), (c2, ref["s2"], "c2")):
        want = torch.from_numpy((s.numpy() / float(count)).astype("float32")).to(dev())
        ok = got == want
        if not E.pow2(count):
            ok = ok | (got == torch.nextafter(want, torch.full_like(want, float("inf")))) | (got == torch.nextafter(want, torch.full_like(want, -float("inf"))))
        assert_exact(got, want, what + f" {name} ({used} tiles, count {count})", ok=ok)
    # ---- apply with the dyadic c1 / c2 of the builder
    dy = out_buffer((N, H, W, C), dt)
    if head:
        ops.bn_act_bwd_apply_head(p["y"], dl, wh, p["scale"], p["shift"], p["mean"], p["invstd"], p["c1"], p["c2"], act, dy)
    else:
        co = [p[k] if (c["bn"] or c["scale"] is not None) else None for k in ("mean", "invstd", "c1", "c2")]      # identity: all NULL
        ops.bn_act_bwd_apply(p["y"], p["dza"], p["sa"], p["ca"], p["dzp"], p["scale"], p["shift"], co[0], co[1], co[2], co[3], act, c["bn"], dy,
                             p["dzb"], act_b, p["keep"], c["keep_scale"])
    torch.cuda.synchronize()
    assert_exact(dy, expect16(channels_last(ref["dy"]), dt), what + " dy")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.BN_CASES, ids=E.bn_id)
def test_bn_act_chain_exact(case, dtn, dt):
    """forward apply, backward reduce, coefficients and backward apply of one (shape, pooled, variant) at zero tolerance: see
    exact_reference.BN_VARIANTS for the variants and BN_SHAPES for what each shape reaches"""
    from semantic_segmentation_amd import ops
    shape, pooled, _ = case
    if shape in E.BN_TWO_STAGE_SHAPES:                         # what reaches the two-stage path of gs_bn_bwd_coeffs
        assert ops.bn_bwd_tiles_used(*shape[:3], pooled) > 512
    _bn_chain(ops, cached(_bn_build_any, case), dt, f"bn {E.bn_id(case)} {dtn}")


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.BN_FWD_ONLY_CASES, ids=E.bn_id)
def test_bn_act_apply_grid_stride_exact(case, dtn, dt):
    """1.18 M work items on the 4096-block grid: the grid-stride loop of the forward apply takes a second trip, tail first"""
    from semantic_segmentation_amd import ops
    N, H, W, C = case[0]
    assert N * H * W * (C // 8) > 4096 * 256
    _bn_chain(ops, cached(_bn_build_any, case), dt, f"bn forward {E.bn_id(case)} {dtn}", backward=False)


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("case", E.BN_HEAD_CASES, ids=_id)
def test_bn_bwd_head_source_exact(case, dtn, dt):
    """the head-source reduce and apply (dz_a formed in fp32 from dl and w_head, 1, 2 and 4 classes) at zero tolerance"""
    from semantic_segmentation_amd import ops
    _bn_chain(ops, cached(_bn_build_any, case), dt, f"bn head {_id(case)} {dtn}")


def test_bn_bwd_head_source_two_lds_chunks_exact():
    """2.17 M pixels in 1024 tiles of 2116: the logit gradients of a tile are staged in LDS in a chunk of 2048 and one of 68"""
    from semantic_segmentation_amd import ops
    N, H, W, C, ncls = E.BN_HEAD_TWO_CHUNKS
    assert -(-N * H * W // ops.bn_bwd_tiles_used(N, H, W, False)) > 2048
    _bn_chain(ops, cached(_bn_build_any, E.BN_HEAD_TWO_CHUNKS), torch.float16, f"bn head {_id(E.BN_HEAD_TWO_CHUNKS)} f16")


def _check_neighbours(got, ref64_cl, what):
    ok, share = E.neighbour16(got, ref64_cl)
    print(f"{what}: {100 * share:.3f} % of the elements on the neighbour")
    assert_exact(got, ref64_cl.to(got.dtype), what, ok=ok)
    assert share <= E.TANH_NEIGHBOUR_SHARE, f"{what}: {share} of the elements sit on the neighbouring 16-bit value"


@pytest.mark.parametrize("dtn,dt", DTS)
@pytest.mark.parametrize("shape,pooled", E.TANH_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else ("pool" if v else "plain"))
def test_bn_act_tanh_per_element(shape, pooled, dtn, dt):
    """ACT_TANH (the generic kernel, NULL coefficients; the Pix2Pix output layer): the forward apply with and without the pool
    and the bn = 0 backward apply, per element against fp64 -- the correctly rounded 16-bit value or its neighbour; no norm.
    Why one place at most: the kernel forms tanhf(y) (a few fp32 ulp, relative error below 2^-21) and for the gradient
    dz * (1 - t * t), whose cancellation multiplies the error of t by 2 t^2 / (1 - t^2) <= 9.1 for |y| <= 1.5 -- still below
    2^-17 relative, while neighbouring 16-bit values are at least 2^-11 (fp16) or 2^-8 (bf16) apart, relatively.  The computed
    value therefore lies within a small fraction of one 16-bit step of the true one, at most one rounding boundary lies
    between them, and round-to-nearest lands on the same value or the adjacent one.  The share that does land on the neighbour
    is about error / step: capped at TANH_NEIGHBOUR_SHARE, the figure the CPU test asserts for an fp32 evaluation of the same
    operands.  zp must be EXACTLY the maximum over the z the kernel stored."""
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd._lib import ACT_TANH
    N, H, W, C = shape
    r = cached(E.tanh_build, shape, pooled)
    what = f"tanh {_id(shape)} {dtn}"
    y = sliced(channels_last(r["y"]), dt)
    z = out_buffer((N, H, W, C), dt)
    zp = out_buffer((N, H // 2, W // 2, C), dt) if pooled else None
    ops.bn_act_apply(y, None, None, ACT_TANH, z, C, 0, zp)
    dy = out_buffer((N, H, W, C), dt)
    ops.bn_act_bwd_apply(y, sliced(channels_last(r["dz"]), dt), C, 0, None, None, None, None, None, None, None, ACT_TANH, False, dy)
    torch.cuda.synchronize()
    _check_neighbours(z, channels_last(r["z"]), what + " z")
    if pooled:
        assert torch.equal(zp, F.max_pool2d(z.permute(0, 3, 1, 2).float(), 2).permute(0, 2, 3, 1).to(dt)), what + " zp is not the max over the stored z"
    _check_neighbours(dy, channels_last(r["dy"]), what + " dy")


def _assert_coeffs(got, ref, roundings, what):
    for name, t in got.items():
        err = (t.double().cpu().numpy() - ref[name])
        bound = E.coeff_bound(ref, name, roundings)
        bad = ~(abs(err) <= bound)                             # a NaN is bad
        assert not bad.any(), f"{what} {name}: channels {bad.nonzero()[0].tolist()[:8]} err {err[bad][:4]} bound {bound[bad][:4]}"


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "null"])
@pytest.mark.parametrize("ntiles", E.BN_FINALIZE_TILES)
@pytest.mark.parametrize("C", E.BN_FINALIZE_C)
def test_bn_finalize_against_fp64(C, ntiles, affine):
    """gs_bn_finalize on synthetic fp32 partials against numpy fp64, direct (<= 512 tiles) and two-stage; momentum 0.1.  Not
    exact (1 / sqrt), so each output is bounded by its fp32 roundings, each at most 2^-24 of the magnitude of the terms it
    touches (exact_reference.BN_FINALIZE_ROUNDINGS); the double sums before them (about 1e-9 of invstd at most, on the
    channel with |mean| = 100 std) get no allowance of their own:
      mean    1  (float) of the double mean
      invstd  1  (float) of the double 1 / sqrt(var + eps)
      scale   2  invstd, gamma * invstd
      shift   5  on mean * scale: (float) mean, the two of scale, the product; on the result: the subtraction -- relative
                 to |beta| + |mean * scale|
      running 3  on each term of (1 - m) * r + m * x: the factor (1 - m, or (float) x), the product, the sum -- relative to
                 |(1 - m) r| + |m x|
    Channel 0 is constant with a raw variance below zero: it must clamp (invstd = 1 / sqrt(eps), not NaN); channel 1 has
    |mean| = 100 std; with one tile, a second call has count = 1 (the unbiased variance must not divide by zero)."""
    from semantic_segmentation_amd import ops
    for count_one in ((False, True) if ntiles == 1 else (False,)):
        r = E.bn_finalize_build(C, ntiles, count_one)
        ref = E.bn_finalize_reference(r, affine)
        part = nan32(ops.bn_partials_numel(ntiles, C))
        part[: ntiles * 2 * C] = r["partials"].reshape(-1).to(dev())
        out = {k: nan32(C) for k in ("scale", "shift", "mean", "invstd")}
        rm, rv = zeros32(C), zeros32(C)
        rm.copy_(r["rm"]), rv.copy_(r["rv"])
        ops.bn_finalize(part, ntiles, C, r["count"], _vec(r["gamma"]) if affine else None, _vec(r["beta"]) if affine else None, rm, rv,
                        E.BN_MOMENTUM, E.BN_EPS, out["scale"], out["shift"], out["mean"], out["invstd"])
        torch.cuda.synchronize()
        out.update(rm=rm, rv=rv)
        what = f"bn_finalize C{C} tiles{ntiles} count{r['count']:.0f}"
        _assert_coeffs(out, ref, E.BN_FINALIZE_ROUNDINGS, what)
        import numpy as np
        assert float(out["invstd"][0]) == float(np.float32(1.0 / np.sqrt(float(np.float32(E.BN_EPS))))), what + ": the constant channel did not clamp"


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "null"])
@pytest.mark.parametrize("C", E.BN_FINALIZE_C)
def test_bn_eval_coeffs_against_fp64(C, affine):
    """gs_bn_eval_coeffs (all fp32) against numpy fp64 (exact_reference.BN_EVAL_ROUNDINGS): invstd 3 (the sum rv + eps counts
    half, the square root, the division); scale 4 (+ the product); shift 6 (the four of scale and the product on rm * scale, the
    subtraction) relative to |beta| + |rm * scale|; mean is rm itself."""
    import numpy as np
    from semantic_segmentation_amd import ops
    r = E.bn_finalize_build(C, 2)
    gamma = r["gamma"].numpy().astype(np.float64) if affine else np.ones(C)
    beta = r["beta"].numpy().astype(np.float64) if affine else np.zeros(C)
    rm, rv = r["rm"].numpy().astype(np.float64), r["rv"].numpy().astype(np.float64)
    invstd = 1.0 / np.sqrt(rv + float(np.float32(E.BN_EPS)))
    ref = {"mean": rm, "invstd": invstd, "scale": gamma * invstd, "shift": beta - rm * gamma * invstd,
           "mag": {"mean": np.abs(rm), "invstd": invstd, "scale": np.abs(gamma * invstd), "shift": np.abs(beta) + np.abs(rm * gamma * invstd)}}
    out = {k: nan32(C) for k in ("scale", "shift", "mean", "invstd")}
    ops.bn_eval_coeffs(C, _vec(r["gamma"]) if affine else None, _vec(r["beta"]) if affine else None, _vec(r["rm"]), _vec(r["rv"]), E.BN_EPS,
                       out["scale"], out["shift"], out["mean"], out["invstd"])
    torch.cuda.synchronize()
    _assert_coeffs(out, ref, E.BN_EVAL_ROUNDINGS, f"bn_eval_coeffs C{C}")


def bn_rev_child():
    """runs in a fresh process started with GSSEG_BN_REV=4: the cases of BN_REV_CASES, both dtypes, the same exact assertions"""
    import os
    from semantic_segmentation_amd import ops
    assert os.environ.get("GSSEG_BN_REV") == "4"
    for case in E.BN_REV_CASES:
        for dtn, dt in DTS:
            _bn_chain(ops, cached(_bn_build_any, case), dt, f"bn GSSEG_BN_REV=4 {E.bn_id(case)} {dtn}")
    torch.cuda.synchronize()
    for flat, n in _GUARDED:
        assert bool((flat[:GUARD] == GUARD_VALUE).all()) and bool((flat[GUARD + n:] == GUARD_VALUE).all()), "guard words overwritten"
    print("bn_rev_child OK")


def test_bn_traversal_knob_reversed_backward_apply():
    """GSSEG_BN_REV is read once per process and its default 3 never reverses the backward apply: three small cases here, then
    the same in ONE fresh child process with GSSEG_BN_REV=4 (forward apply and reduce head first, backward apply tail first).
    A failure here ends the test before the child is started."""
    import os
    import subprocess
    import sys
    from semantic_segmentation_amd import ops
    for case in E.BN_REV_CASES:
        _bn_chain(ops, cached(_bn_build_any, case), torch.float16, f"bn default traversal {E.bn_id(case)} f16")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GSSEG_BN_REV="4")
    res = subprocess.run([sys.executable, "-c", "from tests.test_exact_kernels_gpu import bn_rev_child; bn_rev_child()"], cwd=root, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0 and "bn_rev_child OK" in res.stdout, res.stdout[-4000:]
