"""CPU proofs for the 3-D Pix2Pix generator's two operators (tests/cell3d_reference.py), no GPU:
  * the fp64 statements equal torch.autograd through three nn.Conv3d plus softmax, and through interpolate + split / stack / sum, at 1e-9,
    and the fixture the reference's own classes made (tests/golden/pix2pix3d_cells.npz);
  * the gathered 64-tap form equals the k8 conv EXACTLY on integers (odd sizes, N = 2); the reachable-tap rule holds;
  * on the GPU tests' seeds a right implementation passes the GPU bounds and the stated wrong implementations do not;
  * the module tree, state-dict keys and shapes of networks3d.Cell_conv equal the fixture's key list (strict load); the 2-D module's
    globals have not moved; the new entry points are declared, bound and exported with ABI 54."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from golden_util import grad_summary, tensor_checksum
from golden_util_cell3d import FIXTURES, fixture_arch, fixture_input, fixture_state_dict
from tests import cell3d_reference as c3
from tests import exact_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(min(torch.get_num_threads(), 16))
SHAPES = [(3, 4, True, 2, (4, 6, 8)), (2, 3, True, 1, (5, 7, 6)), (2, 2, False, 2, (2, 2, 2)), (1, 2, True, 2, (3, 2, 5))]


def close(a, b, tol=1e-9):
    return float((a.detach().double() - b.detach().double()).norm()) <= tol * max(float(b.detach().double().norm()), 1e-300)


@pytest.mark.parametrize("Cin,Cout,bias,N,vol", SHAPES)
def test_cell_statement_equals_autograd_through_three_conv3d_and_softmax(Cin, Cout, bias, N, vol):
    g = torch.Generator().manual_seed(5)
    convs = [nn.Conv3d(Cin, Cout, k, stride=2, padding=c3.KSP[k][1], bias=bias).double() for k in c3.KS]
    for c in convs:
        for p in c.parameters():
            p.data = torch.randn(p.shape, generator=g, dtype=torch.float64)
    x = torch.randn((N, Cin) + vol, generator=g, dtype=torch.float64, requires_grad=True)
    row = torch.randn(3, generator=g, dtype=torch.float64, requires_grad=True)
    sm = F.softmax(row, dim=-1)
    y = sum(w * c(x) for w, c in zip(sm, convs))
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    ws = [c.weight.detach() for c in convs]
    bs = [c.bias.detach() for c in convs] if bias else None
    for form in ("k8", "gathered"):
        r = c3.cell_statement(x.detach(), ws, bs, sm.detach(), dy, form=form)
        assert close(r["y"], y) and close(r["dx"], x.grad) and close(c3.softmax_row_grad(row.detach(), r["dsm"]), row.grad), form
        for k, c in zip(c3.KS, convs):
            assert close(r[f"dw{k}"], c.weight.grad), (form, k)
            if bias:
                assert close(r[f"db{k}"], c.bias.grad), (form, k)


@pytest.mark.parametrize("C,N,vol", [(8, 2, (2, 3, 4)), (4, 1, (1, 1, 1)), (8, 1, (3, 2, 5)), (12, 1, (4, 4, 4))])
def test_upsample_statement_equals_interpolate_split_stack_sum(C, N, vol):
    g = torch.Generator().manual_seed(6)
    x = torch.randn((N, C) + vol, generator=g, dtype=torch.float64, requires_grad=True)
    y = c3.torch_upsample(x)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    r = c3.upsample_statement(x.detach(), dy)
    assert close(r["y"], y) and close(r["dx"], x.grad)
    for n in (1, 2, 5):                                           # output 0 equals x[0]; every row sums to one
        U = c3.up_matrix(n)
        assert float(U[0, 0]) == 1.0 and float(U[-1, -1]) == 1.0 and torch.equal(U.sum(1), torch.ones(2 * n, dtype=torch.float64))


def fixture_reference(f, g, store=None):
    t = f["tag"] + "/"
    x, dense = fixture_input(f), torch.from_numpy(g[t + "dense"])
    if f["kind"] == "up":
        return c3.upsample_statement(x, dense, store=store), None, None
    sd, arch = fixture_state_dict(f), fixture_arch(f)
    ks = c3.KS if f["kind"] in ("cell", "mixed") else (int(f["kind"][5]),)
    pre = {"cell": "_ops._ops.%d.", "mixed": "_ops.%d."}.get(f["kind"])
    ws, bs = [], []
    for k in c3.KS:
        if k in ks:
            p = pre % ks.index(k) if pre else ""
            ws.append(sd[p + "op.weight"])
            bs.append(sd.get(p + "op.bias"))
        else:
            ws.append(torch.zeros((f["cout"], f["cin"], k, k, k)))
            bs.append(torch.zeros(f["cout"]))
    sm = torch.softmax(arch[f["layer"]], -1) if len(ks) == 3 else torch.tensor([float(k in ks) for k in c3.KS], dtype=torch.float64)
    return c3.cell_statement(x, ws, bs if f["bias"] else None, sm, dense, store=store), sd, arch


@pytest.mark.parametrize("i", range(len(FIXTURES["pix2pix3d_cells"])))
def test_statement_equals_the_fixture_of_the_reference(i, golden_dir):
    """the reference's own Cell_conv / MixedOp_conv / conv_* / LinearAdditiveUpsample in double: output, dx, every parameter gradient and
    the conv_arch gradient at 1e-9; the seeded weights have the stored checksums"""
    f = FIXTURES["pix2pix3d_cells"][i]
    g = dict(np.load(os.path.join(golden_dir, "pix2pix3d_cells.npz")))
    t = f["tag"] + "/"
    assert os.path.getsize(os.path.join(golden_dir, "pix2pix3d_cells.npz")) < 512 * 1024
    assert np.array_equal(g[t + "input"], fixture_input(f).numpy())
    r, sd, arch = fixture_reference(f, g)
    assert close(r["y"], torch.from_numpy(g[t + "y"]))
    assert np.allclose(grad_summary(r["dx"]), g[t + "gsum/dx"], rtol=1e-9, atol=1e-18)
    if sd is None:
        return
    assert np.array_equal(g[t + "arch"], arch.numpy())
    for k, v in sd.items():
        assert np.array_equal(tensor_checksum(v), g[t + "wsum/" + k]), k
        kk = v.shape[2] if v.dim() == 5 else sd[k[:-4] + "weight"].shape[2]
        if v.dim() == 5:
            assert np.allclose(grad_summary(r[f"dw{kk}"]), g[t + "gsum/" + k], rtol=1e-9, atol=1e-18), k
        else:
            assert close(r[f"db{kk}"], torch.from_numpy(g[t + "grad/" + k])), k
    want = torch.from_numpy(g[t + "grad/arch"])
    if f["kind"] == "cell":
        assert close(c3.softmax_row_grad(arch[f["layer"]], r["dsm"]), want[f["layer"]])
        assert not bool(want[[j for j in range(6) if j != f["layer"]]].any())
    elif f["kind"] == "mixed":
        assert close(c3.softmax_row_grad(arch[f["layer"]], r["dsm"]), want[f["layer"]])


@pytest.mark.parametrize("Cin,Cout,N,vol", [(2, 3, 2, (4, 6, 8)), (3, 2, 2, (5, 7, 6)), (1, 2, 1, (2, 2, 2)), (2, 2, 2, (3, 2, 9))])
def test_gathered_64_tap_form_equals_the_k8_conv_exactly_on_integers(Cin, Cout, N, vol):
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-8, 9, (N, Cin) + vol, generator=g).double()
    wm = torch.randint(-12, 13, (Cout, Cin, 8, 8, 8), generator=g).double() / 4
    want = F.conv3d(x, wm, None, stride=2, padding=3)
    assert torch.equal(c3.gathered_conv(x, wm), want)
    xg = c3.gather(x)
    assert xg.shape == (N, 8 * Cin) + tuple(c3.gathered_size(d) for d in vol)
    assert torch.equal(c3.ungathered_weight(c3.gathered_weight(wm)), wm)
    for m in ("unshifted_parity",) + (("sample_leak",) if N > 1 else ()):
        assert not torch.equal(c3.gathered_conv(x, wm, m), want), m
    # the expected device tensors of the kernel test are the same statement
    dt0, nd = (-1, -1, -1), (4, 4, 4)
    pf = c3.pack_fwd_expected(wm, dt0, nd)
    assert pf.shape == (64, Cout, 8 * Cin) and float(pf[0, 1, 0]) == float(wm[1, 0, 0, 0, 0]) and float(pf[63, 0, 7 * Cin]) == float(wm[0, 0, 7, 7, 7])
    pd = c3.pack_dgrad_expected(wm, (0, 0, 0), (8, 8, 8), 8)
    assert pd.shape == (512, 8, Cout) and float(pd[511, Cin - 1, 1]) == float(wm[1, Cin - 1, 7, 7, 7]) and not bool(pd[:, Cin:].any())


def test_reachable_tap_rule():
    """tap k meets data iff some output o has 0 <= 2o + k - 3 < d: the host rule equals brute force; the taps outside the box change
    nothing and receive no gradient; 8 of 512 taps live at 2x2x2, 216 at 4x4x4; the gathered box covers the tap box"""
    from semantic_segmentation_amd import ops
    for d in range(2, 20):
        ks = c3.reachable_taps(d)
        assert ops.cell3d_reachable_taps(d) == ks == list(range(ks[0], ks[-1] + 1))
        assert ops.cell3d_gathered_size(d) == c3.gathered_size(d) == -(-(d + 1) // 2)
    assert len(c3.reachable_taps(2)) ** 3 == 8 and len(c3.reachable_taps(4)) ** 3 == 216 and len(c3.reachable_taps(6)) == 8
    g = torch.Generator().manual_seed(8)
    for vol in ((2, 2, 2), (3, 4, 2), (4, 5, 6)):
        dt0, nd, k0, nk = ops.cell3d_boxes(*vol)
        for a in range(3):
            ks = c3.reachable_taps(vol[a])
            assert (k0[a], nk[a]) == (ks[0], len(ks))
            assert 2 * dt0[a] + 2 <= ks[0] and ks[-1] <= 2 * (dt0[a] + nd[a] - 1) + 3 and -1 <= dt0[a] and dt0[a] + nd[a] <= 3
        x = torch.randn((2, 2) + vol, generator=g, dtype=torch.float64, requires_grad=True)
        wm = torch.randn((3, 2, 8, 8, 8), generator=g, dtype=torch.float64, requires_grad=True)
        y = F.conv3d(x, wm, None, stride=2, padding=3)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        dx, dw = torch.autograd.grad(y, [x, wm], dy)
        mask = torch.zeros(8, 8, 8, dtype=torch.float64)
        mask[k0[0]:k0[0] + nk[0], k0[1]:k0[1] + nk[1], k0[2]:k0[2] + nk[2]] = 1
        assert not bool((dw * (1 - mask)).any()) and bool((dw * mask).abs().sum() > 0)
        xb = x.detach().clone().requires_grad_(True)
        yb = F.conv3d(xb, wm.detach() * mask, None, stride=2, padding=3)
        assert torch.equal(yb, y.detach()) and torch.equal(torch.autograd.grad(yb, xb, dy)[0], dx)
    assert ops.cell3d_boxes(2, 2, 2, full=True) == ((-1, -1, -1), (4, 4, 4), (0, 0, 0), (8, 8, 8))
    with pytest.raises(NotImplementedError):
        ops.cell3d_boxes(1, 4, 4)


def _exact16(t, dt):
    return er.expect16(t, dt)


def test_exact_cases_are_exact_and_tell_the_wrong_cells():
    """every case of tests/test_cell3d_kernels_gpu.py: the operands hold the exactness conditions (an fp32 evaluation in the gathered form
    -- another order of summation -- gives the very same numbers), merged weights are exact in bf16, and each stated wrong implementation
    differs from the expected values in some element of some case"""
    told = {m: False for m in c3.CELL_MUTANTS}
    for case in c3.CELL_CASES + [c3.COFF_CASE]:
        for smn in sorted(c3.SM_SETS):
            r = c3.cell_build(case, smn)
            assert torch.equal(r["wm"].to(torch.bfloat16).double(), r["wm"]) and float(r["wm"].abs().max()) <= 3
            er.require_integers(r["x"], r["dy"], *r["ws"], *r["bs"])
            for rr in (r, r["dots"]):
                f32 = c3.cell_statement(r["x"], r["ws"], r["bs"], r["sm"], rr["dy"], dtype=torch.float32, form="gathered")
                for k in ("y", "dx", "dsm", "dw4", "dw6", "dw8", "db4", "db6", "db8"):
                    assert torch.equal(f32[k].double(), rr[k]), (case, smn, k)
                assert bool(rr["dy"].any())
            if smn != "mixed":
                continue
            for m in c3.CELL_MUTANTS:
                w = c3.cell_statement(r["x"], r["ws"], r["bs"], r["sm"], r["dots"]["dy"], mutant=m)
                keys = {"no_sm_dw": ("dw4", "dw6", "dw8"), "no_bias_share": ("dsm",)}.get(m, ("y", "dx", "dw8"))
                if any(not torch.equal(_exact16(w[k], torch.float16) if k in ("y", "dx") else w[k].float(),
                                       _exact16(r["dots"][k], torch.float16) if k in ("y", "dx") else r["dots"][k].float()) for k in keys):
                    told[m] = True
    assert all(told.values()), told


def test_exact_cases_tell_the_wrong_upsamples():
    told = {m: False for m in c3.UP_MUTANTS}
    for case in c3.UP_CASES:
        r = c3.up_build(case)
        er.require_integers(r["x"], r["dy"])
        f32 = c3.upsample_statement(r["x"], r["dy"], dtype=torch.float32)
        assert torch.equal(f32["y"].double(), r["y"]) and torch.equal(f32["dx"].double(), r["dx"])
        assert torch.equal(r["y"] * 64, (r["y"] * 64).round()) and torch.equal(r["dx"] * 64, (r["dx"] * 64).round())
        for m in c3.UP_MUTANTS:
            w = c3.upsample_statement(r["x"], r["dy"], mutant=m)
            if any(not torch.equal(_exact16(w[k], torch.bfloat16) if m != "align_corners" else w[k].to(torch.bfloat16),
                                   _exact16(r[k], torch.bfloat16)) for k in ("y", "dx")):
                told[m] = True
    assert all(told.values()), told


def test_module_bounds_pass_a_right_implementation_and_fail_the_wrong_ones():
    """the cases and seeds of tests/test_cell3d_modules_gpu.py under its comparer: an fp32 evaluation through the gathered form with the
    engine's 16-bit stores passes every tensor of every case; each stated wrong implementation fails in some case"""
    told = {m: False for m in c3.CELL_MUTANTS + c3.UP_MUTANTS}
    for cid in sorted(c3.MODULE_CASES):
        dt = c3.DT[c3.MODULE_CASES[cid][5]]
        r64, r16 = c3.module_reference(cid), c3.module_reference(cid, store=dt)
        rep, bad = c3.hold(c3.module_reference(cid, store=dt, dtype=torch.float32, form="gathered"), r64, r16)
        assert not bad, (cid, {k: rep[k] for k in bad})
        assert all(v["e16"] > 0 for k, v in rep.items() if not k.startswith("db")), cid
        for m in c3.CELL_MUTANTS:
            told[m] |= bool(c3.hold(c3.module_reference(cid, store=dt, mutant=m), r64, r16)[1])
    for cid in sorted(c3.UP_MODULE_CASES):
        dt = c3.DT[c3.UP_MODULE_CASES[cid][3]]
        r64, r16 = c3.up_module_reference(cid), c3.up_module_reference(cid, store=dt)
        rep, bad = c3.hold(c3.up_module_reference(cid, store=dt, dtype=torch.float32), r64, r16)
        assert not bad, (cid, {k: rep[k] for k in bad})
        for m in c3.UP_MUTANTS:
            told[m] |= bool(c3.hold(c3.up_module_reference(cid, store=dt, mutant=m), r64, r16)[1])
    assert all(told.values()), told


def test_module_tree_and_state_dict_keys_are_the_references(golden_dir):
    """networks3d.Cell_conv / MixedOp_conv / conv_*: the fixture's key lists and 5-D shapes, load_state_dict(strict=True) on the CPU; the
    module globals of the 3-D file (6 rows, arch_parameters() == [conv_arch], read NOW) and of the 2-D file (unchanged); CPU tensors raise"""
    from semantic_segmentation_amd.architecture_pix2pix import operations
    from semantic_segmentation_amd.models_pix2pix import networks, networks3d
    g = dict(np.load(os.path.join(golden_dir, "pix2pix3d_cells.npz")))
    for f in FIXTURES["pix2pix3d_cells"]:
        if f["kind"] == "up":
            continue
        t = f["tag"] + "/"
        if f["kind"] == "cell":
            net = networks3d.Cell_conv(f["cin"], f["cout"], f["bias"], f["layer"])
            assert [n for n, _ in net.named_modules()][:4] == ["", "_ops", "_ops._ops", "_ops._ops.0"] and net._layer_index == f["layer"]
        elif f["kind"] == "mixed":
            net = networks3d.MixedOp_conv(f["cin"], f["cout"], f["bias"])
        else:
            net = operations.OPS[f["kind"]](f["cin"], f["cout"], f["bias"])
            assert isinstance(net.op, nn.Conv3d) and (net.op.kernel_size[0], net.op.stride[0], net.op.padding[0]) == operations.CONV_KSP[f["kind"]]
        sd = net.state_dict()
        assert list(sd.keys()) == [str(k) for k in g[t + "keys"]]
        for (k, v), shp in zip(sd.items(), g[t + "shapes"]):
            assert list(v.shape) == [int(s) for s in shp[:v.dim()]], k
        net.load_state_dict(fixture_state_dict(f), strict=True)
        with pytest.raises(RuntimeError, match="MI355X"):
            net(fixture_input(f)) if f["kind"] != "mixed" else net(fixture_input(f), torch.ones(3) / 3)
    cell = networks3d.Cell_conv(8, 16, True, 3)
    assert sorted(cell.state_dict()) == sorted(f"_ops._ops.{j}.op.{p}" for j in range(3) for p in ("weight", "bias"))
    assert tuple(networks3d.conv_arch.shape) == (6, 3) and networks3d.conv_arch.requires_grad
    before = networks3d.conv_arch
    try:
        networks3d.conv_arch = torch.zeros(6, 3, requires_grad=True)
        assert len(networks3d.arch_parameters()) == 1 and networks3d.arch_parameters()[0] is networks3d.conv_arch
    finally:
        networks3d.conv_arch = before
    assert tuple(networks.conv_arch.shape) == (8, 3) and tuple(networks.upconv_arch.shape) == (8, 3) and len(networks.arch_parameters()) == 2
    assert set(operations.OPS) == {"re_conv_421", "re_conv_622", "re_conv_823", "conv_421", "conv_622", "conv_823"}
    assert isinstance(operations.OPS["re_conv_823"](8, 8, True).op, nn.ConvTranspose2d)
    up = networks3d.LinearAdditiveUpsample(2, 4, True)
    assert (up.scale_factor, up.n_splits, up.mode) == (2, 4, "trilinear") and not up.state_dict()
    with pytest.raises(RuntimeError, match="MI355X"):
        up(torch.zeros(1, 32, 2, 2, 2))


def test_cell3d_symbols_are_declared_bound_and_exported_with_abi_54():
    from semantic_segmentation_amd import _lib
    names = ["gs_cell3d_gather", "gs_cell3d_merge_pack", "gs_cell3d_split_wgrad_ws_floats", "gs_cell3d_split_wgrad",
             "gs_upsample_add3d_fwd", "gs_upsample_add3d_bwd"]
    hdr = open(os.path.join(ROOT, "include", "gsseg.h")).read()
    assert int(re.search(r"#define GS_ABI_VERSION (\d+)", hdr).group(1)) == 54 == _lib.ABI_VERSION
    assert int(re.search(r"#define GS_MAX_TAPS (\d+)", hdr).group(1)) == 64 == _lib.GS_MAX_TAPS
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.PROTOTYPES, n
    assert "GenSeg-3D/models/networks.py:570-601" in hdr and "networks.py:50-81" in hdr
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.gs_abi_version() == 54
    assert lib.gs_cell3d_split_wgrad_ws_floats(8, 8) == 3 * 8 and lib.gs_cell3d_split_wgrad_ws_floats(512, 520) == 3 * 520 * 32
    # refusals are synchronous and need no device: the checks come before any launch
    assert lib.gs_cell3d_gather(None, None, None, 1, 4, 4, 4, 8, 8, 0, 0, None) == -1 and b"gs_cell3d_gather" in lib.gs_last_error()
    assert lib.gs_upsample_add3d_fwd(4096, 8192, 1, 2, 2, 2, 16, 16, 0, 8, 0, 0, None) == -3 and b"multiple of 32" in lib.gs_last_error()
    assert lib.gs_cell3d_merge_pack(4096, 4096, 4096, 4096, 4096, None, 5, 8, 8, None, None, None, None, 0, None) == -3
    assert b"1..4" in lib.gs_last_error()
