"""The 3-D Pix2Pix generator's two operators behind the reference's module classes (models_pix2pix/networks3d.py: Cell_conv, MixedOp_conv,
LinearAdditiveUpsample; architecture_pix2pix/operations.py: conv_421 / 622 / 823) on the HIP path (GPU only), held to the project's bound
against the fp64 statement (tests/cell3d_reference.py) and the fixture the reference's own classes made (tests/golden/pix2pix3d_cells.npz):
    the forward and every gradient (dx, the six parameter tensors, the conv_arch row):  err <= 4 max(e16, FLOOR32), per tensor and per
    output-channel row (backward_replay.compare; d_U = 0: there is no activation)
with e16 the same statement with the engine's 16-bit stores rounded (source, packs, output, dy, dx).  tests/test_cell3d_reference_cpu.py
proves on these seeds that the bound tells the stated wrong implementations from a right one.  None of the modules exists without the feature."""
import os

import numpy as np
import pytest
import torch

from golden_util import grad_summary
from golden_util_cell3d import FIXTURES, fixture_arch, fixture_input, fixture_state_dict
from tests import cell3d_reference as c3
from tests.backward_replay import FLOOR32
from tests.disc3d_reference import summary_failures

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(torch.get_num_threads(), 16))


def set_dtype(monkeypatch, dtn):
    """the stand-alone modules run in the process-wide compute dtype (GSSEG_DTYPE, read per call)"""
    monkeypatch.setenv("GSSEG_DTYPE", dtn)


def report(key, rep, bad):
    worst = max(rep, key=lambda k: rep[k]["ratio"])
    print(f"{key}: worst {worst} err {rep[worst]['err']:.3g} e16 {rep[worst]['e16']:.3g} ratio {rep[worst]['ratio']:.3g}; "
          + ", ".join(f"{k} {v['ratio']:.2f}" for k, v in sorted(rep.items())))
    assert not bad, {k: rep[k] for k in bad}


def build_module(kind, cin, cout, bias, layer=c3.LAYER_INDEX):
    from semantic_segmentation_amd.architecture_pix2pix.operations import OPS
    from semantic_segmentation_amd.models_pix2pix import networks3d
    if kind == "cell":
        return networks3d.Cell_conv(cin, cout, bias, layer)
    if kind == "mixed":
        return networks3d.MixedOp_conv(cin, cout, bias)
    return OPS[{"k4": "conv_421", "k6": "conv_622", "k8": "conv_823"}.get(kind, kind)](cin, cout, bias)


def state_dict_of(kind, ws, bs):
    pre = {"cell": "_ops._ops.%d.", "mixed": "_ops.%d."}.get(kind)
    sd = {}
    for j, k in enumerate(c3.KS):
        if pre is None and kind != f"k{k}":
            continue
        p = pre % j if pre else ""
        sd[p + "op.weight"] = ws[j]
        if bs is not None:
            sd[p + "op.bias"] = bs[j]
    return sd


def run_module(net, kind, x, arch, dy, layer=c3.LAYER_INDEX):
    """forward + backward of a module on the device -> dict of CPU tensors named as cell3d_reference.module_reference names them"""
    from semantic_segmentation_amd.models_pix2pix import networks3d
    net = net.cuda()
    for p in net.parameters():
        p.grad = None
    xd = x.cuda().requires_grad_(True)
    leaf = None
    if kind == "cell":
        leaf = networks3d.conv_arch = arch.float().cuda().requires_grad_(True)          # rebinding: the next forward must see it
        y = net(xd)
    elif kind == "mixed":
        leaf = torch.softmax(arch[layer], -1).float().cuda().requires_grad_(True)
        y = net(xd, leaf)
    else:
        y = net(xd)
    y.backward(dy.float().cuda())
    torch.cuda.synchronize()
    got = {"y": y.detach().cpu(), "dx": xd.grad.cpu()}
    for name, p in net.named_parameters():
        k = int(p.shape[2]) if p.dim() == 5 else None
        if k is None:                                        # a bias: its kernel size from the sibling weight
            k = int(dict(net.named_parameters())[name[:-4] + "weight"].shape[2])
        got[("dw%d" if p.dim() == 5 else "db%d") % k] = p.grad.cpu()
    if kind == "cell":
        g = leaf.grad.cpu()
        assert not bool(g[[i for i in range(6) if i != layer]].any()), "rows of conv_arch the cell does not read got a gradient"
        got["darch"] = g[layer]
    elif kind == "mixed":
        got["dsm"] = leaf.grad.cpu()
    return got


@pytest.mark.parametrize("cid", sorted(c3.MODULE_CASES))
def test_cell_modules_hold_the_bound(cid, monkeypatch):
    Cin, Cout, bias, N, vol, dtn, kind = c3.MODULE_CASES[cid]
    set_dtype(monkeypatch, dtn)
    x, ws, bs, arch, dy = c3.module_inputs(cid)
    net = build_module(kind, Cin, Cout, bias)
    net.load_state_dict(state_dict_of(kind, ws, bs), strict=True)
    got = run_module(net, kind, x, arch, dy)
    r64, r16 = c3.module_reference(cid), c3.module_reference(cid, store=c3.DT[dtn])
    assert set(got) == set(r64), set(got) ^ set(r64)
    assert got["y"].shape == (N, Cout, vol[0] // 2, vol[1] // 2, vol[2] // 2) and got["dx"].shape == x.shape
    rep, bad = c3.hold(got, r64, r16)
    report(cid, rep, bad)
    again = run_module(net, kind, x, arch, dy)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"


@pytest.mark.parametrize("cid", sorted(c3.UP_MODULE_CASES))
def test_upsample_module_holds_the_bound(cid, monkeypatch):
    from semantic_segmentation_amd.models_pix2pix import networks3d
    C, N, vol, dtn = c3.UP_MODULE_CASES[cid]
    set_dtype(monkeypatch, dtn)
    x, dy = c3.up_module_inputs(cid)
    net = networks3d.LinearAdditiveUpsample(2, 4, True)
    assert net.mode == "trilinear" and not list(net.parameters())
    runs = []
    for _ in range(2):
        xd = x.cuda().requires_grad_(True)
        y = net(xd)
        y.backward(dy.float().cuda())
        runs.append({"y": y.detach().cpu(), "dx": xd.grad.cpu()})
    got = runs[0]
    assert got["y"].shape == (N, C // 4, 2 * vol[0], 2 * vol[1], 2 * vol[2])
    rep, bad = c3.hold(got, c3.up_module_reference(cid), c3.up_module_reference(cid, store=c3.DT[dtn]))
    report(cid, rep, bad)
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in got), "two runs differ"


def test_fixture_of_the_reference(golden_dir, monkeypatch):
    """tests/golden/pix2pix3d_cells.npz (the reference's own classes in double): load_state_dict(strict=True) from the fixture's weights,
    the output and every gradient of sum(y * dense) within 4 max(e16, FLOOR32) of the fp64 statement (whose values equal the stored ones
    at 1e-9, tests/test_cell3d_reference_cpu.py), and against the STORED values themselves: y, the biases' and conv_arch's gradients in
    full, dx and the weights' as summaries (disc3d_reference.summary_failures)."""
    from semantic_segmentation_amd.models_pix2pix import networks3d
    g = dict(np.load(os.path.join(golden_dir, "pix2pix3d_cells.npz")))
    set_dtype(monkeypatch, "f16")
    dt = torch.float16
    for f in FIXTURES["pix2pix3d_cells"]:
        t = f["tag"] + "/"
        x = fixture_input(f)
        assert np.array_equal(g[t + "input"], x.numpy())
        dense = torch.from_numpy(g[t + "dense"])
        if f["kind"] == "up":
            xd = x.cuda().requires_grad_(True)
            y = networks3d.LinearAdditiveUpsample(2, 4, True)(xd)
            y.backward(dense.float().cuda())
            got = {"y": y.detach().cpu(), "dx": xd.grad.cpu()}
            r64, r16 = c3.upsample_statement(x, dense), c3.upsample_statement(x, dense, store=dt)
            stored_full = {}
        else:
            sd, arch = fixture_state_dict(f), fixture_arch(f)
            kind = f["kind"]
            net = build_module(kind, f["cin"], f["cout"], f["bias"], f["layer"])
            assert list(net.state_dict().keys()) == [str(k) for k in g[t + "keys"]]
            net.load_state_dict(sd, strict=True)
            mk = {"conv_421": "k4", "conv_622": "k6", "conv_823": "k8"}.get(kind, kind)
            got = run_module(net, mk, x, arch, dense, f["layer"])
            ws = [sd.get(k) for k in sorted(sd) if k.endswith("weight")]
            bs = [sd.get(k) for k in sorted(sd) if k.endswith("bias")] or None
            if kind in ("cell", "mixed"):
                sm = torch.softmax(arch[f["layer"]], -1)
            else:                                            # one primitive: the other two kernels are zeros with weight zero
                k0 = int(kind[5])
                w1, b1 = ws[0], (bs[0] if bs else None)
                ws = [w1 if k == k0 else torch.zeros((f["cout"], f["cin"], k, k, k)) for k in c3.KS]
                bs = None if b1 is None else [b1 if k == k0 else torch.zeros(f["cout"]) for k in c3.KS]
                sm = torch.tensor([float(k == k0) for k in c3.KS], dtype=torch.float64)
            r64, r16 = (c3.cell_statement(x, ws, bs, sm, dense, store=s) for s in (None, dt))
            for r in (r64, r16):
                r.pop("dwm")
                dsm = r.pop("dsm")
                if kind == "cell":
                    r["darch"] = c3.softmax_row_grad(arch[f["layer"]], dsm)
                elif kind == "mixed":
                    r["dsm"] = dsm
                for k in [k for k in r if k not in got]:
                    r.pop(k)
            names = dict(net.named_parameters())
            stored_full = {("db%d" % names[n[:-4] + "weight"].shape[2]): g[t + "grad/" + n] for n in names if n.endswith("bias")}
            if kind == "cell":
                stored_full["darch"] = g[t + "grad/arch"][f["layer"]]
            for n, p in names.items():
                if p.dim() == 5:
                    k = "dw%d" % p.shape[2]
                    e16 = float((r16[k] - r64[k]).norm() / r64[k].norm())
                    fails, shares = summary_failures(grad_summary(got[k]), g[t + "gsum/" + n], got[k].numel(), e16)
                    assert not fails, (t, n, shares)
        assert set(got) == set(r64), (t, set(got) ^ set(r64))
        rep, bad = c3.hold(got, r64, r16)
        report(t, rep, bad)
        ref_y = torch.from_numpy(g[t + "y"])
        e16 = float((r16["y"] - r64["y"]).norm() / r64["y"].norm())
        assert float((got["y"].double() - ref_y).norm() / ref_y.norm()) <= 4 * max(e16, FLOOR32)
        e16 = float((r16["dx"] - r64["dx"]).norm() / r64["dx"].norm())
        fails, shares = summary_failures(grad_summary(got["dx"]), g[t + "gsum/dx"], got["dx"].numel(), e16)
        assert not fails, (t, "dx", shares)
        for k, ref in stored_full.items():
            ref = torch.from_numpy(np.asarray(ref)).double()
            e16 = float((r16[k] - r64[k]).norm() / r64[k].norm())
            assert float((got[k].double() - ref).norm() / ref.norm()) <= 4 * max(e16, FLOOR32 / 4), (t, k)


def test_rebinding_conv_arch_is_seen_by_the_next_forward(monkeypatch):
    """Cell_conv.forward reads the tensor networks3d.conv_arch is bound to NOW, and arch_parameters() returns that tensor"""
    from semantic_segmentation_amd.models_pix2pix import networks3d
    set_dtype(monkeypatch, "f16")
    cid = "cell_c16_bf16"
    Cin, Cout, bias, N, vol, _, kind = c3.MODULE_CASES[cid]
    x, ws, bs, arch, dy = c3.module_inputs(cid)
    net = build_module(kind, Cin, Cout, bias)
    net.load_state_dict(state_dict_of(kind, ws, bs), strict=True)
    net = net.cuda()
    outs = []
    for row in ([8.0, 0.0, 0.0], [0.0, 0.0, 8.0]):
        a = torch.zeros(6, 3)
        a[c3.LAYER_INDEX] = torch.tensor(row)
        networks3d.conv_arch = a.cuda().requires_grad_(True)
        assert networks3d.arch_parameters()[0] is networks3d.conv_arch and len(networks3d.arch_parameters()) == 1
        with torch.no_grad():
            outs.append(net(x.cuda()).cpu().double())
        want = c3.cell_statement(x, ws, bs, torch.softmax(a[c3.LAYER_INDEX].double(), -1))["y"]
        assert float((outs[-1] - want).norm() / want.norm()) < 4e-3
    assert float((outs[0] - outs[1]).norm() / outs[0].norm()) > 0.5


def test_refusals_name_the_limits():
    from semantic_segmentation_amd.architecture_pix2pix.operations import conv_823
    from semantic_segmentation_amd.models_pix2pix import networks3d
    dev = torch.device("cuda:0")
    with pytest.raises(NotImplementedError, match=r"1\.\.4.*multiple of 8"):
        networks3d.Cell_conv(12, 16, True, 0).cuda()(torch.zeros(1, 12, 4, 4, 4, device=dev))
    with pytest.raises(NotImplementedError, match="C_out a multiple of 8"):
        networks3d.MixedOp_conv(8, 12, True).cuda()(torch.zeros(1, 8, 4, 4, 4, device=dev), torch.ones(3, device=dev) / 3)
    with pytest.raises(NotImplementedError, match=">= 2"):
        conv_823(8, 8, False).cuda()(torch.zeros(1, 8, 1, 4, 4, device=dev))
    up = networks3d.LinearAdditiveUpsample
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        up(2, 4, True)(torch.zeros(1, 16, 2, 2, 2, device=dev))
    with pytest.raises(NotImplementedError, match="n_splits == 4"):
        up(2, 2, True)(torch.zeros(1, 32, 2, 2, 2, device=dev))
    with pytest.raises(NotImplementedError, match="scale_factor == 2"):
        up(4, 4, True)(torch.zeros(1, 32, 2, 2, 2, device=dev))
    with pytest.raises(NotImplementedError, match="threed=True"):
        up(2, 4, False)(torch.zeros(1, 32, 1, 2, 2, device=dev))
    with pytest.raises(RuntimeError, match="MI355X"):
        networks3d.Cell_conv(8, 8, True, 0)(torch.zeros(1, 8, 4, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X"):
        up(2, 4, True)(torch.zeros(1, 32, 2, 2, 2))
