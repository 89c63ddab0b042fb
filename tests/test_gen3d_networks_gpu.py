"""The 3-D Pix2Pix generator (networks3d.UnetGenerator on Generator3DEngine) against the fp64 statement (tests/gen3d_reference.py) and
the fixture the reference's own classes made (tests/golden/pix2pix3d_gen.npz): the three fixture networks (BatchNorm3d in train and
eval mode, InstanceNorm3d, six downs with dropout blocks in eval mode), one bf16 case and one train-mode dropout case with given
keep masks.  The image, every parameter gradient, the conv_arch gradient and dx within the project's bound of the statement, per
tensor and per output-channel row: 4 max(e16, FLOOR32) for the image, 4 max(e16, FLOOR32 / 4) for the gradients
(cell3d_reference.hold over backward_replay.compare), with d_U = 0; biases cancelled by a norm get exact zeros.  Also: two runs
bit-equal, the skipped outermost data gradient, the pack cache, running statistics in eval mode, a Pix2Pix step with the 3-D
discriminators, the refusals (GPU only)."""
import argparse
import os

import numpy as np
import pytest
import torch

from golden_util_gen3d import lattice
from tests import cell3d_reference as c3
from tests import gen3d_reference as g3
from tests.backward_replay import FLOOR32

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(torch.get_num_threads(), 16))

WORST = {}


def build(f, dtn):
    from semantic_segmentation_amd.models_pix2pix import networks, networks3d
    net = networks3d.UnetGenerator(f["input_nc"], f["output_nc"], f["num_downs"], f["ngf"],
                                   norm_layer=networks.get_norm_layer(f["norm"], threed=True), use_dropout=f["use_dropout"],
                                   compute_dtype=dtn)
    return net


def run_case(cid, x_grad=True, net=None):
    """forward + backward of a case on the device -> (flat dict of CPU tensors named as gen3d_reference.flat names them, net)"""
    from semantic_segmentation_amd.models_pix2pix import networks3d
    f, sd, arch, x, dense, masks = g3.case_inputs(cid)
    if net is None:
        net = build(f, f["dtype"])
        net.load_state_dict(sd, strict=True)
        net = net.cuda()
    net.train(f["train"])
    for p in net.parameters():
        p.grad = None
    leaf = networks3d.conv_arch = arch.float().cuda().requires_grad_(True)      # rebinding: the next forward must see it
    xd = x.cuda().requires_grad_(x_grad)
    dm = None if masks is None else [c3.slices(m).cuda() for m in masks]
    y = net(xd, dropout_masks=dm)
    y.backward(dense.float().cuda())
    torch.cuda.synchronize()
    got = {"y": y.detach().cpu(), "darch": leaf.grad.cpu()}
    if x_grad:
        got["dx"] = xd.grad.cpu()
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        got["g/" + k] = p.grad.cpu()
    return got, net


@pytest.mark.parametrize("cid", g3.NET_CASE_IDS)
def test_network_holds_the_bound(cid, golden_dir):
    f = g3.net_cases()[cid]
    dt = g3.DT[f["dtype"]]
    got, net = run_case(cid)
    r64, r16 = g3.case_reference(cid), g3.case_reference(cid, store=dt)
    assert set(got) == set(r64), set(got) ^ set(r64)
    assert got["y"].shape == (f["N"], f["output_nc"], f["D"], f["H"], f["W"]) and got["dx"].shape[1] == f["input_nc"]
    rep, bad = g3.gen_hold(got, r64, r16)
    k, w = g3.worst(rep)
    WORST[cid] = (k, w["ratio"], w.get("row_worst", 0.0))
    print(f"{cid}: image err {rep['y']['err']:.3g} e16 {rep['y']['e16']:.3g} ratio {rep['y']['ratio']:.2f}; worst gradient {k} "
          f"err {w['err']:.3g} e16 {w['e16']:.3g} ratio {w['ratio']:.2f} rows {w.get('row_worst', 0.0):.2f}; "
          f"dx {rep['dx']['ratio']:.2f} darch {rep['darch']['ratio']:.2f}")
    assert not bad, (bad, {n: rep[n] for n in bad if n in rep})
    unused = [i for i in range(6) if i >= f["num_downs"]]
    assert not bool(got["darch"][unused].any()), "rows of conv_arch no cell reads got a gradient"
    # two runs are bit-equal
    again, _ = run_case(cid, net=net)
    for n in got:
        assert torch.equal(got[n], again[n]), f"{n}: two runs differ"
    # x.requires_grad=False skips the outermost cell's data gradient: the same parameter gradients bit for bit
    nodx, _ = run_case(cid, x_grad=False, net=net)
    assert "dx" not in nodx
    for n in nodx:
        assert torch.equal(got[n], nodx[n]), f"{n}: differs without the input gradient"
    # the fixture the reference's own classes made in double: the image, the biases / norm parameters and the conv_arch gradient
    tag = f["tag"] + "/"
    g = dict(np.load(os.path.join(golden_dir, "pix2pix3d_gen.npz")))
    if tag + "y_lattice" in g:
        fix = {"y": torch.from_numpy(g[tag + "y_lattice"]), "darch": torch.from_numpy(g[tag + "grad/arch"])}
        sub = {"y": lattice(got["y"], f), "darch": got["darch"]}
        s64, s16 = {"y": lattice(r64["y"], f), "darch": r64["darch"]}, {"y": lattice(r16["y"], f), "darch": r16["darch"]}
        for n in r64:
            if n.startswith("g/") and r64[n].dim() == 1 and float(r64[n].abs().max()) > 0:
                fix[n] = torch.from_numpy(g[tag + "grad/" + n[2:]])
                sub[n], s64[n], s16[n] = got[n], r64[n], r16[n]
        for n in fix:                                         # (the statement equals the fixture at 1e-9: the CPU file)
            assert float((fix[n] - s64[n]).norm()) <= 1e-9 * float(s64[n].norm()), n
        rep2, bad2 = c3.hold(sub, fix, s16)
        print(f"{cid} against the fixture: image ratio {rep2['y']['ratio']:.2f}, worst of {len(fix) - 1} gradients "
              f"{max(v['ratio'] for n, v in rep2.items() if n != 'y'):.2f}")
        assert not bad2, bad2


def test_eval_uses_running_statistics():
    """eval mode reads running_mean / running_var (the bn5_eval case holds the bound against a statement that does); a train-mode
    forward moves them and the counters, an eval forward does not"""
    got, net = run_case("bn5_eval")
    bufs = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    f, sd, arch, x, dense, masks = g3.case_inputs("bn5_eval")
    with torch.no_grad():
        y_eval = net(x.cuda())
    for k, v in net.state_dict().items():
        if k in bufs:
            assert torch.equal(v, bufs[k]), k
    net.train()
    with torch.no_grad():
        y_train = net(x.cuda())
    assert not torch.equal(y_eval, y_train)
    moved = [k for k, v in net.state_dict().items() if k in bufs and not torch.equal(v, bufs[k])]
    assert len(moved) == len(bufs), set(bufs) - set(moved)
    assert all(int(v) == 4 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked"))


def test_pack_cache_follows_weights_and_arch():
    """forwards without a graph reuse the merged packs; after an in-place weight update, an in-place edit of a conv_arch row and a
    rebinding of networks3d.conv_arch the next forward follows: the image matches the statement each time"""
    from golden_util_gen3d import block_prefix
    from semantic_segmentation_amd.models_pix2pix import networks3d
    f, sd, arch, x, dense, masks = g3.case_inputs("bn5_eval")
    net = build(f, "f16")
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    xd = x.cuda()

    def check(sd_now, arch_now, what):
        with torch.no_grad():
            y = net(xd).cpu().double()
        r64 = g3.generator_statement(f, sd_now, arch_now, x)["y"]
        r16 = g3.generator_statement(f, sd_now, arch_now, x, store=torch.float16)["y"]
        err, e16 = float((y - r64).norm() / r64.norm()), float((r16 - r64).norm() / r64.norm())
        print(f"pack cache, {what}: err {err:.3g} e16 {e16:.3g}")
        assert err <= 4 * max(e16, FLOOR32), what
        return y

    networks3d.conv_arch = arch.float().cuda()
    y0 = check(sd, arch, "first forward")
    with torch.no_grad():
        assert torch.equal(net(xd).cpu().double(), y0)                          # cached packs: the same image
    key = block_prefix(2) + "1._ops._ops.2.op.weight"
    with torch.no_grad():
        dict(net.named_parameters())[key].mul_(1.5)
    sd1 = dict(sd)
    sd1[key] = sd[key] * 1.5
    y1 = check(sd1, arch, "after an in-place weight update")
    assert not torch.equal(y1, y0)
    with torch.no_grad():
        networks3d.conv_arch[2] += torch.tensor([1.0, -1.0, 0.5], device="cuda")
    arch2 = arch.clone()
    arch2[2] += torch.tensor([1.0, -1.0, 0.5], dtype=arch.dtype)
    y2 = check(sd1, arch2, "after an in-place conv_arch edit")
    assert not torch.equal(y2, y1)
    arch3 = torch.flip(arch2, dims=(0,)).contiguous()
    networks3d.conv_arch = arch3.float().cuda()
    y3 = check(sd1, arch3, "after rebinding conv_arch")
    assert not torch.equal(y3, y2)


@pytest.mark.parametrize("netD", ["basic", "pixel"])
def test_pix2pix_step_with_3d_discriminators(netD):
    """steps.generator_step_loss / discriminator_step_loss with this generator and the 3-D discriminators take a step: every
    parameter of G gets a finite gradient, non-zero exactly where a following norm does not cancel it; G gets none in the D step"""
    from semantic_segmentation_amd import steps
    from semantic_segmentation_amd.models_pix2pix import networks, networks3d
    torch.manual_seed(5)
    netG = networks.define_G(1, 1, 16, "unet_128", norm="batch", threed=True, upsampling="linear", init_gain=0.2).cuda()
    netD = networks.define_D(2, 16, netD, n_layers_D=2, norm="batch", threed=True, init_gain=0.2).cuda()
    networks3d.conv_arch = (0.5 * torch.randn(6, 3)).cuda().requires_grad_(True)
    crit = networks.GANLoss("vanilla").cuda()
    mask, image = torch.randn(1, 1, 64, 64, 64, device="cuda"), torch.rand(1, 1, 64, 64, 64, device="cuda") * 2 - 1
    loss = steps.generator_step_loss(netG, netD, crit, mask, image)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    for k, p in netG.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        cancelled = k.endswith(".bias") and p.dim() == 1 and k.rsplit(".", 2)[-2] in ("4", "6") and not k.startswith("model.model.4")
        assert bool(p.grad.any()) != cancelled, (k, "cancelled by the norm behind it" if cancelled else "must be non-zero")
    assert networks3d.conv_arch.grad is not None and bool(networks3d.conv_arch.grad.any())
    for p in list(netG.parameters()) + list(netD.parameters()):
        p.grad = None
    lossD = steps.discriminator_step_loss(netG, netD, crit, mask, image)
    lossD.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lossD))
    assert all(p.grad is None for p in netG.parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in netD.parameters())


def test_refusals_on_the_device():
    from semantic_segmentation_amd.models_pix2pix import create_model, networks3d
    net = networks3d.UnetGenerator(1, 1, 5, 16).cuda()
    with pytest.raises(ValueError, match="volume"):
        net(torch.zeros(1, 1, 32, 32, device="cuda"))
    with pytest.raises(ValueError, match="multiple of 32"):
        net(torch.zeros(1, 1, 32, 32, 48, device="cuda"))
    with pytest.raises(RuntimeError, match="MI355X only"):
        net(torch.zeros(1, 1, 32, 32, 32))
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        networks3d.UnetGenerator(1, 1, 5, 40)
    with pytest.raises(NotImplementedError):
        create_model(argparse.Namespace(model="pix2pix3d"))
    assert net(torch.zeros(1, 1, 32, 32, 32, device="cuda")).shape == (1, 1, 32, 32, 32)


def test_zz_report_worst_ratios():
    """(prints what DESIGN.md quotes; runs last in this file)"""
    for cid, (k, ratio, rows) in WORST.items():
        print(f"{cid}: worst {k} ratio {ratio:.2f} (bound 4) rows {rows:.2f} (bound 1)")
