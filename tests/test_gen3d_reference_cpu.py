"""CPU proofs for the 3-D Pix2Pix generator (tests/gen3d_reference.py, tests/golden/pix2pix3d_gen.npz):
  * the fp64 statement = torch.autograd through plain nn modules (our module tree walked with F.conv3d x 3 + softmax,
    F.interpolate + split / stack / sum, the norm modules themselves) = the fixture the reference's own classes made in double, at
    1e-9, d conv_arch and dx included; the tail statement = autograd through F.conv3d + tanh;
  * key set and 5-D shapes of our classes equal the fixture's; load_state_dict(strict=True);
  * define_G routing and every refusal that needs no device; the 2-D define_G('unet_128') still builds 7 downs of Conv2d;
  * on the GPU tests' seeds a right implementation (the statement with 16-bit stores, evaluated in fp32) passes the GPU bound and each
    stated mutant fails it."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from golden_util import grad_summary, tensor_checksum
from golden_util_gen3d import FIXTURES, fixture_arch, fixture_dense, fixture_input, fixture_state_dict, key_shapes, lattice
from tests import cell3d_reference as c3
from tests import gen3d_reference as g3

TOL = 1e-9
PARTS = FIXTURES["pix2pix3d_gen"]


def close(a, b, what):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    n = float(b.norm())
    err = float((a - b).norm()) / (n if n > 0 else 1.0)
    assert err <= TOL, f"{what}: relative error {err:.3e}"


def build(f):
    from semantic_segmentation_amd.models_pix2pix import networks, networks3d
    net = networks3d.UnetGenerator(f["input_nc"], f["output_nc"], f["num_downs"], f["ngf"],
                                   norm_layer=networks.get_norm_layer(f["norm"], threed=True), use_dropout=f["use_dropout"])
    net.load_state_dict(fixture_state_dict(f), strict=True)
    return net


def plain_forward(net, x, arch, masks=None):
    """the reference's forward over our module tree with plain torch ops; the in-place LeakyReLU / ReLU act as they do there: the
    skip operand of torch.cat is the LeakyReLU'd input"""
    mi = [0]

    def run(block, h):
        skip = None
        for m in block.model:
            n = type(m).__name__
            if n == "LeakyReLU":
                h = F.leaky_relu(h, 0.2)
                skip = h                                     # in place: x itself is now leaky(x)
            elif n == "ReLU":
                h = torch.relu(h)
            elif n == "Cell_conv":
                sm = torch.softmax(arch[m._layer_index], -1)
                h = sum(sm[j] * F.conv3d(h, o.op.weight, o.op.bias, stride=2, padding=p)
                        for j, (o, p) in enumerate(zip(m._ops._ops, (1, 2, 3))))
            elif n == "LinearUpsampleUnetSkipConnectionBlock":
                h = run(m, h)
            elif n == "LinearAdditiveUpsample":
                h = c3.torch_upsample(h)
            elif n == "Dropout":
                if net.training:
                    h = h * masks[mi[0]].to(h.dtype) * 2.0
                    mi[0] += 1
            else:                                            # Conv3d, BatchNorm3d, InstanceNorm3d, Tanh
                h = m(h)
        return h if block.outermost else torch.cat([skip, h], 1)
    return run(net.model, x)


def autograd_reference(f, masks=None):
    net = build(f).double()
    net.train(f["train"])
    arch = fixture_arch(f).requires_grad_(True)
    x = fixture_input(f).double().requires_grad_(True)
    y = plain_forward(net, x, arch, masks)
    (y * fixture_dense(f)).sum().backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in net.named_parameters()}
    return dict(y=y.detach(), dx=x.grad, darch=arch.grad, grads=grads), net


@pytest.mark.parametrize("i", range(len(PARTS)))
def test_statement_equals_autograd_and_fixture(i, golden_dir):
    f = PARTS[i]
    path = os.path.join(golden_dir, "pix2pix3d_gen.npz")
    assert os.path.getsize(path) < 1024 * 1024
    g = dict(np.load(path))
    t = f["tag"] + "/"
    ref, net = autograd_reference(f)
    # keys and 5-D shapes of our classes are the reference's
    assert list(net.state_dict().keys()) == [str(k) for k in g[t + "keys"]] == [k for k, _ in key_shapes(f)]
    shapes = [list(v.shape) + [0] * (5 - v.dim()) for v in net.state_dict().values()]
    assert shapes == g[t + "shapes"].tolist()
    for k, v in fixture_state_dict(f).items():
        if v.is_floating_point():
            assert np.array_equal(tensor_checksum(v), g[t + "wsum/" + k]), k
    st = g3.generator_statement(f, fixture_state_dict(f), fixture_arch(f), fixture_input(f), fixture_dense(f))
    for name, r in (("statement", st), ("autograd", ref)):
        close(lattice(r["y"], f), g[t + "y_lattice"], f"{name} image on the lattice")
        close(tensor_checksum(r["y"]), g[t + "ysum"], f"{name} image checksum")
        close(grad_summary(r["y"]), g[t + "gsum/y"], f"{name} image summary")
        close(grad_summary(r["dx"]), g[t + "gsum/dx"], f"{name} dx summary")
        close(r["darch"], g[t + "grad/arch"], f"{name} d conv_arch")
        for k, v in r["grads"].items():
            if v.dim() > 1:
                close(grad_summary(v), g[t + "gsum/" + k], f"{name} gradient summary {k}")
            elif float(np.abs(g[t + "grad/" + k]).max()) == 0.0 or "bias" in k and float(v.abs().max()) == 0.0:
                # cancelled by the norm behind it: the reference's autograd leaves roundoff (1e-17), the statement exact zeros
                assert float(np.abs(g[t + "grad/" + k]).max()) <= 1e-12 and float(v.abs().max()) <= 1e-12, k
            else:
                close(v, g[t + "grad/" + k], f"{name} gradient {k}")
    close(st["y"], ref["y"], "statement vs autograd image")
    close(st["dx"], ref["dx"], "statement vs autograd dx")
    close(st["darch"], ref["darch"], "statement vs autograd d conv_arch")
    for k, v in ref["grads"].items():
        if float(st["grads"][k].abs().max()) == 0.0:
            assert float(v.abs().max()) <= 1e-12, k
        else:
            close(st["grads"][k], v, f"statement vs autograd {k}")


def test_statement_equals_autograd_with_keep_masks():
    f, sd, arch, x, dense, masks = g3.case_inputs("bn6_drop_train")
    assert masks is not None and len(masks) == 1 and tuple(masks[0].shape) == (1, 128, 4, 4, 4)
    ref, _ = autograd_reference(f, masks)
    st = g3.flat(g3.generator_statement(f, sd, arch, x, dense, masks))
    got = g3.flat(ref)
    for k in st:
        if float(st[k].abs().max()) == 0.0:
            assert float(got[k].abs().max()) <= 1e-12, k
        else:
            close(st[k], got[k], k)


def test_tail_statement_equals_autograd():
    x, w, b, dout = g3.tail_tanh_inputs(g3.TAIL_CASES[2])
    xs, ws, bs = (t.double().requires_grad_(True) for t in (x, w, b))
    t = torch.tanh(F.conv3d(xs, ws, bs, padding=1))
    dx, dw, db = torch.autograd.grad(t, [xs, ws, bs], 4.0 * dout.double())
    r = g3.tail_statement(x, w, b, dout, gscale=4.0)
    for a, bb, what in ((r["t"], t.detach(), "t"), (r["dx"], dx, "dx"), (r["dw"], dw, "dw"), (r["db"], db, "db")):
        close(a, bb, what)
    base = {k: r[k] for k in ("dx", "dw", "db")}
    for m in g3.TAIL_MUTANTS:                                 # every tail mutant moves the forward or a gradient
        rm = g3.tail_statement(x, w, b, dout, gscale=4.0, mutant=m)
        moved = max(float((rm[k] - r[k]).norm() / r[k].norm()) for k in list(base) + ["t"])
        assert moved > 1e-3, (m, moved)
    for case in g3.TAIL_CASES:                                # the exact cases are exact: every statement value is an integer
        rr = g3.tail_build(case)
        for k in ("t", "dx", "dw", "db"):
            assert torch.equal(rr[k], rr[k].round()) and float(rr[k].abs().max()) < 2 ** 24


def test_define_g_routing_and_refusals():
    from semantic_segmentation_amd.models_pix2pix import create_model, networks, networks3d
    from semantic_segmentation_amd.models_pix2pix.generator3d_engine import Generator3DEngine
    net = networks.define_G(1, 1, 16, "unet_128", threed=True, upsampling="linear")
    assert isinstance(net, networks3d.UnetGenerator) and isinstance(net.engine, Generator3DEngine)
    assert len(net.engine.blocks()) == 6 and sum(isinstance(m, nn.Conv3d) for m in net.modules()) == 6 * 3 + 6
    assert sum(isinstance(m, nn.BatchNorm3d) for m in net.modules()) == 9
    assert [b.model[0 if b.outermost else 1]._layer_index for b in net.engine.blocks()] == [5, 4, 3, 2, 1, 0]
    inst = networks.define_G(2, 3, 32, "unet_128", norm="instance", use_dropout=True, threed=True, upsampling="linear")
    assert sum(isinstance(m, nn.InstanceNorm3d) for m in inst.modules()) == 9 and sum(isinstance(m, nn.Dropout) for m in inst.modules()) == 1
    assert len(inst.state_dict()) == 48                       # 6 cells x 3 kernels x (weight, bias) + 6 up-convs x 2
    for kw, pat in ((dict(netG="unet_256", upsampling="linear"), "6 rows"), (dict(netG="unet_128"), "upsampling='linear'"),
                    (dict(netG="resnet_9blocks", upsampling="linear"), "upsampling='linear'"),
                    (dict(netG="resnet_6blocks"), "upsampling='linear'")):
        with pytest.raises(NotImplementedError, match=pat):
            networks.define_G(1, 1, 16, kw.pop("netG"), threed=True, **kw)
    with pytest.raises(NotImplementedError, match="threed=True"):
        networks.define_G(1, 1, 64, "unet_128", upsampling="linear")
    # the 2-D behaviour does not move: 'unet_128' is 7 downs of Conv2d there
    g2 = networks.define_G(1, 1, 64, "unet_128")
    assert isinstance(g2, networks.UnetGenerator) and len(g2.engine.blocks()) == 7
    assert sum(isinstance(m, nn.Conv2d) for m in g2.modules()) == 7 and not any(isinstance(m, nn.Conv3d) for m in g2.modules())
    # construction limits
    bn = networks.get_norm_layer("batch", threed=True)
    for args in ((1, 1, 5, 24), (1, 1, 5, 8), (0, 1, 5, 16), (5, 1, 5, 16), (1, 5, 5, 16), (1, 1, 4, 16), (1, 1, 7, 16)):
        with pytest.raises(NotImplementedError, match="multiple of 16"):
            networks3d.UnetGenerator(*args, norm_layer=bn)
    with pytest.raises(NotImplementedError, match="upsampling='linear'"):
        networks3d.UnetGenerator(1, 1, 5, 16, norm_layer=bn, upsampling="deconvolution")
    for bad in (networks.get_norm_layer("batch"), networks.get_norm_layer("instance"), nn.GroupNorm,
                functools.partial(nn.InstanceNorm3d, affine=True, track_running_stats=False),
                functools.partial(nn.BatchNorm3d, affine=False, track_running_stats=True)):
        with pytest.raises(NotImplementedError):
            networks3d.UnetGenerator(1, 1, 5, 16, norm_layer=bad)
    g5 = networks3d.UnetGenerator(1, 1, 5, 16)
    with pytest.raises(ValueError, match="5|volume"):
        g5(torch.zeros(1, 1, 32, 32))
    with pytest.raises(ValueError, match="multiple of 32"):
        g5(torch.zeros(1, 1, 32, 48, 32))
    with pytest.raises(RuntimeError, match="MI355X only"):
        g5(torch.zeros(1, 1, 32, 32, 32))
    with pytest.raises(RuntimeError, match="UnetGenerator.forward"):
        g5.model(torch.zeros(1, 1, 32, 32, 32))
    with pytest.raises(NotImplementedError, match="pix2pix3d"):
        create_model(argparse.Namespace(model="pix2pix3d"))
    assert networks3d.arch_parameters()[0] is networks3d.conv_arch and tuple(networks3d.conv_arch.shape) == (6, 3)


# mutant -> the GPU case that shows it (the cheapest one where it can act)
MUTANT_CASE = {"no_up_relu": "bn5_train", "skip_leaky": "bn5_train", "halves_swapped": "bn5_train", "layer_index_outside": "bn5_train",
               "innermost_norm": "bn5_train", "tail_no_bias": "bn5_train", "no_tanh_grad": "bn5_train", "up_unflipped": "bn5_train",
               "tail_sample_leak": "bn5_train", "strided_groups": "bn5_train", "eval_c12": "bn5_eval", "keep_factor": "bn6_drop_train"}


@pytest.mark.parametrize("cid", ["bn5_train", "bn5_eval", "bn6_drop_train"])
def test_bound_passes_a_right_implementation(cid):
    """the statement with 16-bit stores evaluated in fp32 -- another valid rounding of the same plan -- is inside the GPU bound"""
    dt = g3.DT[g3.net_cases()[cid]["dtype"]]
    r64, r16 = g3.case_reference(cid), g3.case_reference(cid, store=dt)
    rep, bad = g3.gen_hold(g3.case_reference(cid, store=dt, dtype=torch.float32), r64, r16)
    k, w = g3.worst(rep)
    print(f"{cid}: right implementation worst {k} ratio {w['ratio']:.2f} rows {w.get('row_worst', 0.0):.2f}")
    assert not bad, (bad, {k: rep[k] for k in bad if k in rep})


@pytest.mark.parametrize("mutant", g3.GEN_MUTANTS)
def test_bound_rejects_mutant(mutant):
    cid = MUTANT_CASE[mutant]
    dt = g3.DT[g3.net_cases()[cid]["dtype"]]
    r64, r16 = g3.case_reference(cid), g3.case_reference(cid, store=dt)
    rep, bad = g3.gen_hold(g3.case_reference(cid, store=dt, mutant=mutant), r64, r16)
    print(f"{mutant} on {cid}: {len(bad)} tensors outside the bound, e.g. {bad[:4]}")
    assert bad, f"the bound does not see the mutant {mutant} on {cid}"
