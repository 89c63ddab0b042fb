"""The Pix2Pix engines under `--norm instance` held to the fp64 statement of tests/instnorm_reference.py, on the cases of
instnorm_reference.G_CASES / D_CASES (whose mutants tests/test_instnorm_reference_cpu.py proves the bounds catch):

  gradients  one forward with need_grad=True under torch.no_grad(), one direct backward on a fixed dense gradient; the saved state is
             adapted to the plain state, replayed in fp64 (R64) and with the engine's 16-bit stores (R16), and every parameter
             gradient, d arch and dx hold  err <= 4 * max(e16, FLOOR32 / 4) + d_U  (backward_replay.compare, rows included); the
             biases directly in front of a norm, whose gradient the engine returns as exact zeros, are held in absolute terms to
             2 u(dt) * sum |dy| of their stage (compare3d).
  forward    cases A and B (weights, image and arch of tests/golden/pix2pix_instance_{a,b}.npz, made by the reference in double):
             err(gpu) <= 4 * e16_fwd against the fixture's image / logits, e16_fwd the error of the fp64 forward with the engine's
             stores rounded (computed here); the measured ratio is printed.  (Fixture B's discriminator has six input channels,
             more than the engine's first-layer kernel takes; its logits are held on the CPU only.)
Generator cases run in train mode without dropout, in train mode with explicit keep masks and in eval mode (InstanceNorm takes
instance statistics in both; eval drops the masks).  About 2 to 6 s a case, nearly all of it the CPU replays."""
import os

import numpy as np
import pytest
import torch

from tests import instnorm_reference as ir

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(torch.get_num_threads(), 16))
# train, eval, and -- where the network has a dropout block (more than five downs) -- train with explicit keep masks
G_RUNS = [(cid, mode) for cid in sorted(ir.G_CASES) for mode in ("train", "train_dropout", "eval")
          if mode != "train_dropout" or ir.G_CASES[cid]["D"] > 5]


def load_golden(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name + ".npz")))


def hold(key, got, rp, dt):
    r64, r16, d_u, n_und, bias_scale = rp
    assert set(got) == set(r64), set(got) ^ set(r64)
    rep, bad = ir.hold(got, rp, dt)
    ir.record(key, rep, n_und)
    rel = {k: r for k, r in rep.items() if not r.get("absolute")}
    worst = max(rel, key=lambda k: rel[k]["ratio"])
    print(f"{key}: undecided {n_und}, worst {worst} ratio {rel[worst]['ratio']:.3g}, largest row_worst "
          f"{max(r['row_worst'] for r in rel.values()):.3g}, max d_U {max(d_u.values()):.3g}, cancelled biases worst "
          f"{max(r['ratio'] for r in rep.values() if r.get('absolute')):.3g} of their bound")
    for k in bias_scale:
        assert not bool(ir.d64(got[k]).any()), f"{k}: the gradient of a bias in front of a norm is exact zeros"
    for k in r64:
        if k not in bias_scale:
            assert d_u[k] <= max(rep[k]["e16"], ir.FLOOR32), f"{k}: d_U {d_u[k]:.3g} above e16 {rep[k]['e16']:.3g}: this case needs another seed"
    assert not bad, {k: rep[k] for k in bad}


@pytest.mark.parametrize("cid,mode", G_RUNS)
def test_generator(cid, mode, golden_dir):
    from semantic_segmentation_amd.models_pix2pix import networks, pix2pix_backward as pb
    c = ir.G_CASES[cid]
    dt = ir.TORCH_DT[c["dtype"]]
    dev = torch.device("cuda:0")
    sd, x, arch, dout, masks = ir.generator_case(c)
    train = mode != "eval"
    net = networks.UnetGenerator(c["cin"], c["cout"], c["D"], 64, norm_layer=networks.get_norm_layer("instance"), use_dropout=True,
                                 compute_dtype=c["dtype"])
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train(train)
    use_masks = mode == "train_dropout"
    masks = masks if use_masks else None
    if train and not use_masks:
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0                                    # train mode without dropout
    dmasks = [m.permute(0, 2, 3, 1).contiguous().to(torch.uint8).to(dev) for m in masks] if use_masks else None
    xd, archd = x.to(dev), arch.to(dev)
    eng = net.engine
    with torch.no_grad():
        out, ctx = eng.forward(xd, archd, train, True, dmasks)
        grads, darch, dx = pb.generator_backward(eng, ctx, archd, dout.float().to(dev), True)
    torch.cuda.synchronize()
    assert all(lv.get("inorm") is not None for lv in ctx["levels"][2:c["D"]]) and ctx["levels"][c["D"]].get("inorm") is None
    assert all(ctx["ups"][d].get("inorm") is not None for d in range(1, c["D"]))
    kept = [d for d in range(1, c["D"]) if ctx["ups"][d]["keep"] is not None]
    assert kept == ([d for d in range(1, c["D"]) if 1 <= c["D"] - 1 - d <= c["D"] - 5] if use_masks else [])
    assert set(grads) == set(sd) and not list(net.buffers())

    # ---- forward against the fixture
    if c["fixture"] and not use_masks:
        g = load_golden(golden_dir, c["fixture"])
        ref = torch.from_numpy(g["image" if train else "image_eval"])
        _, im16 = ir.generator_forward_state(sd, arch, x, None, c["D"], store=dt)
        e16, err = ir.rel_err(im16, ref), ir.rel_err(out.detach().cpu(), ref)
        print(f"instnorm_g/{cid}/{mode}: forward err {err:.3g} e16_fwd {e16:.3g} ratio {err / e16:.3g}")
        assert err <= 4 * e16, (err, e16)

    # ---- gradients against the replay of the engine's own state
    got = {k: v.detach().cpu() for k, v in grads.items()}
    got["darch"], got["dx"] = darch.detach().cpu(), dx.detach().cpu()
    state = ir.state_from_generator_ctx(eng, ctx, archd)
    hold(f"instnorm_g/{cid}/{mode}", got, ir.replays(state, ir.d64(dout), True, dt), dt)


@pytest.mark.parametrize("cid", sorted(ir.D_CASES))
def test_discriminator(cid, golden_dir):
    from semantic_segmentation_amd.models_pix2pix import networks
    c = ir.D_CASES[cid]
    dt = ir.TORCH_DT[c["dtype"]]
    golden = load_golden(golden_dir, c["fixture"]) if c["fixture"] else None
    sd, x = ir.discriminator_case(c, golden)
    net = networks.NLayerDiscriminator(c["cin"], 64, c["n_layers"], networks.get_norm_layer("instance"), compute_dtype=c["dtype"])
    net.load_state_dict(sd, strict=True)
    net = net.cuda().train()
    eng = net.engine
    xd = x.cuda()
    with torch.no_grad():
        logits, ctx = eng.forward(xd, True, True)
        ref64 = ir.discriminator_forward_state(sd, x)[1]
        dl = ir.dlogits_of(ref64, c["seed"])
        grads, dx = eng.backward(ctx, dl.float().cuda(), True)
    torch.cuda.synchronize()
    assert [r["kind"] for r in ctx["recs"]] == ["first"] + ["mid"] * c["n_layers"] + ["last"]
    assert all(r.get("inorm") is not None for r in ctx["recs"][1:-1]) and set(grads) == set(sd)
    if golden is not None:
        ref = torch.from_numpy(golden["logits_fake"])
        _, l16 = ir.discriminator_forward_state(sd, x, store=dt)
        e16, err = ir.rel_err(l16, ref), ir.rel_err(logits.detach().cpu(), ref)
        print(f"instnorm_d/{cid}: forward err {err:.3g} e16_fwd {e16:.3g} ratio {err / e16:.3g}")
        assert err <= 4 * e16, (err, e16)
    got = {k: v.detach().cpu() for k, v in grads.items()}
    got["dx"] = dx.detach().cpu()
    state = ir.state_from_discriminator_ctx(eng, ctx)
    hold(f"instnorm_d/{cid}", got, ir.replays(state, dl, True, dt), dt)


def test_eval_and_train_give_the_same_image_and_autograd_reaches_every_parameter(monkeypatch):
    """the public path: G(x) in train (dropout p = 0) and eval mode are bit-equal, and backward() through autograd fills every
    parameter, the architecture tensor and x"""
    from semantic_segmentation_amd.models_pix2pix import networks
    c = ir.G_CASES["g5_32"]
    sd, x, arch, dout, _ = ir.generator_case(c)
    net = networks.UnetGenerator(1, 1, 5, 64, norm_layer=networks.get_norm_layer("instance"), use_dropout=True)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    arch_leaf = arch.cuda().requires_grad_(True)
    monkeypatch.setattr(networks, "upconv_arch", arch_leaf)
    xl = x.cuda().requires_grad_(True)
    out = net.train()(xl)
    (out * dout.float().cuda()).sum().backward()
    with torch.no_grad():
        assert torch.equal(net.eval()(x.cuda()), out.detach())
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert arch_leaf.grad is not None and xl.grad is not None and float(xl.grad.abs().sum()) > 0
    nm = ir.block_names(5)
    cancelled = [nm[d]["conv"] + ".bias" for d in range(1, 4)] + [f"{nm[d]['cell']}._ops._ops.{j}.op.bias" for d in range(1, 5) for j in range(3)]
    params = dict(net.named_parameters())
    assert all(not bool(params[n].grad.any()) for n in cancelled), "biases in front of a norm: exact zeros"
    assert all(bool(p.grad.any()) for n, p in params.items() if n not in cancelled)


def test_one_element_plane_raises_before_any_launch():
    from semantic_segmentation_amd.models_pix2pix import networks
    net = networks.NLayerDiscriminator(2, 64, 3, networks.get_norm_layer("instance")).cuda()
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        net(torch.zeros(1, 2, 16, 16, device="cuda"))
    assert net(torch.zeros(1, 2, 32, 32, device="cuda")).shape == (1, 1, 2, 2)


def test_create_model_with_instance_norm_takes_a_step(tmp_path):
    """create_model(opt) with opt.norm = 'instance' (the default of --norm): one optimize_parameters() updates G and D"""
    import argparse
    from semantic_segmentation_amd.models_pix2pix import create_model
    opt = argparse.Namespace(model="pix2pix", input_nc=1, output_nc=1, ngf=64, ndf=64, netG="unet_128", netD="basic", n_layers_D=3,
                             norm="instance", no_dropout=False, init_type="normal", init_gain=0.02, gpu_ids=[0], cuda_index=0,
                             isTrain=True, gan_mode="vanilla", lr=2e-4, beta1=0.5, arch_lr=3e-4, lambda_L1=100.0, lr_policy="linear",
                             n_epochs=2, n_epochs_decay=2, epoch_count=1, checkpoints_dir=str(tmp_path), name="p2p_in",
                             continue_train=False, verbose=False)
    torch.manual_seed(3)
    model = create_model(opt)
    model.setup(opt)
    assert any(k.endswith(".bias") for k in model.netD.state_dict()) and not list(model.netG.buffers())
    g = torch.Generator().manual_seed(1)
    model.set_input(torch.rand((2, 1, 128, 128), generator=g) * 2 - 1, (torch.rand((2, 1, 128, 128), generator=g) > 0.5).float())
    before = [[p.detach().clone() for p in net.parameters()] for net in (model.netG, model.netD)]
    model.optimize_parameters()
    torch.cuda.synchronize()
    for net, old in zip((model.netG, model.netD), before):
        assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
        assert any(not torch.equal(a, b) for a, b in zip(old, net.parameters()))
    losses = model.get_current_losses()
    assert set(losses) == {"G_GAN", "G_L1", "D_real", "D_fake"} and all(v == v and abs(v) < 1e4 for v in losses.values())
