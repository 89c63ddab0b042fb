"""The fp64 statement of the ResNet generator (tests/resnet_reference.py) is the reference's, its hand-derived backward is
torch.autograd, and the bounds the GPU tests put on the engine tell a right implementation from each stated wrong one -- on the
seeds the GPU tests use.  No GPU, no library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import grad_summary, tensor_checksum
from golden_util_resnet import FIXTURES, fixture_inputs, fixture_loss, fixture_state_dict
from tests import resnet_reference as rr

torch.set_num_threads(8)


@pytest.fixture(scope="module", params=sorted(FIXTURES))
def fx(request, golden_dir):
    f = FIXTURES[request.param]
    g = np.load(f"{golden_dir}/{request.param}.npz")
    sd = fixture_state_dict(f)
    x, real, dense = fixture_inputs(f)
    cfg = dict(n_blocks=f["n_blocks"], norm=f["norm"], use_dropout=f["use_dropout"])
    return dict(f=f, g=g, sd=sd, x=x, real=real, dense=dense, cfg=cfg)


def test_fixture_inputs_and_weights_are_the_seeded_ones(fx):
    g = fx["g"]
    assert np.array_equal(g["input"], fx["x"].double().numpy())
    keys = {k[5:] for k in g.files if k.startswith("wsum/")}
    assert keys == set(fx["sd"])
    for k, v in fx["sd"].items():
        assert np.array_equal(g["wsum/" + k], tensor_checksum(v)), k


def test_forward_is_the_reference(fx):
    for train, key in ((True, "image"), (False, "image_eval")):
        _, im = rr.forward_state(fx["sd"], fx["cfg"], fx["x"], train)
        assert float((im - torch.from_numpy(fx["g"][key])).abs().max()) <= 1e-9, key


def test_gradient_summaries_are_the_reference(fx):
    g = fx["g"]
    st, im = rr.forward_state(fx["sd"], fx["cfg"], fx["x"], True)
    im = im.detach().requires_grad_(True)
    loss = fixture_loss(im, fx["real"].double(), fx["dense"].double())
    assert abs(loss.item() - float(g["loss"])) <= 1e-9 * abs(float(g["loss"]))
    loss.backward()
    grads, dx, bias_scale = rr.replay(st, im.grad, True)
    grads = dict(grads, dx=dx)
    names = {k[5:] for k in g.files if k.startswith("gsum/")}
    assert names == set(grads)
    for k in names:
        ref, got = g["gsum/" + k], grad_summary(grads[k])
        scale = bias_scale.get(k, abs(ref[1]))          # a cancelled bias: zero up to rounding, measured against sum|dy|
        assert np.abs(got - ref).max() <= 1e-9 * scale, (k, np.abs(got - ref).max(), scale)


# ---- the statement against torch.autograd, with dropout masks and in eval mode ----------------------------------------------
def autograd_forward(sd, cfg, x, train, masks):
    """the reference's module tree (networks.py:321-439) written with torch.nn.functional, differentiable"""
    nm = rr.layout(cfg["n_blocks"], cfg["use_dropout"])

    def norm(t, nname):
        if cfg["norm"] == "instance":
            return F.instance_norm(t, eps=1e-5)
        return F.batch_norm(t, sd[nname + ".running_mean"].clone(), sd[nname + ".running_var"].clone(), sd[nname + ".weight"],
                            sd[nname + ".bias"], training=train, momentum=0.1, eps=1e-5)

    def conv(t, cname, **kw):
        return F.conv2d(t, sd[cname + ".weight"], sd.get(cname + ".bias"), **kw)

    a = F.relu(norm(conv(F.pad(x, [3] * 4, mode="reflect"), nm["stem"][0]), nm["stem"][1]))
    for c, n in nm["downs"]:
        a = F.relu(norm(conv(a, c, stride=2, padding=1), n))
    for b, ((c1, n1), (c2, n2)) in enumerate(nm["blocks"]):
        q = F.relu(norm(conv(F.pad(a, [1] * 4, mode="reflect"), c1), n1))
        if cfg["use_dropout"] and train and masks is not None:
            q = q * masks[b].double() * 2.0
        a = a + norm(conv(F.pad(q, [1] * 4, mode="reflect"), c2), n2)
    for c, n in nm["ups"]:
        a = F.relu(norm(F.conv_transpose2d(a, sd[c + ".weight"], sd.get(c + ".bias"), stride=2, padding=1, output_padding=1), n))
    return torch.tanh(conv(F.pad(a, [3] * 4, mode="reflect"), nm["head"]))


@pytest.mark.parametrize("cid", ["r2_bn_drop_16x24", "r3_in_12x8_bf16", "r2_in_8", "r6_bn_8"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_backward_is_autograd(cid, train):
    c = rr.CASES[cid]
    sd, x, dout, masks = rr.case_inputs(c)
    cfg = rr.cfg_of(c)
    sd64 = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.double())
            for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    im = autograd_forward(sd64, cfg, x64, train, masks)
    (im * dout).sum().backward()
    st, im_s = rr.forward_state(sd, cfg, x, train, masks)
    assert float((im_s - im.detach()).abs().max()) <= 1e-9
    grads, dx, bias_scale = rr.replay(st, dout, True)
    assert float((dx - x64.grad).norm()) <= 1e-9 * float(x64.grad.norm())
    learnable = {k for k, v in sd64.items() if v.requires_grad}
    assert learnable == set(grads)
    for k in learnable:
        ref = sd64[k].grad
        scale = bias_scale.get(k, float(ref.norm()))
        assert float((grads[k] - ref).norm()) <= 1e-9 * scale, (k, float((grads[k] - ref).norm()), scale)


def test_fold_is_the_adjoint_of_the_pad():
    """every plane size the kernel tests use, corners included: <pad(x), d> == <x, fold(d)>, and fold == autograd of F.pad"""
    g = torch.Generator().manual_seed(5)
    for p, H, W in ((1, 2, 2), (1, 5, 7), (3, 4, 4), (3, 5, 7), (1, 33, 70), (3, 33, 70)):
        x = torch.randn((2, 3, H, W), generator=g, dtype=torch.float64, requires_grad=True)
        d = torch.randn((2, 3, H + 2 * p, W + 2 * p), generator=g, dtype=torch.float64)
        (F.pad(x, [p] * 4, mode="reflect") * d).sum().backward()
        assert float((rr.fold64(d, p) - x.grad).abs().max()) <= 1e-12, (p, H, W)


# ---- the GPU tests' bounds on the GPU tests' seeds -----------------------------------------------------------------------------
_ROUNDED = {}


def _rounded(cid, train):
    if (cid, train) not in _ROUNDED:
        c = rr.CASES[cid]
        dt = rr.DT[c["dtype"]]
        sd, x, dout, masks = rr.case_inputs(c)
        cfg = rr.cfg_of(c)
        state, image16 = rr.forward_state(sd, cfg, x, train, masks, store=dt)
        _, image64 = rr.forward_state(sd, cfg, x, train, masks)
        _ROUNDED[(cid, train)] = dict(c=c, dt=dt, cfg=cfg, inputs=(sd, x, dout, masks), state=state, image16=image16,
                                      image64=image64, rp=rr.replays(state, dout, True, dt))
    return _ROUNDED[(cid, train)]


def _stand_in(case, mutant=None):
    """the stand-in for the engine: the 16-bit replay of the (right or mutated) plan with its rounding perturbed by another
    power-of-two scale, held as the GPU tests hold the engine"""
    state = case["state"]
    S = rr.loss_scale(state["N"], state["H"], state["W"]) / 64
    grads, dx, _ = rr.replay(state, case["inputs"][2], True, case["dt"], S=S, mutant=mutant)
    return rr.hold(dict(grads, dx=dx), case["rp"], case["dt"])


ALL = sorted(rr.CASES)
DROPOUT = [c for c in ALL if rr.CASES[c]["use_dropout"]]
BATCH = [c for c in ALL if rr.CASES[c]["norm"] == "batch"]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("cid", ALL)
def test_bound_passes_a_right_implementation(cid, train):
    case = _rounded(cid, train)
    rep, bad = _stand_in(case)
    assert not bad, {k: rep[k] for k in bad}
    r64, _, d_u, _, _ = case["rp"]
    for k in r64:
        assert d_u[k] <= max(rep[k]["e16"], rr.FLOOR32), (k, d_u[k], rep[k]["e16"])


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("cid", ALL)
def test_head_bias_gradient_is_no_cancelling_sum(cid, train):
    """see resnet_reference.case_inputs: FLOOR32 holds sums of condition number below 4"""
    case = _rounded(cid, train)
    cond = rr.head_bias_condition(case["image64"], case["inputs"][2])
    assert float(cond.max()) < 4, cond


@pytest.mark.parametrize("cid", ALL)
@pytest.mark.parametrize("mutant", ["fold_drops_diagonal", "no_fold_at_head", "drop_stream_grad", "drop_branch_grad",
                                    "no_tanh_derivative"])
def test_backward_bound_catches(mutant, cid):
    rep, bad = _stand_in(_rounded(cid, True), mutant)
    assert bad, f"{mutant}: inside the bound on every tensor"


@pytest.mark.parametrize("cid", DROPOUT)
@pytest.mark.parametrize("mutant", ["ignore_keep_bwd", "keep_no_scale_bwd"])
def test_backward_bound_catches_a_wrong_keep_mask(mutant, cid):
    """the cases with Dropout modules, in train mode with explicit masks"""
    rep, bad = _stand_in(_rounded(cid, True), mutant)
    assert bad, f"{mutant}: inside the bound on every tensor"


@pytest.mark.parametrize("cid", BATCH)
def test_backward_bound_catches_c12_kept_in_eval(cid):
    """running statistics (BatchNorm in eval mode) are constants: c1 = c2 = 0.  InstanceNorm has no such mode."""
    rep, bad = _stand_in(_rounded(cid, False), "eval_keeps_c12")
    assert bad


def _fwd_ratio(cid, mutant, train=True):
    case = _rounded(cid, train)
    sd, x, _, masks = case["inputs"]
    e16 = rr.rel_err(case["image16"], case["image64"])
    _, im = rr.forward_state(sd, case["cfg"], x, train, masks, store=case["dt"], mutant=mutant)
    err = rr.rel_err(im, case["image64"])
    print(f"{cid} {mutant}: err {err:.3g} e16_fwd {e16:.3g}")
    return err / e16


@pytest.mark.parametrize("cid", ALL)
@pytest.mark.parametrize("mutant", ["replicate_pad", "symmetric_pad", "zero_pad", "border_in_stats", "residual_before_norm",
                                    "output_padding_leading", "unflipped_convT", "classes_exchanged"])
def test_forward_bound_catches(mutant, cid):
    """err(image) <= 4 * e16_fwd, e16_fwd the error of the forward with the engine's stores rounded: every wrong forward is outside"""
    assert _fwd_ratio(cid, mutant) > 4


@pytest.mark.parametrize("cid", DROPOUT)
def test_forward_bound_catches_an_ignored_keep_mask(cid):
    assert _fwd_ratio(cid, "ignore_keep") > 4


def test_forward_bound_catches_the_unbiased_variance_on_small_batches_only():
    """BatchNorm over 2 x 2 x 2 elements (case r6_bn_8): 8 / 7 of the variance moves the image outside the bound.  Under InstanceNorm,
    and under BatchNorm over more elements, the mutant is INVISIBLE in the image at every shape tried (2 x 2 planes included, case
    r2_in_8): a constant factor on a norm's output passes a bias-free conv and is removed by the next norm, and what is left (the
    branch against the residual stream) stays below 2 * e16_fwd.  The statistics kernels themselves (gs_in_stats, gs_bn_finalize)
    are held to the biased variance by the InstanceNorm / BatchNorm kernel tests."""
    assert _fwd_ratio("r6_bn_8", "unbiased_var") > 4
    assert _fwd_ratio("r2_in_8", "unbiased_var") < 4


@pytest.mark.parametrize("cid", DROPOUT)
def test_a_dropped_factor_two_is_invisible_in_the_image_but_not_in_the_state(cid):
    """`keep` without its factor 2 scales a block's first activation by one constant; the bias-free conv and the norm behind it
    remove it (up to eps), so NO image shows it.  The padded tensor the engine saves does: the exact kernel test
    (test_resnet_kernels_gpu.py) holds gs_reflect_norm_apply to keep * keep_scale element by element, and the backward's factor is
    caught by the replay bound (test_backward_bound_catches_a_wrong_keep_mask)."""
    assert _fwd_ratio(cid, "keep_no_scale") < 4
    case = _rounded(cid, True)
    sd, x, _, masks = case["inputs"]
    st, _ = rr.forward_state(sd, case["cfg"], x, True, masks, store=case["dt"], mutant="keep_no_scale")
    q, q_wrong = case["state"]["blocks"][0][1]["inp"], st["blocks"][0][1]["inp"]
    assert rr.rel_err(q_wrong, q) > 0.4


# ---- public surface (no library needed): each of these fails without the ResNet generator ----------------------------------------
def test_define_g_builds_the_default_generator_with_the_reference_keys():
    from golden_util_resnet import seeded_resnet_state_dict
    from semantic_segmentation_amd.models_pix2pix import networks
    for netG, nb in (("resnet_9blocks", 9), ("resnet_6blocks", 6)):
        for norm in ("instance", "batch"):
            for drop in (False, True):
                net = networks.define_G(1, 1, 64, netG, norm=norm, use_dropout=drop)
                assert isinstance(net, networks.ResnetGenerator)
                sd = seeded_resnet_state_dict(1, 1, 1, 64, nb, norm, drop)
                assert set(net.state_dict()) == set(sd), (netG, norm, drop)
                net.load_state_dict(sd, strict=True)
                if norm == "instance":
                    assert not any("running" in k for k in sd) and "model.1.bias" in sd
                else:
                    assert "model.2.running_mean" in sd and "model.1.bias" not in sd
    net = networks.define_G(3, 3, 16, "resnet_6blocks", norm="batch")
    assert set(net.state_dict()) == set(fixture_state_dict(FIXTURES["pix2pix_resnet_b"]))


def test_every_multiple_of_eight_and_every_channel_count_up_to_four_builds():
    """the refusals are the stated ones and no others: the canonical RGB generator define_G(3, 3, 64, 'resnet_9blocks') loads a
    reference state dict, and so do 4 channels and an ngf that is no 8 * 2^j"""
    from golden_util_resnet import seeded_resnet_state_dict
    from semantic_segmentation_amd.models_pix2pix import networks
    for cin, cout, ngf, netG, nb in ((3, 3, 64, "resnet_9blocks", 9), (4, 2, 64, "resnet_6blocks", 6), (1, 4, 24, "resnet_6blocks", 6),
                                     (3, 3, 72, "resnet_6blocks", 6), (2, 2, 8, "resnet_6blocks", 6)):
        for norm in ("instance", "batch"):
            net = networks.define_G(cin, cout, ngf, netG, norm=norm)
            net.load_state_dict(seeded_resnet_state_dict(1, cin, cout, ngf, nb, norm, False), strict=True)


def test_unsupported_configurations_are_refused_by_name():
    from semantic_segmentation_amd.models_pix2pix import networks
    bn = networks.get_norm_layer("batch")
    with pytest.raises(NotImplementedError, match="reflect"):
        networks.ResnetGenerator(1, 1, 16, norm_layer=bn, padding_type="zero")
    with pytest.raises(NotImplementedError, match="reflect"):
        networks.ResnetGenerator(1, 1, 16, norm_layer=bn, padding_type="replicate")
    with pytest.raises(NotImplementedError, match="batch"):
        networks.define_G(1, 1, 16, "resnet_9blocks", norm="none")
    with pytest.raises(NotImplementedError, match="above 4"):
        networks.ResnetGenerator(5, 1, 16, norm_layer=bn)
    with pytest.raises(NotImplementedError, match="above 4"):
        networks.ResnetGenerator(1, 5, 16, norm_layer=bn)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        networks.ResnetGenerator(1, 1, 20, norm_layer=bn)
    with pytest.raises(NotImplementedError, match="not on the MI355X hot path"):
        networks.define_G(1, 1, 16, "resnet_3blocks")


def test_input_sizes_are_refused_before_any_device_work():
    """CPU tensors: the refusals come before the engine asks for a device (which a CPU tensor fails with RuntimeError)"""
    from semantic_segmentation_amd.models_pix2pix import networks
    for norm in ("batch", "instance"):
        net = networks.define_G(1, 1, 16, "resnet_6blocks", norm=norm)
        with pytest.raises(ValueError, match="multiple of 4"):
            net(torch.zeros(1, 1, 30, 32))
        with pytest.raises(ValueError, match="multiple of 4"):
            net(torch.zeros(1, 1, 32, 18))
        with pytest.raises(ValueError, match="Padding size should be less than the corresponding input dimension"):
            net(torch.zeros(1, 1, 4, 32))                      # 1 at H/4 under a pad of 1
        with pytest.raises(ValueError, match="Padding size should be less than the corresponding input dimension"):
            net(torch.zeros(1, 1, 32, 4))
        with pytest.raises(RuntimeError, match="MI355X"):
            net(torch.zeros(1, 1, 8, 8))                       # a fine size on the CPU: no fallback
