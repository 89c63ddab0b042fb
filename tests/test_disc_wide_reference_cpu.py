"""What tests/test_disc_wide_kernels_gpu.py and tests/test_disc_wide_networks_gpu.py rest on, proven on the CPU (no GPU, no native
library):

  * every kernel case of disc_wide_reference.CASES is exact: its fp32 evaluation equals fp64 bit for bit, in another accumulation
    order too, so zero tolerance is the right bound;
  * on those very cases each stated wrong first layer gives at least one wrong element (where a wrong implementation is the right
    one at a shape -- k 1 has no taps to exchange and no pad -- the test says so and names the cases that catch it);
  * PixelDiscriminator: the fp64 statement (tests/pixel_reference.py + the discriminator replays) equals torch.autograd at 1e-9 under
    both norms, the module's key sets are the reference's, and the refusals that need no device are raised by name;
  * the fp64 statements (the PatchGAN replay at six channels, the PixelDiscriminator one) equal the fixtures the reference's own
    classes made in double (tests/golden/pix2pix_disc_{patch,pixel}.npz), logits in train and eval mode and every gradient summary;
  * on the seeds and shapes of the network tests a right implementation with the engine's 16-bit stores passes the GPU bounds and
    each stated wrong one does not."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import grad_summary, tensor_checksum
from golden_util_disc import FIXTURES, fixture_dense, fixture_input, fixture_state_dict, perturbed_running
from tests import disc_wide_reference as dw
from tests import exact_reference as er
from tests import instnorm_reference as ir
from tests import pix2pix_backward_replay as pr
from tests import pixel_reference as px

torch.set_num_threads(min(torch.get_num_threads(), 16))
K4 = [c for c in dw.CASES if c[2] == 4]
K1 = [c for c in dw.CASES if c[2] == 1]


# ================================================================================================ kernel cases
def test_the_case_list_covers_what_the_kernels_branch_on():
    assert {c[0] for c in dw.CASES} == {5, 6, 7, 8, 9, 11, 16} and {c[1] for c in dw.CASES} == {8, 24, 32, 64, 96, 128}
    assert {(c[4], c[5]) for c in K4} >= {(2, 2), (5, 7), (19, 23), (38, 134)} and {(c[4], c[5]) for c in K1} >= {(1, 1), (5, 7), (19, 67)}
    for cases in (K4, K1):
        big = [c for c in cases if dw.out_hw(c)[0] > 8 and dw.out_hw(c)[1] > 32 and dw.out_hw(c)[0] % 4 and dw.out_hw(c)[1] % 32]
        assert big, "an output larger than the 8 x 32 patch both ways and a multiple of neither patch"
        patches = [c[3] * -(-dw.out_hw(c)[0] // 4) * -(-dw.out_hw(c)[1] // 32) for c in cases]
        assert min(patches) == 1 or min(patches) == 3 and max(patches) > 256, "one block ... blocks that walk several patches"
    assert any(c[3] == 1 and dw.out_hw(c) == (1, 1) for c in dw.CASES), "the one-block weight gradient"


@pytest.mark.parametrize("case", dw.CASES, ids=dw.case_id)
def test_cases_are_exact_in_fp32_in_any_order(case):
    Cin, Cout, k, N, H, W = case
    s, p = dw.GEOM[k]
    for vset in ("S", "P"):
        c = dw.build(case, vset)                                  # asserts the product bounds
        x, w, dy = c["x"], c["w"], c["dy"]
        assert torch.equal(F.conv2d(x, w, None, stride=s, padding=p).double(), c["y"])
        perm = torch.randperm(Cin, generator=torch.Generator().manual_seed(1))
        acc = sum(F.conv2d(x[:, i:i + 1], w[:, i:i + 1], None, stride=s, padding=p) for i in perm.tolist())
        assert torch.equal(acc.double(), c["y"]), "channel by channel in a permuted order"
        assert torch.equal(torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=s, padding=p).double(), c["dw"])
        assert torch.equal(torch.nn.grad.conv2d_input(x.shape, w, dy, stride=s, padding=p).double(), c["dx"])
        er.expect32(c["dw"], dw.GSCALE), er.expect32(c["dx"], dw.GSCALE), er.expect16(c["y"], torch.bfloat16)
        assert float((c["y"] + c["b"].view(1, -1, 1, 1)).abs().max()) < er.LIMIT


def _differs(a, b):
    return er.mismatches(a.float(), b.float()).shape[0] > 0


@pytest.mark.parametrize("case", dw.CASES, ids=dw.case_id)
def test_wrong_first_layers_are_wrong_on_the_cases(case):
    """assert_exact sees each mutant on every case at which it is a different function.  Not different, by construction: k 1 has one
    tap and no pad (`ky/kx exchanged`, `pad at the bottom/right`, `classes exchanged`: the k 4 cases catch them); a 1 x 1 output has
    no border to leave out (`bias gradient without the border` is zero there, which the 2 x 2 cases catch as a wrong value)."""
    Cin, Cout, k, N, H, W = case
    c = dw.build(case, "S")
    x, w, b, dy = c["x"].double(), c["w"].double(), c["b"].double(), c["dy"].double()
    right = dw.fwd_right(x, w, b, k)
    for name, fn in dw.FWD_MUTANTS.items():
        same_function = k == 1 and name in ("ky/kx exchanged", "pad at the bottom/right")
        assert _differs(fn(x, w, b, k), right) != same_function, name
    assert _differs(dw.db_without_border(dy), dw.db_right(dy))
    assert _differs(dw.dgrad_classes_exchanged(dy, w, x.shape, k), dw.dgrad_right(dy, w, x.shape, k)) == (k == 4)


# ================================================================================================ PixelDiscriminator: the statement
def assert_1e9(got, ref):
    assert set(got) == set(ref), set(got) ^ set(ref)
    for k in ref:
        assert float((got[k] - ref[k]).norm()) <= 1e-9 * float(ref[k].norm()), k


@pytest.mark.parametrize("norm,cin,ndf,N,H,W,train", [("batch", 2, 64, 2, 8, 8, True), ("batch", 2, 64, 2, 8, 8, False),
                                                      ("instance", 6, 32, 3, 5, 7, True), ("batch", 6, 16, 2, 3, 5, True)])
def test_pixel_statement_equals_autograd(norm, cin, ndf, N, H, W, train):
    sd = px.seeded_pixel_state_dict(dw.SEED, cin, ndf, norm)
    if not train:
        pr.perturb_running(sd, dw.SEED + 2)
    net = px.torch_module(cin, ndf, norm)
    net.load_state_dict(sd, strict=True)                            # the key set
    net.train(train)
    x = torch.randn((N, cin, H, W), generator=torch.Generator().manual_seed(3), dtype=torch.float64).requires_grad_(True)
    out = net(x)
    dl = ir.dlogits_of(out.detach(), 5)
    (out * dl).sum().backward()
    state, logits = px.forward_state(sd, x.detach(), norm, train)
    assert float((logits - out.detach()).norm()) <= 1e-9 * float(out.detach().norm())
    m = ir if norm == "instance" else pr
    res = m.replay_discriminator(state, dl, True)
    got = pr.flat(res[:2])
    ref = {k: p.grad for k, p in net.named_parameters()}
    ref["dx"] = x.grad
    if norm == "instance":                                          # the bias in front of the norm: zero up to rounding on both sides
        bs = res[2]
        assert set(bs) == {"net.2.bias"}
        for k in bs:
            assert float(got.pop(k).abs().max()) <= 1e-9 * bs[k] and float(ref.pop(k).abs().max()) <= 1e-9 * bs[k]
    assert_1e9(got, ref)
    assert m.replay_discriminator(state, dl, False)[1] is None


def test_pixel_key_sets_and_refusals_by_name():
    from semantic_segmentation_amd.models_pix2pix import networks
    bn = networks.define_D(2, 64, "pixel", norm="batch")
    inn = networks.define_D(6, 32, "pixel", norm="instance")
    assert isinstance(bn, networks.PixelDiscriminator) and isinstance(bn.net, torch.nn.Sequential) and bn.engine.net is bn
    assert set(bn.state_dict()) == {"net.0.weight", "net.0.bias", "net.2.weight", "net.3.weight", "net.3.bias", "net.3.running_mean",
                                    "net.3.running_var", "net.3.num_batches_tracked", "net.5.weight"}
    assert set(inn.state_dict()) == {"net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.5.weight", "net.5.bias"}
    for norm, net, cin, ndf in (("batch", bn, 2, 64), ("instance", inn, 6, 32)):
        sd = px.seeded_pixel_state_dict(1, cin, ndf, norm)
        net.load_state_dict(sd, strict=True)
        px.torch_module(cin, ndf, norm).load_state_dict(net.state_dict(), strict=True)
        assert set(net.engine.param_names()) == {k for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    with pytest.raises(NotImplementedError, match="not on the MI355X hot path"):
        networks.define_D(2, 64, "patch")
    # refused by name before the engine asks for a device (a CPU tensor otherwise fails with RuntimeError)
    with pytest.raises(NotImplementedError, match="up to 16"):
        networks.define_D(17, 64, "basic")(torch.zeros(1, 17, 32, 32))
    with pytest.raises(NotImplementedError, match="up to 16"):
        networks.define_D(17, 64, "pixel")(torch.zeros(1, 17, 4, 4))
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        networks.define_D(6, 20, "basic")(torch.zeros(1, 6, 32, 32))
    with pytest.raises(NotImplementedError, match="at most 128"):
        networks.define_D(6, 136, "pixel")(torch.zeros(1, 6, 4, 4))
    with pytest.raises(NotImplementedError, match="up to 16"):
        networks.define_G(17, 1, 16, "unet_128")(torch.zeros(1, 17, 128, 128))
    for net in (networks.define_D(6, 64, "basic"), networks.define_D(16, 64, "pixel"), networks.define_D(4, 20, "basic")):
        with pytest.raises(RuntimeError, match="MI355X only"):
            net(torch.zeros(1, net.engine.layout()[0][1].in_channels, 32, 32))


# ================================================================================================ the fixtures of the reference
@pytest.mark.parametrize("name,i", [(n, i) for n in sorted(FIXTURES) for i in range(len(FIXTURES[n]))])
def test_statement_equals_the_reference_fixture(name, i, golden_dir):
    f = FIXTURES[name][i]
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    t = f["tag"] + "/"
    sd, x = fixture_state_dict(f), fixture_input(f)
    assert np.array_equal(g[t + "input"], x.double().numpy())
    assert {k[len(t + "wsum/"):] for k in g if k.startswith(t + "wsum/")} == set(sd)          # the reference's key set (strict=True there)
    for k, v in sd.items():
        assert np.array_equal(g[t + "wsum/" + k], tensor_checksum(v)), k
    inst = f["norm"] == "instance"

    def forward(sd_, train):
        if f["kind"] == "patch":
            return pr.discriminator_forward_state(sd_, x, train)
        return px.forward_state(sd_, x, f["norm"], train)
    state, logits = forward(sd, True)
    assert ir.rel_err(logits, torch.from_numpy(g[t + "logits"])) < 1e-9
    assert ir.rel_err(forward(perturbed_running(sd, f["seed"] + 3), False)[1], torch.from_numpy(g[t + "logits_eval"])) < 1e-9
    dense = fixture_dense(logits.shape, f)
    assert np.array_equal(g[t + "dense"], dense.numpy())
    res = (ir if inst else pr).replay_discriminator(state, dense, True)
    got = pr.flat(res[:2])
    keys = {k[len(t + "gsum/"):] for k in g if k.startswith(t + "gsum/")}
    assert keys == set(got), keys ^ set(got)
    for k in keys:
        s_got, s_ref = grad_summary(got[k]), g[t + "gsum/" + k]
        if inst and k in res[2]:                 # in front of the norm: zero up to rounding on both sides
            assert np.abs(s_got).max() <= 1e-9 * res[2][k] and np.abs(s_ref).max() <= 1e-9 * res[2][k], k
        else:
            assert np.linalg.norm(s_got - s_ref) <= 1e-9 * np.linalg.norm(s_ref), k


# ================================================================================================ the GPU bounds and the mutants
def logits_bound(ref64, l16):
    return 4 * max(ir.rel_err(l16, ref64), pr.FLOOR32)


@pytest.mark.parametrize("cid", sorted(dw.P_CASES))
def test_pixel_forward_bound_tells_the_wrong_norms(cid):
    """logits err <= 4 e16_fwd: the right forward with 16-bit stores passes (it IS e16); batch statistics for instance statistics
    and the reverse, the unbiased variance and a head bias under BatchNorm do not.  Invisible by construction: in eval mode BatchNorm
    takes its running statistics, so the two statistics mutants are the right function there (p2_bn_train catches them)."""
    cin, ndf, norm, N, H, W, train, dtn, need_dx = dw.P_CASES[cid]
    dt = ir.TORCH_DT[dtn]
    sd = px.seeded_pixel_state_dict(dw.SEED, cin, ndf, norm)
    if not train:
        pr.perturb_running(sd, dw.SEED + 2)
    x = 0.5 * torch.randn((N, cin, H, W), generator=torch.Generator().manual_seed(dw.SEED))
    ref64 = px.forward_state(sd, x, norm, train)[1]
    bound = logits_bound(ref64, px.forward_state(sd, x, norm, train, store=dt)[1])
    for mutant in px.MUTANTS:
        err = ir.rel_err(px.forward_state(sd, x, norm, train, store=dt, mutant=mutant)[1], ref64)
        same_function = (mutant == "head_bias_under_bn" and norm == "instance") or \
                        (mutant in ("swapped_stats", "unbiased_var") and norm == "batch" and not train)
        print(f"{cid} {mutant}: err {err:.3g} bound {bound:.3g}")
        if mutant == "unbiased_var" and dtn == "bf16":
            # 35 / 34 on the variance of a 5 x 7 plane moves the logits by 1.5e-2, under four bf16 forward errors (1.6e-2): invisible
            # in bf16 at this shape; the same network in fp16 (p6_in_5x7) and p2_bn_train catch it
            assert bound / 4 < err <= bound, (cid, mutant, err, bound)
            continue
        assert (err > bound) != same_function, (cid, mutant, err, bound)


def _mutated_first_layer(sd, x, name):
    """(sd', x') whose RIGHT forward is the wrong first layer `name` on (sd, x)"""
    sd = dict(sd)
    if name == "ky/kx exchanged":
        sd["model.0.weight"] = sd["model.0.weight"].transpose(2, 3).contiguous()
    elif name == "pad at the bottom/right":
        x = F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:]                    # the image one pixel up and left: no pad before, two after
    elif name == "channels reversed":
        x = x.flip(1)
    elif name == "concat halves exchanged":
        h = x.shape[1] // 2
        x = torch.cat((x[:, h:], x[:, :h]), 1)
    elif name == "bias dropped":
        sd["model.0.bias"] = torch.zeros_like(sd["model.0.bias"])
    return sd, x


@pytest.mark.parametrize("cid", sorted(dw.D_CASES))
def test_patchgan_bounds_tell_the_wrong_first_layers(cid):
    cin, ndf, nl, norm, N, H, W, train, dtn, need_dx = dw.D_CASES[cid]
    dt = ir.TORCH_DT[dtn]
    sd, x = dw.patchgan_case(cid)
    ref64 = dw.patchgan_forwards(cid, sd, x)[1]
    state16, l16 = dw.patchgan_forwards(cid, sd, x, store=dt)
    bound = logits_bound(ref64, l16)
    for name in dw.FWD_MUTANTS:
        sdm, xm = _mutated_first_layer(sd, x, name)
        err = ir.rel_err(dw.patchgan_forwards(cid, sdm, xm, store=dt)[1], ref64)
        print(f"{cid} {name}: err {err:.3g} bound {bound:.3g}")
        assert err > bound, (cid, name, err, bound)
    if norm == "batch":
        # the backward mutants of the first layer, against compare() on the right plan's replays
        dl = ir.dlogits_of(ref64, dw.SEED)
        r64, r16, d_u, _ = pr.replays(state16, dl, True, dt)
        _, bad = pr.compare(r16, r64, r16, d_u)
        assert not bad
        for mutant in pr.MUTANTS_D:
            if mutant == "d_dx_class_swapped" and (H % 2 or W % 2):
                continue             # (the statement's mutant exchanges equal-sized classes: the even-sized cases carry it)
            got = pr.flat(pr.replay_discriminator(state16, dl, True, dt, mutant=mutant))
            _, bad = pr.compare(got, r64, r16, d_u)
            assert bad, (cid, mutant)
