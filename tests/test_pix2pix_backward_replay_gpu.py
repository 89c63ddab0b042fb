"""generator_backward and DiscriminatorEngine.backward held to the fp64 replay of the state their own forward saved
(tests/pix2pix_backward_replay.py), at generators of 5 to 7 downs, non-square images, 1 and 3 channels on either side, and
discriminators of 2 and 3 layers -- configurations no other test builds.

One forward with need_grad=True under torch.no_grad(), one direct backward on a fixed dense gradient of magnitude 1 / (N H W),
then: adapt ctx -> plain state, replay in fp64 (R64) and with the engine's 16-bit stores (R16), and per tensor
    |gpu - R64| / |R64|  <=  4 * max(|R16 - R64| / |R64|, FLOOR32 / 4) + d_U
(per output-channel row in absolute terms: backward_replay.compare; darch is a [D, 3] tensor whose rows are the layers).
Every case also holds the engine's forward to the oracle's fp64 forward of the same weights, image and keep masks (generator: mean
|d| < 1e-3, max |d| < 1e-2; discriminator: max |d| < 2e-2 * max(1, |pred| max), the bounds of test_pix2pix_gpu.py), and asserts the
cheap observable of the branch it is for.  Ratios err(gpu) / e16 of every tensor go to parity_reports/backward_replay.json.

The forward bounds are fp16 ones: the two bf16 cases, whose networks an fp16 case shares, print their figures only.

Seconds per case on an MI355X host (16 CPU threads; nearly all of it the CPU fp64 replays and the oracle's forward), pytest
--durations: g7_128_dropout 7.6, g6_64x128_dx 6.3, g6_64_dropout 5.8, g5_32_f16 3.7 (the first: library load), g5_32_bf16 3.3,
g_wide_pixels 3.3, g5_eval 3.1, g_rgb_generic_wgrad 2.7, the six other 32 x 32 generator cases and chain_g_step 2.3 to 2.5 each,
the five discriminator cases 0.04 to 0.08 each; the file 55 s.

The shapes: 32 x 32 is the smallest image of a 5-down generator (the innermost level 1 x 1), 64 x 64 of a 6-down one, 128 x 128 of
a 7-down one (the generator of define_G's unet_128).  A 6-down generator takes no 32 x 64 image (multiples of 64 only): the
non-square case is 64 x 128.  g_ksplit asks the library for the smallest shape at which an inner up-conv splits K (batch 2 at
32 x 32, where block 1 does); g_onepart is batch 1, where no inner block does.  g_wide_pixels: the weight-streaming igemm
form takes a conv of up to 8192 output pixels, and the widest MFMA conv, level 2, has N H W / 16 of them -- 1 x 384 x 352 is
8448, just above that."""
import pytest
import torch

from golden_util import seeded_discriminator_state_dict, seeded_generator_state_dict
from oracle import oracle
from tests import pix2pix_backward_replay as pr

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(torch.get_num_threads(), 16))

# One seed per case, fixed here: the weights, the image, the masks and the gradient of a case come from it.  A seed is taken when no
# element of the saved state has an activation sign that fp32 cannot decide (d_U = 0), else when d_U <= e16 on every tensor; the
# test asserts the latter.  Chosen on the GPU: the state is the engine's own.
SEEDS = {"g5_32_f16": 11, "g5_32_bf16": 12, "g6_64_dropout": 11, "g6_64x128_dx": 11, "g7_128_dropout": 11, "g5_eval": 11,
         "g_rgb_generic_wgrad": 11, "g_generic_image_layer": 15, "g_ksplit": 12, "g_onepart": 11, "g_wide_pixels": 11,
         "g_input3": 11, "g_hook": 13, "g_autograd": 14, "d3_64_f16": 11, "d3_64_bf16": 12, "d2_48x80": 11, "d3_rgb_eval": 11,
         "d3_no_dx": 12, "chain_g_step": 11}


def GC(cid, cin=1, cout=1, D=5, N=2, H=32, W=32, dtype="f16", train=True, dropout=False, need_dx=False, **extra):
    return pytest.param(dict(id=cid, cin=cin, cout=cout, D=D, N=N, H=H, W=W, dtype=dtype, train=train, dropout=dropout,
                             need_dx=need_dx, seed=SEEDS[cid], **extra), id=cid)


def up_parts(N, H, W, D):
    """K parts of the merged transposed conv's weight gradient per block depth 1 .. D-1 (ngf 64), asked of the library"""
    from semantic_segmentation_amd import ops
    c = [0, 64, 128, 256, 512] + [512] * (D - 4)
    out = {}
    for d in range(1, D):
        cin_t = c[d + 1] * (2 if d + 1 < D else 1)
        out[d] = ops.conv_wgrad_parts(ops.geom_convT_class(N, H >> (d + 1), W >> (d + 1), cin_t, c[d], 8, 3, 0, 0))
    return out


def smallest_ksplit_shape():
    """the first of the shapes below, in order of their pixel count, at which some inner up-conv splits K"""
    for N, H, W in ((1, 32, 32), (2, 32, 32), (1, 32, 64), (1, 64, 64), (2, 64, 64)):
        if max(up_parts(N, H, W, 5).values()) > 1:
            return N, H, W
    raise AssertionError("no K-split shape among the candidates")


G_CASES = [
    GC("g5_32_f16"), GC("g5_32_bf16", dtype="bf16"),
    GC("g6_64_dropout", D=6, H=64, W=64, dropout=True),
    GC("g6_64x128_dx", D=6, H=64, W=128, need_dx=True),
    GC("g7_128_dropout", D=7, N=1, H=128, W=128, dropout=True),
    GC("g5_eval", train=False),
    GC("g_rgb_generic_wgrad", cout=3), GC("g_generic_image_layer", generic_image=True),
    GC("g_ksplit", ksplit=True), GC("g_onepart", N=1),
    GC("g_wide_pixels", N=1, H=384, W=352),
    GC("g_input3", cin=3, need_dx=True),
    GC("g_hook", hook=True), GC("g_autograd", autograd=True, need_dx=True),
]


def make_generator(c):
    from semantic_segmentation_amd.models_pix2pix import networks
    sd = seeded_generator_state_dict(c["seed"], c["cin"], c["cout"], c["D"], 64, bias_std=0.05)
    if not c["train"]:
        pr.perturb_running(sd, c["seed"] + 2)          # running statistics that are not the initial 0 / 1
    net = networks.UnetGenerator(c["cin"], c["cout"], c["D"], 64, norm_layer=networks.get_norm_layer("batch"),
                                 use_dropout=c["dropout"], compute_dtype=c["dtype"])
    net.load_state_dict(sd, strict=True)
    return net.cuda().train(c["train"]), sd


def generator_forward(c, net, sd):
    """the inputs of case c on the GPU, one forward with need_grad=True, and the forward held to the oracle"""
    dev = torch.device("cuda:0")
    x, dout, arch, masks = pr.gen_inputs(c["cin"], c["cout"], c["D"], c["N"], c["H"], c["W"], c["seed"])
    use_masks = c["dropout"] and c["train"]
    dmasks = [m.permute(0, 2, 3, 1).contiguous().to(torch.uint8).to(dev) for m in masks] if use_masks else None
    xd, archd = x.to(dev), arch.to(dev)
    with torch.no_grad():
        out, ctx = net.engine.forward(xd, archd, c["train"], True, dmasks)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    ref = oracle.unet_generator_forward(sd64, arch.double(), x.double(), train=c["train"],
                                        dropout_masks=masks if use_masks else None, num_downs=c["D"])
    d = (out.detach().cpu().double() - ref).abs()
    assert out.shape == ref.shape
    print(f"{c['id']}: forward mean |d| {float(d.mean()):.3g} max |d| {float(d.max()):.3g}")
    if c["dtype"] == "f16":             # the bounds are fp16 ones; the bf16 cases share their network with an fp16 case
        assert float(d.mean()) < 1e-3 and float(d.max()) < 1e-2, ("forward against the oracle", float(d.mean()), float(d.max()))
    return xd, archd, dmasks, dout.float().to(dev), out, ctx


def hold(key, got, state_replays):
    r64, r16, d_u, n_und = state_replays
    assert set(got) == set(r64), set(got) ^ set(r64)
    rep, bad = pr.compare(got, r64, r16, d_u)
    pr.record(key, rep, n_und)
    worst = max(rep, key=lambda k: rep[k]["ratio"])
    print(f"{key}: undecided {n_und}, worst {worst} ratio {rep[worst]['ratio']:.3g} row_worst {rep[worst]['row_worst']:.3g}, "
          f"largest row_worst {max(r['row_worst'] for r in rep.values()):.3g}, max d_U {max(d_u.values()):.3g}")
    for k in r64:
        assert d_u[k] <= max(rep[k]["e16"], pr.FLOOR32), f"{k}: d_U {d_u[k]:.3g} above e16 {rep[k]['e16']:.3g}: this case needs another seed"
    assert not bad, {k: rep[k] for k in bad}


@pytest.mark.parametrize("c", G_CASES)
def test_generator_backward_is_the_replay(c, monkeypatch):
    from semantic_segmentation_amd import ops
    from semantic_segmentation_amd.models_pix2pix import networks, pix2pix_backward as pb, pix2pix_engine as pe
    if c.get("ksplit"):
        c = dict(c)
        c["N"], c["H"], c["W"] = smallest_ksplit_shape()
    if c.get("generic_image"):
        monkeypatch.setattr(pb, "IMAGE_WGRAD_DIRECT", False)
        monkeypatch.setattr(pe, "DIRECT_IMAGE_LAYER", False)
    net, sd = make_generator(c)
    eng = net.engine
    xd, archd, dmasks, dout, out, ctx = generator_forward(c, net, sd)
    announced = {}
    if c.get("hook"):
        eng.grad_ready_hook = lambda name, gr: announced.setdefault(name, []).append(gr.clone())
    with torch.no_grad():
        grads, darch, dx = pb.generator_backward(eng, ctx, archd, dout, c["need_dx"])
    torch.cuda.synchronize()
    eng.grad_ready_hook = None
    N, D, H, W = c["N"], c["D"], c["H"], c["W"]

    # ---- the branch this case is for
    ups, levels = ctx["ups"], ctx["levels"]
    assert ctx["D"] == D and ctx["hs"][D] == H >> D and ctx["ws"][D] == W >> D
    assert ups[0]["cpad"] == 8 and ups[0]["u"] is not None, "the image layer saves its pre-activation"
    direct_fwd = pe.DIRECT_IMAGE_LAYER and ops.upconv8_image_fits(128, c["cout"])
    direct_wgrad = pb.IMAGE_WGRAD_DIRECT and ops.upconv8_image_wgrad_ok(128, c["cout"])
    assert direct_fwd == (c["cout"] == 1 and not c.get("generic_image")), "the direct image layer is the one-channel one"
    assert direct_wgrad == (c["cout"] == 1 and not c.get("generic_image")), "direct image wgrad: one output channel"
    assert all(lv["stats"] == (c["train"] and 1 < k < D) for k, lv in enumerate(levels) if k >= 1)
    assert all(ups[d]["stats"] == c["train"] for d in range(1, D))
    kept = [d for d in range(1, D) if ups[d]["keep"] is not None]
    assert kept == ([d for d in range(1, D) if 1 <= D - 1 - d <= D - 5] if (c["dropout"] and c["train"]) else [])
    assert all(ups[d]["kscale"] == 2.0 for d in kept)
    assert (dx is not None) == c["need_dx"]
    nparts = up_parts(N, H, W, D)
    if c["id"] == "g_onepart":
        assert max(nparts.values()) == 1, nparts
    if c.get("ksplit"):
        split = [d for d, n in nparts.items() if n > 1]
        assert split, nparts
        # the `direct` condition of upconv_bwd: the split pass sums the slabs itself
        assert all(ups[d]["cout"] % 8 == 0 and ops.upconv_split_wgrad_parts_ok(ups[d]["cin"], ups[d]["cout"]) for d in split)
    # the weight-streaming igemm form writes one BatchNorm partial row per 16 output pixels, the tiled form one per 128
    M2 = N * (H >> 2) * (W >> 2)
    assert ops.conv_igemm_mtiles(levels[2]["geom"]) == -(-M2 // (16 if M2 <= 8192 else 128))
    assert (M2 > 8192) == (c["id"] == "g_wide_pixels")

    # ---- replay and compare
    got = {k: v.detach().cpu() for k, v in grads.items()}
    got["darch"] = darch.detach().cpu()
    if dx is not None:
        got["dx"] = dx.detach().cpu()
    state = pr.state_from_generator_ctx(eng, ctx, archd)
    hold("pix2pix_g/" + c["id"], got, pr.replays(state, pr.d64(dout), c["need_dx"], eng.tdt))

    if c.get("hook"):
        # every gradient is announced exactly once and is the returned one
        assert set(announced) == set(grads)
        for k in grads:
            assert len(announced[k]) == 1 and torch.equal(announced[k][0], grads[k]), k
    if c.get("autograd"):
        # the public path: G(mask) then backward; bit-equal to the direct call, which pins the name-to-parameter mapping
        arch_leaf = archd.clone().requires_grad_(True)
        monkeypatch.setattr(networks, "upconv_arch", arch_leaf)
        x_leaf = xd.clone().requires_grad_(True)
        net.load_state_dict(sd, strict=True)
        out2 = net(x_leaf, dmasks)
        assert torch.equal(out2.detach(), out)
        (out2 * dout).sum().backward()
        torch.cuda.synchronize()
        params = dict(net.named_parameters())
        assert set(params) == set(grads)
        for k, p in params.items():
            assert torch.equal(p.grad, grads[k].reshape(p.shape)), k
        assert torch.equal(arch_leaf.grad, darch) and torch.equal(x_leaf.grad, dx)


# ================================================================================================ discriminator
def DC(cid, cin=2, n_layers=3, N=2, H=64, W=64, dtype="f16", train=True, need_dx=True):
    return pytest.param(dict(id=cid, cin=cin, n_layers=n_layers, N=N, H=H, W=W, dtype=dtype, train=train, need_dx=need_dx,
                             seed=SEEDS[cid]), id=cid)


D_CASES = [DC("d3_64_f16"), DC("d3_64_bf16", dtype="bf16"), DC("d2_48x80", n_layers=2, H=48, W=80),
           DC("d3_rgb_eval", cin=4, train=False), DC("d3_no_dx", need_dx=False)]


def make_discriminator(c):
    from semantic_segmentation_amd.models_pix2pix import networks
    sd = seeded_discriminator_state_dict(c["seed"], c["cin"], 64, c["n_layers"], bias_std=0.05)
    if not c["train"]:
        pr.perturb_running(sd, c["seed"] + 2)
    net = networks.NLayerDiscriminator(c["cin"], 64, c["n_layers"], networks.get_norm_layer("batch"), compute_dtype=c["dtype"])
    net.load_state_dict(sd, strict=True)
    return net.cuda().train(c["train"]), sd


def discriminator_forward(c, net, sd, xd):
    with torch.no_grad():
        logits, ctx = net.engine.forward(xd, c["train"], True)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    ref = oracle.nlayer_discriminator_forward(sd64, xd.detach().cpu().double(), train=c["train"], n_layers=c["n_layers"])
    assert logits.shape == ref.shape
    d = float((logits.detach().cpu().double() - ref).abs().max())
    print(f"{c['id']}: forward max |d| {d:.3g} of |pred| max {float(ref.abs().max()):.3g}")
    if c["dtype"] == "f16":
        assert d < 2e-2 * max(1.0, float(ref.abs().max())), ("forward against the oracle", d)
    g = torch.Generator().manual_seed(c["seed"] + 1)
    dl = (torch.rand(ref.shape, generator=g, dtype=torch.float64) * 2 - 1) / ref.numel()
    return logits, ctx, dl.float().to(xd.device)


@pytest.mark.parametrize("c", D_CASES)
def test_discriminator_backward_is_the_replay(c):
    net, sd = make_discriminator(c)
    eng = net.engine
    g = torch.Generator().manual_seed(c["seed"])
    xd = torch.randn((c["N"], c["cin"], c["H"], c["W"]), generator=g).cuda()
    logits, ctx, dl = discriminator_forward(c, net, sd, xd)
    with torch.no_grad():
        grads, dx = eng.backward(ctx, dl, c["need_dx"])
    torch.cuda.synchronize()
    recs = ctx["recs"]
    assert [r["kind"] for r in recs] == ["first"] + ["mid"] * c["n_layers"] + ["last"]
    assert [r["s"] for r in recs] == [2] * c["n_layers"] + [1, 1]
    assert all(r["stats"] == c["train"] for r in recs[1:-1])
    assert (dx is not None) == c["need_dx"]
    got = {k: v.detach().cpu() for k, v in grads.items()}
    if dx is not None:
        got["dx"] = dx.detach().cpu()
    state = pr.state_from_discriminator_ctx(eng, ctx)
    hold("pix2pix_d/" + c["id"], got, pr.replays(state, pr.d64(dl), c["need_dx"], eng.tdt))


def test_chain_of_the_generator_step():
    """the generator step's chain through both engines, called directly: G forward, D forward on cat(mask, fake), D backward on a
    dense dlogits with need_dx, G backward on the fake image's share of that dx; the replay chains the two statements the same way"""
    from semantic_segmentation_amd.models_pix2pix import pix2pix_backward as pb
    seed = SEEDS["chain_g_step"]
    cg = dict(id="chain_g_step", cin=1, cout=1, D=5, N=2, H=32, W=32, dtype="f16", train=True, dropout=False, need_dx=False, seed=seed)
    cd = dict(id="chain_g_step", cin=2, n_layers=3, N=2, H=32, W=32, dtype="f16", train=True, need_dx=True, seed=seed + 5)
    netg, sdg = make_generator(cg)
    netd, sdd = make_discriminator(cd)
    xd, archd, _, _, fake, ctxg = generator_forward(cg, netg, sdg)
    pair = torch.cat((xd, fake), 1)
    logits, ctxd, dl = discriminator_forward(cd, netd, sdd, pair)
    with torch.no_grad():
        _, dxd = netd.engine.backward(ctxd, dl, True)
        grads, darch, dx = pb.generator_backward(netg.engine, ctxg, archd, dxd[:, 1:].contiguous(), False)
    torch.cuda.synchronize()
    assert dx is None and dxd.shape == pair.shape
    got = {k: v.detach().cpu() for k, v in grads.items()}
    got["darch"] = darch.detach().cpu()
    state_d = pr.state_from_discriminator_ctx(netd.engine, ctxd)
    state_g = pr.state_from_generator_ctx(netg.engine, ctxg, archd)
    hold("pix2pix_g/chain_g_step", got, pr.replays_chain(state_d, state_g, pr.d64(dl), netg.engine.tdt, 1))
