"""The fp64 backward replay (backward_replay.py) proven on the CPU: it IS the backward of the reference network, its bound tells
each stated wrong backward from a right one, and its adapter reads the engine's layouts."""
from types import SimpleNamespace

import pytest
import torch

from tests import backward_replay as br
from oracle import oracle

torch.set_num_threads(min(torch.get_num_threads(), 16))

# (n_channels, n_classes, N, H, W, train, bilinear, need_dx): the network variants of test_unet_backward_replay_gpu.py
VARIANTS = [(1, 2, 2, 64, 64, True, False, False), (1, 1, 2, 48, 80, True, False, True), (1, 2, 2, 44, 52, True, False, False),
            (3, 2, 2, 32, 32, True, False, True), (8, 9, 2, 32, 32, True, False, True), (1, 2, 2, 44, 52, True, True, False),
            (1, 2, 2, 32, 32, False, False, False)]


def _inputs(cin, ncls, N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, cin, H, W), generator=g)
    dl = (torch.rand((N, ncls, H, W), generator=g, dtype=torch.float64) * 2 - 1) / (N * H * W)
    return x, dl


@pytest.mark.parametrize("v", VARIANTS, ids=lambda v: "c{}k{}_n{}_{}x{}_{}{}{}".format(
    v[0], v[1], v[2], v[3], v[4], "train" if v[5] else "eval", "_bilinear" if v[6] else "", "_dx" if v[7] else ""))
def test_replay_is_the_backward(v):
    """state from the oracle's forward in fp64 (nothing rounded, exact statistics): the replay's gradients are torch.autograd's
    through the oracle's network, to 1e-9 relative, every tensor and dx"""
    cin, ncls, N, H, W, train, bilinear, need_dx = v
    sd = oracle.unet_state_dict(cin, ncls, seed=5, bilinear=bilinear)
    if not train:                       # running statistics that are not the initial 0 / 1
        g = torch.Generator().manual_seed(9)
        for k in sd:
            if k.endswith("running_mean"):
                sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
            elif k.endswith("running_var"):
                sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    x, dl = _inputs(cin, ncls, N, H, W, seed=3)
    state, logits = br.unet_forward_state(sd, x, train=train, bilinear=bilinear)
    leaves = {k: t.double().requires_grad_(True) for k, t in sd.items()
              if t.is_floating_point() and "running" not in k}
    sd64 = {k: (leaves[k] if k in leaves else (t.double() if t.is_floating_point() else t)) for k, t in sd.items()}
    x64 = x.double().requires_grad_(True)
    ref_logits = oracle.unet_forward(sd64, x64, train=train, bilinear=bilinear)
    assert torch.allclose(logits, ref_logits.detach(), rtol=1e-11, atol=1e-11)
    names = list(leaves)
    ref = dict(zip(names + ["dx"], torch.autograd.grad(ref_logits, [leaves[k] for k in names] + [x64], dl)))
    grads, dx = br.replay(state, dl, need_dx)
    assert set(grads) == set(names)
    assert (dx is not None) == need_dx
    if need_dx:
        grads["dx"] = dx
    for k, g in grads.items():
        e = float((g - ref[k]).norm()) / float(ref[k].norm())
        assert e < 1e-9, (k, e)


MUT = dict(cin=1, ncls=2, N=1, H=44, W=52)          # odd sizes at three up levels (5 / 11 rows, 13 columns), training statistics


@pytest.fixture(scope="module")
def rounded_case():
    """a CPU-made state with fp16 storage, its two replays, and the stand-in 'result'"""
    c = MUT
    sd = oracle.unet_state_dict(c["cin"], c["ncls"], seed=5)
    x, dl = _inputs(c["cin"], c["ncls"], c["N"], c["H"], c["W"], seed=4)
    state, _ = br.unet_forward_state(sd, x, train=True, store=torch.float16)
    r64, r16, d_u, n_und = br.replays(state, dl, False, torch.float16)
    return state, dl, r64, r16, d_u, n_und


def test_bound_passes_a_right_backward(rounded_case):
    """the stand-in: a second 16-bit replay whose rounding is perturbed by another power-of-two S (fp16 subnormals move)"""
    state, dl, r64, r16, d_u, _ = rounded_case
    S = br.loss_scale(MUT["N"], MUT["H"], MUT["W"])
    got, _ = br.replay(state, dl, False, torch.float16, S=S / 64)
    rep, bad = br.compare(got, r64, r16, d_u)
    assert not bad, {k: rep[k] for k in bad}
    for k in r64:
        assert d_u[k] <= max(rep[k]["e16"], br.FLOOR32), (k, d_u[k], rep[k]["e16"])


@pytest.mark.parametrize("mutant", br.MUTANTS)
def test_bound_catches(rounded_case, mutant):
    state, dl, r64, r16, d_u, _ = rounded_case
    S = br.loss_scale(MUT["N"], MUT["H"], MUT["W"])
    got, _ = br.replay(state, dl, False, torch.float16, S=S / 64, mutant=mutant)
    rep, bad = br.compare(got, r64, r16, d_u)
    assert bad, f"{mutant}: inside 4 * e16 + d_U on every tensor"


def _as_engine_ctx(state, dt, pair, cpad=None):
    """the plain state laid out as UNetEngine lays its own out: NHWC, 16-bit; pair=True: every stage input and up input the hi
    plane of a [hi | lo] buffer (a concat buffer: [skip_h up_h | skip_l up_l]) with a non-zero lo plane; cpad: the image stage's
    input zero-padded to cpad channels"""
    g = torch.Generator().manual_seed(1)

    def nhwc(t, lo=False, pad=0):
        t = t.permute(0, 2, 3, 1)
        parts = [t]
        if pad:
            parts.append(torch.zeros(t.shape[:3] + (pad,), dtype=t.dtype))
        if lo:
            parts.append(torch.rand(t.shape[:3] + (t.shape[3] + pad,), generator=g, dtype=torch.float64))
        return torch.cat(parts, 3).to(dt)

    recs, ups, params = [], [], {}
    for name, st in state["stages"].items():
        r = SimpleNamespace(name=name, wkey=st["wkey"], bnkey=st["bnkey"], inp_is_image=st["image"], train_stats=st["train_stats"],
                            cout=st["w"].shape[0], cin=st["w"].shape[1], wide=0, inp_stride=None,
                            h=st["inp"].shape[2], w=st["inp"].shape[3])
        if st["image"]:
            r.inp = st["inp"].float()
        elif name == "inc.0":
            r.wide, r.cin = r.cin, cpad
            r.inp = nhwc(st["inp"], pad=cpad - r.wide)
        else:
            r.inp = nhwc(st["inp"], lo=pair)
            r.inp_stride = 2 * r.cin if pair else None
        r.y = None if st["y"] is None else nhwc(st["y"])
        r.coef = torch.stack([st["scale"], st["shift"], st["mean"], st["invstd"]]).float()
        recs.append(r)
        params[st["wkey"]] = st["w"].float()
    for name, u in state["ups"].items():
        ups.append(SimpleNamespace(name=name, zin=nhwc(u["zin"], lo=pair), cin=u["zin"].shape[1], pt=u["pt"], pl=u["pl"], h=u["h"],
                                   w=u["w_"], H2=u["H2"], W2=u["W2"], geom_bwd=object() if u["transposed"] else None))
        if u["transposed"]:
            params[name + ".up.weight"] = u["w"].float()
    head = state["head"]
    params["outc.conv.weight"], params["outc.conv.bias"] = head["w"].float(), head["b"].float()
    z_last = None if head["z_last"] is None else nhwc(head["z_last"])
    return dict(recs=recs, ups=ups, z_last=z_last, N=state["N"], H=state["H"], W=state["W"]), params


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b), (path, set(a) ^ set(b))
        for k in a:
            _same(a[k], b[k], f"{path}/{k}")
    elif torch.is_tensor(a):
        assert a.shape == b.shape and torch.equal(a, b), path
    else:
        assert a == b, (path, a, b)


@pytest.mark.parametrize("cfg", [(8, 9, "f16", True), (5, 2, "bf16", False), (1, 2, "f16", True)], ids=lambda c: f"c{c[0]}k{c[1]}_{c[2]}_{'pair' if c[3] else 'dense'}")
def test_adapter_round_trip(cfg):
    """CPU tensors in the engine's layouts -- strided hi planes, channel offsets of the concat buffers, padded image channels --
    come back as the plain state they were made from"""
    cin, ncls, dtn, pair = cfg
    dt = br.DT[dtn]
    sd = oracle.unet_state_dict(cin, ncls, seed=2)
    x, _ = _inputs(cin, ncls, 1, 16, 24, seed=6)
    state, _ = br.unet_forward_state(sd, x, train=True, store=dt)
    if cin == 1:
        state["stages"]["inc.0"]["y"] = None          # the fused stem never stores its conv output
    ctx, params = _as_engine_ctx(state, dt, pair, cpad=(cin + 7) // 8 * 8)
    back = br.state_from_unet_ctx(br.engine_like(dtn, ncls), ctx, params)
    _same(state, back)


# ================================================================================================ UNet3D
# (in_channels, classes, level_channels, bottleneck, NB, D, H, W, train): the variants of test_unet3d_backward_replay_gpu.py
NARROW = ((16, 32, 64), 128)
VARIANTS3D = [(1, 2, (64, 128, 256), 512, 2, 8, 16, 16, True), (2, 9, (64, 128, 256), 512, 1, 16, 16, 16, True),
              (1, 2) + NARROW + (1, 16, 16, 16, True), (1, 2, (64, 128, 256), 512, 1, 8, 16, 16, False)]


def _inputs3d(cin, ncls, NB, D, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((NB, cin, D, H, W), generator=g)
    dl = (torch.rand((NB, ncls, D, H, W), generator=g, dtype=torch.float64) * 2 - 1) / (NB * D * H * W)
    return x, dl


def _sd3d(cin, ncls, lc, bc, train, seed=5):
    sd = oracle.unet3d_state_dict(cin, ncls, seed=seed, level_channels=lc, bottleneck_channel=bc)
    if not train:
        g = torch.Generator().manual_seed(9)
        for k in sd:
            if k.endswith("running_mean"):
                sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
            elif k.endswith("running_var"):
                sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    return sd


@pytest.mark.parametrize("v", VARIANTS3D, ids=lambda v: "c{}k{}_w{}_n{}_{}x{}x{}_{}".format(
    v[0], v[1], v[2][0], v[4], v[5], v[6], v[7], "train" if v[8] else "eval"))
def test_replay3d_is_the_backward(v):
    """as test_replay_is_the_backward for UNet3D; the bias of a conv in front of batch statistics comes out as an exact ~1e-16"""
    cin, ncls, lc, bc, NB, D, H, W, train = v
    sd = _sd3d(cin, ncls, lc, bc, train)
    x, dl = _inputs3d(cin, ncls, NB, D, H, W, seed=3)
    state, logits = br.unet3d_forward_state(sd, x, train=train)
    leaves = {k: t.double().requires_grad_(True) for k, t in sd.items() if t.is_floating_point() and "running" not in k}
    sd64 = {k: (leaves[k] if k in leaves else (t.double() if t.is_floating_point() else t)) for k, t in sd.items()}
    ref_logits = oracle.unet3d_forward(sd64, x.double(), train=train)
    assert torch.allclose(logits, ref_logits.detach(), rtol=1e-11, atol=1e-11)
    names = list(leaves)
    ref = dict(zip(names, torch.autograd.grad(ref_logits, [leaves[k] for k in names], dl)))
    grads, bias_scale = br.replay3d(state, dl)
    assert set(grads) == set(names)
    assert (len(bias_scale) == 14) == train
    for k, g in grads.items():
        if k in bias_scale:
            assert float(g.abs().max()) <= 1e-12 * bias_scale[k] and float(ref[k].abs().max()) <= 1e-12 * bias_scale[k], k
            continue
        e = float((g - ref[k]).norm()) / float(ref[k].norm())
        assert e < 1e-9, (k, e)


MUT3D = dict(cin=1, ncls=2, NB=1, D=8, H=16, W=16)


@pytest.fixture(scope="module")
def rounded_case3d():
    c = MUT3D
    sd = _sd3d(c["cin"], c["ncls"], *NARROW, True)
    x, dl = _inputs3d(c["cin"], c["ncls"], c["NB"], c["D"], c["H"], c["W"], seed=4)
    state, _ = br.unet3d_forward_state(sd, x, train=True, store=torch.float16)
    return (state, dl) + br.replays3d(state, dl, torch.float16)


def test_bound3d_passes_a_right_backward(rounded_case3d):
    state, dl, r64, r16, d_u, _, bias_scale = rounded_case3d
    S = br.loss_scale(MUT3D["NB"] * MUT3D["D"], MUT3D["H"], MUT3D["W"])
    got, _ = br.replay3d(state, dl, torch.float16, S=S / 64)
    rep, bad = br.compare3d(got, r64, r16, d_u, bias_scale, torch.float16)
    assert not bad, {k: rep[k] for k in bad}
    assert len(bias_scale) == 14 and all(rep[k]["absolute"] for k in bias_scale)


@pytest.mark.parametrize("mutant", br.MUTANTS3D)
def test_bound3d_catches(rounded_case3d, mutant):
    state, dl, r64, r16, d_u, _, bias_scale = rounded_case3d
    S = br.loss_scale(MUT3D["NB"] * MUT3D["D"], MUT3D["H"], MUT3D["W"])
    got, _ = br.replay3d(state, dl, torch.float16, S=S / 64, mutant=mutant)
    rep, bad = br.compare3d(got, r64, r16, d_u, bias_scale, torch.float16)
    assert bad, f"{mutant}: inside 4 * e16 + d_U on every tensor"


def _as_engine3d_ctx(state, dt, pair):
    """the plain 3-D state as UNet3DEngine lays it out: [NB*D, H, W, C] 16-bit buffers; pair=True: hi planes of pair buffers and
    the concat buffers as [up_h res_h | res_l -]; a multi-channel volume zero-padded to 8 channels"""
    NB = state["NB"]
    g = torch.Generator().manual_seed(1)

    def ndhwc(t, lo=False, pad=0):
        t = t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[3], t.shape[4], t.shape[1])
        parts = [t]
        if pad:
            parts.append(torch.zeros(t.shape[:3] + (pad,), dtype=t.dtype))
        if lo:
            parts.append(torch.rand(t.shape[:3] + (t.shape[3] + pad,), generator=g, dtype=torch.float64))
        return torch.cat(parts, 3).to(dt)

    params, mods, stages = [], {}, []
    for name, st in state["stages"].items():
        conv = SimpleNamespace(weight=st["w"].float(), bias=torch.zeros(st["w"].shape[0]))
        params += [(name + ".weight", conv.weight), (name + ".bias", conv.bias)]
        s = SimpleNamespace(conv=conv, first=st["first"], stats=st["train_stats"], wide=0, in_coff=0, cin=st["w"].shape[1],
                            y=ndhwc(st["y"]), coef=torch.stack([st["scale"], st["shift"], st["mean"], st["invstd"]]).float())
        if st["first"]:
            s.inp = st["inp"].float()
        elif name == "a_block1.conv1":
            s.wide, s.cin = s.cin, 8
            s.inp = ndhwc(st["inp"], pad=8 - s.wide)
        else:
            s.inp = ndhwc(st["inp"], lo=pair)
        stages.append(s)
    ups, cats = {}, {}
    for k, u in state["ups"].items():
        mods[f"s_block{k}.upconv1"] = SimpleNamespace(weight=u["w"].float())
        ups[k] = dict(zin=ndhwc(u["zin"], lo=pair), cin=u["zin"].shape[1], cup=u["cup"])
        z = state["pool_z"][k]
        up_half = torch.rand((z.shape[0], u["cup"]) + z.shape[2:], generator=g, dtype=torch.float64)
        cats[k] = ndhwc(torch.cat((up_half, z), 1), lo=pair)
    hd = state["head"]
    mods["s_block1.conv3"] = SimpleNamespace(weight=hd["w"].float(), bias=hd["b"].float())
    eng = SimpleNamespace(tdt=dt, param_items=lambda: params, submodule=lambda n: mods[n])
    ctx = dict(NB=NB, stages=stages, ups=ups, cats=cats, dims=state["dims"], z_last=ndhwc(hd["z_last"]), pair=pair)
    return eng, ctx


@pytest.mark.parametrize("cfg", [(2, 9, "f16", True), (1, 2, "bf16", False)], ids=lambda c: f"c{c[0]}k{c[1]}_{c[2]}_{'pair' if c[3] else 'dense'}")
def test_adapter3d_round_trip(cfg):
    cin, ncls, dtn, pair = cfg
    dt = br.DT[dtn]
    sd = _sd3d(cin, ncls, *NARROW, True, seed=2)
    x, _ = _inputs3d(cin, ncls, 2, 8, 8, 16, seed=6)
    state, _ = br.unet3d_forward_state(sd, x, train=True, store=dt)
    eng, ctx = _as_engine3d_ctx(state, dt, pair)
    _same(state, br.state_from_unet3d_ctx(eng, ctx))
