"""The fp64 replay of the Pix2Pix backward plans (pix2pix_backward_replay.py) proven on the CPU: it IS the backward of the reference
networks (torch.autograd through the oracle, 1e-9), its bound tells each stated wrong backward from a right one, and its adapters
read the engines' layouts."""
import math
from types import SimpleNamespace

import pytest
import torch

from golden_util import seeded_discriminator_state_dict, seeded_generator_state_dict
from oracle import oracle
from tests import pix2pix_backward_replay as pr

torch.set_num_threads(min(torch.get_num_threads(), 16))
NGF = 8            # the proof is about the plan, not the width: narrow networks keep it quick


def leaves_of(sd):
    leaves = {k: t.double().requires_grad_(True) for k, t in sd.items() if t.is_floating_point() and "running" not in k}
    return leaves, {k: (leaves[k] if k in leaves else (t.double() if t.is_floating_point() else t)) for k, t in sd.items()}


def assert_equal_1e9(got, ref):
    assert set(got) == set(ref), set(got) ^ set(ref)
    for k, g in got.items():
        e = float((g - ref[k]).norm()) / float(ref[k].norm())
        assert e < 1e-9, (k, e)


# (input_nc, output_nc, num_downs, N, H, W, train, dropout)
G_VARIANTS = [(1, 1, 5, 2, 32, 32, True, False), (1, 3, 6, 2, 64, 64, True, True), (3, 1, 5, 2, 32, 64, False, False),
              (1, 1, 6, 1, 64, 128, True, True), (3, 3, 6, 2, 64, 64, False, False)]


@pytest.mark.parametrize("v", G_VARIANTS, ids=lambda v: "i{}o{}_d{}_n{}_{}x{}_{}{}".format(
    v[0], v[1], v[2], v[3], v[4], v[5], "train" if v[6] else "eval", "_dropout" if v[7] else ""))
def test_generator_replay_is_the_backward(v):
    """state from the forward in fp64 (nothing rounded, exact statistics): the replay's gradients are torch.autograd's through
    the oracle's generator for the objective <out, dout>: every parameter, darch and dx, to 1e-9 relative"""
    cin, cout, D, N, H, W, train, dropout = v
    sd = seeded_generator_state_dict(5, cin, cout, D, NGF, bias_std=0.05)
    if not train:
        pr.perturb_running(sd)
    x, dout, arch, masks = pr.gen_inputs(cin, cout, D, N, H, W, seed=3, ngf=NGF)
    masks = masks if dropout else None
    state, out = pr.generator_forward_state(sd, arch, x, train, masks, D)
    leaves, sd64 = leaves_of(sd)
    x64, arch64 = x.double().requires_grad_(True), arch.double().requires_grad_(True)
    ref_out = oracle.unet_generator_forward(sd64, arch64, x64, train=train, dropout_masks=masks, num_downs=D)
    assert torch.allclose(out, ref_out.detach(), rtol=1e-11, atol=1e-11)
    names = list(leaves)
    ref = dict(zip(names + ["darch", "dx"], torch.autograd.grad(ref_out, [leaves[k] for k in names] + [arch64, x64], dout)))
    if dropout:
        assert sum(u["keep"] is not None for u in state["ups"].values()) == D - 5
    assert_equal_1e9(pr.flat(pr.replay_generator(state, dout, True)), ref)
    assert pr.replay_generator(state, dout, False)[2] is None


# (input_nc, n_layers, N, H, W, train)
D_VARIANTS = [(2, 3, 2, 64, 64, True), (2, 2, 2, 48, 80, True), (4, 3, 1, 64, 64, False), (2, 4, 1, 64, 96, True)]


@pytest.mark.parametrize("v", D_VARIANTS, ids=lambda v: "i{}_l{}_n{}_{}x{}_{}".format(v[0], v[1], v[2], v[3], v[4], "train" if v[5] else "eval"))
def test_discriminator_replay_is_the_backward(v):
    cin, n_layers, N, H, W, train = v
    sd = seeded_discriminator_state_dict(5, cin, NGF, n_layers, bias_std=0.05)
    if not train:
        pr.perturb_running(sd)
    g = torch.Generator().manual_seed(3)
    x = torch.randn((N, cin, H, W), generator=g)
    state, logits = pr.discriminator_forward_state(sd, x, train)
    dl = (torch.rand(logits.shape, generator=g, dtype=torch.float64) * 2 - 1) / logits.numel()
    leaves, sd64 = leaves_of(sd)
    x64 = x.double().requires_grad_(True)
    ref_logits = oracle.nlayer_discriminator_forward(sd64, x64, train=train, n_layers=n_layers)
    assert torch.allclose(logits, ref_logits.detach(), rtol=1e-11, atol=1e-11)
    names = list(leaves)
    ref = dict(zip(names + ["dx"], torch.autograd.grad(ref_logits, [leaves[k] for k in names] + [x64], dl)))
    assert_equal_1e9(pr.flat(pr.replay_discriminator(state, dl, True)), ref)
    assert pr.replay_discriminator(state, dl, False)[1] is None


# ================================================================================================ the bound and the mutants
# Seeds chosen so that the right plan alone passes with d_U <= e16 on every tensor (asserted below).
MUT_G = dict(cin=1, cout=1, D=6, N=2, H=64, W=64, seed=4)
MUT_E = dict(cin=1, cout=1, D=5, N=2, H=32, W=32, seed=4)
MUT_D = dict(cin=2, n_layers=3, N=2, H=64, W=64, seed=4)
EVAL_ONLY = ("eval_keeps_c12",)


def _rounded_generator(c, train):
    sd = seeded_generator_state_dict(5, c["cin"], c["cout"], c["D"], NGF, bias_std=0.05)
    if not train:
        pr.perturb_running(sd)
    x, dout, arch, masks = pr.gen_inputs(c["cin"], c["cout"], c["D"], c["N"], c["H"], c["W"], c["seed"], ngf=NGF)
    state, _ = pr.generator_forward_state(sd, arch, x, train, masks if train else None, c["D"], store=torch.float16)
    return (state, dout) + pr.replays(state, dout, True, torch.float16)


@pytest.fixture(scope="module")
def rounded_train():
    return _rounded_generator(MUT_G, True)


@pytest.fixture(scope="module")
def rounded_eval():
    return _rounded_generator(MUT_E, False)


@pytest.fixture(scope="module")
def rounded_disc():
    c = MUT_D
    sd = seeded_discriminator_state_dict(5, c["cin"], NGF, c["n_layers"], bias_std=0.05)
    g = torch.Generator().manual_seed(c["seed"])
    x = torch.randn((c["N"], c["cin"], c["H"], c["W"]), generator=g)
    state, logits = pr.discriminator_forward_state(sd, x, True, store=torch.float16)
    dl = (torch.rand(logits.shape, generator=g, dtype=torch.float64) * 2 - 1) / logits.numel()
    return (state, dl) + pr.replays(state, dl, True, torch.float16)


def _under_test(case, mutant=None):
    """the stand-in result: the 16-bit replay of the (right or mutated) plan, its rounding perturbed by another power-of-two S
    (fp16 subnormals move), held by compare() against the right plan's R64 / R16 / d_U.  S / 64 with batch statistics; S / 2 with
    running statistics, where no 1 / sigma of a small batch amplifies the gradients and S itself already leaves some subnormal"""
    state, dout, r64, r16, d_u, _ = case
    if state["kind"] == "pix2pix_g":
        S = pr.loss_scale(state["N"], state["H"], state["W"])
        S = S / 64 if state["levels"][2]["train_stats"] else S / 2
        got = pr.flat(pr.replay_generator(state, dout, True, torch.float16, S=S, mutant=mutant))
    else:
        S = float(2 ** round(math.log2(dout.numel())))
        got = pr.flat(pr.replay_discriminator(state, dout, True, torch.float16, S=S / 64, mutant=mutant))
    return pr.compare(got, r64, r16, d_u)


@pytest.mark.parametrize("which", ["train", "eval", "disc"])
def test_bound_passes_a_right_backward(which, request):
    case = request.getfixturevalue("rounded_" + which)
    _, _, r64, _, d_u, _ = case
    rep, bad = _under_test(case)
    assert not bad, {k: rep[k] for k in bad}
    for k in r64:
        assert d_u[k] <= rep[k]["e16"], (k, d_u[k], rep[k]["e16"])
    if which == "train":
        state = case[0]
        assert sum(u["keep"] is not None and u["kscale"] == 2.0 for u in state["ups"].values()) == 1
        assert "darch" in r64 and "dx" in r64


@pytest.mark.parametrize("mutant", pr.MUTANTS_G)
def test_generator_bound_catches(mutant, request):
    case = request.getfixturevalue("rounded_eval" if mutant in EVAL_ONLY else "rounded_train")
    rep, bad = _under_test(case, mutant)
    assert bad, f"{mutant}: inside 4 * e16 + d_U on every tensor"


@pytest.mark.parametrize("mutant", pr.MUTANTS_D)
def test_discriminator_bound_catches(mutant, rounded_disc):
    rep, bad = _under_test(rounded_disc, mutant)
    assert bad, f"{mutant}: inside 4 * e16 + d_U on every tensor"


def _plant_zero(rec, y):
    """the shift of channel 0 moved so that scale * y + shift is exactly zero at element (0, 0, 0, 0): a sign fp32 cannot decide"""
    rec["shift"] = rec["shift"].clone()
    rec["shift"][0] = -(rec["scale"][0] * y[0, 0, 0, 0])
    return rec["shift"][0].item()


@pytest.mark.parametrize("where", ["down", "up", "mid"])
def test_undecided_signs_and_forced_replays(where):
    """undecided() finds a planted zero pre-activation and nothing else, and the forced-on / forced-off replays are the replays of
    the state with that pre-activation just above / just below zero (the shift enters the backward through the sign alone), for
    both consumers of a down level, for an up block and for a discriminator stage: d_U is the distance between the two"""
    if where == "mid":
        sd = seeded_discriminator_state_dict(5, 2, NGF, 3, bias_std=0.05)
        g = torch.Generator().manual_seed(8)
        state, logits = pr.discriminator_forward_state(sd, torch.randn((2, 2, 64, 64), generator=g), True)
        dout = (torch.rand(logits.shape, generator=g, dtype=torch.float64) * 2 - 1) / logits.numel()
        key, rec, fn = ("mid", 2), state["recs"][2], pr.replay_discriminator
        y = rec["y"]
    else:
        sd = seeded_generator_state_dict(5, 1, 1, 5, NGF, bias_std=0.05)
        x, dout, arch, _ = pr.gen_inputs(1, 1, 5, 2, 32, 32, seed=8, ngf=NGF)
        state, _ = pr.generator_forward_state(sd, arch, x, True, None, 5)
        key, fn = (where, 2), pr.replay_generator
        rec = state["levels"][2] if where == "down" else state["ups"][2]
        y = rec["y"] if where == "down" else rec["u"]
    assert pr.undecided(state) == ({}, 0)
    s0 = _plant_zero(rec, y)
    masks, n = pr.undecided(state)
    assert n == 1 and set(masks) == {key} and bool(masks[key][0, 0, 0, 0])
    on, off = (pr.flat(fn(state, dout, True, force=(masks, f))) for f in (True, False))
    tiny = 1e-5 * max(abs(s0), 1e-3)               # clear of SIGN_MARGIN, far below the other pre-activations
    for nudged, forced in ((s0 + tiny, on), (s0 - tiny, off)):
        rec["shift"][0] = nudged
        assert pr.undecided(state) == ({}, 0)
        plain = pr.flat(fn(state, dout, True))
        for k in plain:
            assert torch.equal(plain[k], forced[k]), k
    rec["shift"][0] = s0
    r64, _, d_u, n_und = pr.replays(state, dout, True, torch.float16)
    assert n_und == 1 and max(d_u.values()) > 0
    for k in r64:
        assert abs(d_u[k] - float((on[k] - off[k]).norm()) / float(r64[k].norm())) <= 1e-12 * max(d_u[k], 1e-30), k


# ================================================================================================ adapters
def _nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt)


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b), (path, set(a) ^ set(b))
        for k in a:
            _same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)) and a and (torch.is_tensor(a[0]) or isinstance(a[0], dict)):
        assert len(a) == len(b), path
        for i, (p, q) in enumerate(zip(a, b)):
            _same(p, q, f"{path}[{i}]")
    elif torch.is_tensor(a):
        assert a.shape == b.shape and torch.equal(a, b), path
    else:
        assert a == b, (path, a, b)


def _coef32(rec):
    if rec["scale"] is None:
        return None
    return torch.stack([rec["scale"], rec["shift"], rec["mean"], rec["invstd"]]).float()


def _as_generator_ctx(state, dt):
    """the plain state laid out as GeneratorEngine lays its own out: NHWC 16-bit; R[k] 2c wide with the skip half at offset 0 and
    the up half at offset c (R[D]: c wide); the image layer's u padded to cpad = 8 channels (the padding is not zero here, so the
    adapter must cut it); keep masks uint8 NHWC; parts = (conv, downnorm, cell, upnorm, drop) per block depth"""
    g = torch.Generator().manual_seed(1)
    D, N = state["D"], state["N"]
    params, parts = [], []

    def P(name, t):
        t = t.float()
        params.append((name, t))
        return t

    def norm(bnkey, C):
        return None if bnkey is None else SimpleNamespace(weight=P(bnkey + ".weight", torch.ones(C)), bias=P(bnkey + ".bias", torch.zeros(C)))

    for d in range(D):
        lv, u = state["levels"][d + 1], state["ups"][d]
        conv = SimpleNamespace(weight=P(lv["wkey"], lv["w"]))
        prims = [SimpleNamespace(op=SimpleNamespace(weight=P(u["wkeys"][j], u["w"][j]),
                                                    bias=None if u["b"] is None else P(u["bkeys"][j], u["b"][j]))) for j in range(3)]
        cell = SimpleNamespace(_ops=SimpleNamespace(_ops=prims), _layer_index=u["li"])
        parts.append((conv, norm(lv["bnkey"], lv["w"].shape[0]), cell, norm(u["bnkey"], u["w"][0].shape[1]), None))
    levels, L, R, ups = [None] * (D + 1), [None] * (D + 1), [None] * (D + 1), [None] * D
    for k in range(1, D + 1):
        lv = state["levels"][k]
        levels[k] = dict(y=_nhwc(lv["y"], dt), coef=_coef32(lv), stats=lv["train_stats"])
        if k > 1:
            L[k - 1] = _nhwc(lv["inp"], dt)
        rin = state["ups"][k - 1]["rin"]
        if k < D:
            c = rin.shape[1] // 2
            buf = torch.empty((N, rin.shape[2], rin.shape[3], 2 * c), dtype=dt)
            buf[..., :c], buf[..., c:] = _nhwc(rin[:, :c], dt), _nhwc(rin[:, c:], dt)
            R[k] = buf
        else:
            R[k] = _nhwc(rin, dt)
    for d in range(D):
        u = state["ups"][d]
        cout = u["u"].shape[1]
        info = dict(sm=u["sm"].float(), cin=u["rin"].shape[1], cout=cout, li=u["li"])
        if d == 0:
            pad = torch.rand((N, 8 - cout) + u["u"].shape[2:], generator=g, dtype=torch.float64) + 1.0
            info.update(u=_nhwc(torch.cat([u["u"], pad], 1), dt), cpad=8)
        else:
            keep = None if u["keep"] is None else u["keep"].permute(0, 2, 3, 1).contiguous().to(torch.uint8)
            info.update(u=_nhwc(u["u"], dt), coef=_coef32(u), stats=u["train_stats"], keep=keep, kscale=u["kscale"])
        ups[d] = info
    x = state["levels"][1]["inp"].float()
    c = [x.shape[1]] + [state["levels"][k]["w"].shape[0] for k in range(1, D + 1)]
    ctx = dict(N=N, D=D, c=c, hs=[state["H"] >> k for k in range(D + 1)], ws=[state["W"] >> k for k in range(D + 1)], parts=parts,
               x=x, levels=levels, ups=ups, R=R, L=L)
    eng = SimpleNamespace(tdt=dt, param_names=lambda: [n for n, _ in params], param_list=lambda: [p for _, p in params])
    return eng, ctx


@pytest.mark.parametrize("cfg", [(1, 1, 6, "f16", True), (3, 3, 5, "bf16", False)], ids=lambda c: f"i{c[0]}o{c[1]}_d{c[2]}_{c[3]}")
def test_generator_adapter_round_trip(cfg):
    """CPU tensors in the engine's layouts -- NHWC, channel offsets of the concat buffers, the padded image layer, uint8 masks -- come
    back as the plain state they were made from"""
    cin, cout, D, dtn, train = cfg
    dt = pr.DT[dtn]
    sd = seeded_generator_state_dict(2, cin, cout, D, NGF, bias_std=0.05)
    x, _, arch, masks = pr.gen_inputs(cin, cout, D, 2, 64, 1 << D, seed=6, ngf=NGF)
    state, _ = pr.generator_forward_state(pr.perturb_running(sd), arch, x, train, masks, D, store=dt)
    eng, ctx = _as_generator_ctx(state, dt)
    _same(state, pr.state_from_generator_ctx(eng, ctx, arch))


@pytest.mark.parametrize("cfg", [(2, 3, "f16"), (4, 2, "bf16")], ids=lambda c: f"i{c[0]}_l{c[1]}_{c[2]}")
def test_discriminator_adapter_round_trip(cfg):
    cin, n_layers, dtn = cfg
    dt = pr.DT[dtn]
    sd = seeded_discriminator_state_dict(2, cin, NGF, n_layers, bias_std=0.05)
    x = torch.randn((2, cin, 48, 80), generator=torch.Generator().manual_seed(6))
    state, _ = pr.discriminator_forward_state(sd, x, True, store=dt)
    recs = []
    for r in state["recs"]:
        conv = SimpleNamespace(weight=r["w"].float(), bias=None if r["b"] is None else r["b"].float())
        rec = dict(kind=r["kind"], conv=conv, k=r["k"], s=r["s"], p=r["p"], name=r["name"])
        if r["kind"] == "first":
            rec.update(x=r["x"].float(), z=_nhwc(r["z"], dt))
        elif r["kind"] == "mid":
            rec.update(inp=_nhwc(r["inp"], dt), y=_nhwc(r["y"], dt), coef=_coef32(r), stats=r["train_stats"], bnname=r["bnname"])
        else:
            rec.update(inp=_nhwc(r["inp"], dt))
        recs.append(rec)
    ctx = dict(recs=recs, N=state["N"], H=state["H"], W=state["W"])
    _same(state, pr.state_from_discriminator_ctx(SimpleNamespace(tdt=dt), ctx))
