"""fp64 statement of InstanceNorm on the Pix2Pix engines (`--norm instance`): the three kernels of csrc/instnorm.hip and the whole
generator and PatchGAN, forward and hand-derived backward, in the style of pix2pix_backward_replay.py (whose plain-state layout,
order of steps and helpers it shares; read that module's header first).

What differs from the BatchNorm statement:
  * a normed stage keeps mean / invstd per (sample, channel), [N, C], taken over the H x W plane of the STORED 16-bit conv output
    (gs_in_stats reads what the conv wrote), biased variance, invstd = 1 / sqrt(var + 1e-5); train and eval alike; no parameters.
  * xh = (y - mean) * invstd; g = act'(xh) * keep * kscale * dz_a + act_b'(xh) * dz_b;
    dy = invstd * (g - mean_plane(g) - xh * mean_plane(g * xh)).
  * every conv has a bias.  One directly in front of a norm cancels: with store=dt (the engine's plan) the conv does not add it and
    the engine returns exact zeros for its gradient; the statement computes sum(dy) (zero up to rounding) and reports sum |dy| of
    the stage as `bias_scale`, for compare3d's absolute bound.  With store=None (the reference's arithmetic) the bias IS added.
    The other biases (outermost / innermost down conv, the image cell, the PatchGAN's first and last conv) are real.

  in_stats64 / in_act_apply64 / in_act_bwd64                  the three kernels on NCHW fp64 tensors
  generator_forward_state / discriminator_forward_state       CPU forward -> (plain state, image / logits); store=dt rounds every
                                                              tensor the engine stores in 16 bits, the statistics to fp32
  state_from_generator_ctx / state_from_discriminator_ctx     GPU ctx -> the same plain state
  replay_generator / replay_discriminator / replays           the backward; R64, R16, d_U, undecided count, bias_scale
Mutants (one stated wrong implementation each): FWD_MUTANTS change the forward, BWD_MUTANTS the backward; those that live at one
place live at the deepest normed down level (D - 1, the 2 x 2 plane of the smallest image) -- the place the bound is least sure of."""
import math

import torch
import torch.nn.functional as F
from torch.nn import grad as G

from tests.backward_replay import FLOOR32, SIGN_MARGIN, compare, compare3d, d64, loss_scale, nchw, record  # noqa: F401
from tests.exact_reference import act_bwd64, act_fwd64
from tests.pix2pix_backward_replay import _d_u, _forced, _rounders, block_names, flat, gen_inputs, merged_kernel  # noqa: F401

IN_EPS = 1e-5
FWD_MUTANTS = ("batch_stats", "unbiased_var", "no_eps", "innermost_bias_not_added")
BWD_MUTANTS = ("drop_mean_gxh", "drop_mean_g", "keep_not_in_means", "drop_second_consumer", "second_as_relu", "no_bias_grad")


def _pl(t):
    """[N, C] -> [N, C, 1, 1]"""
    return t[:, :, None, None]


# ------------------------------------------------------------------------------------------------ the three kernels
def in_stats64(y, eps=IN_EPS, mutant=None):
    """(mean, invstd), [N, C] each, of y [N, C, H, W]"""
    if mutant == "batch_stats":
        mean = y.mean((0, 2, 3), keepdim=True).expand(y.shape[0], -1, 1, 1)[:, :, 0, 0]
        var = y.var((0, 2, 3), unbiased=False, keepdim=True).expand(y.shape[0], -1, 1, 1)[:, :, 0, 0]
    else:
        mean, var = y.mean((2, 3)), y.var((2, 3), unbiased=(mutant == "unbiased_var"))
    return mean, torch.rsqrt(var + (0.0 if mutant == "no_eps" else eps))


def in_act_apply64(y, mean, invstd, act, keep=None, kscale=1.0):
    z = act_fwd64((y - _pl(mean)) * _pl(invstd), act)
    return z if keep is None else z * keep * kscale


def in_act_bwd64(y, mean, invstd, dz_a, act, dz_b=None, act_b="none", keep=None, kscale=1.0, mutant=None, v=None):
    """(dy, mean_plane(g), mean_plane(g * xh)).  v: the pre-activation whose sign decides (default xh itself)"""
    xh = (y - _pl(mean)) * _pl(invstd)
    v = xh if v is None else v
    ga = act_bwd64(dz_a, v, act)
    g = ga if keep is None else ga * keep * kscale
    gm = ga if (mutant == "keep_not_in_means" and keep is not None) else g
    if dz_b is not None and mutant != "drop_second_consumer":
        gb = act_bwd64(dz_b, v, "relu" if mutant == "second_as_relu" else act_b)
        g, gm = g + gb, gm + gb
    m1, m2 = gm.mean((2, 3)), (gm * xh).mean((2, 3))
    if mutant == "drop_mean_g":
        m1 = torch.zeros_like(m1)
    if mutant == "drop_mean_gxh":
        m2 = torch.zeros_like(m2)
    return _pl(invstd) * (g - _pl(m1) - xh * _pl(m2)), m1, m2


# ------------------------------------------------------------------------------------------------ CPU forward states
def _stats(y, r32, mutant):
    mean, invstd = in_stats64(y, IN_EPS, mutant if mutant in ("batch_stats", "unbiased_var", "no_eps") else None)
    return r32(mean), r32(invstd)


def generator_forward_state(sd, arch, x, dropout_masks, num_downs, store=None, mutant=None):
    """networks.UnetGenerator under InstanceNorm on the CPU -> (plain state, image).  dropout_masks: NCHW keep masks, the block
    next to the innermost first, applied with kscale = 2 (None: no dropout -- eval mode, or train without it)."""
    assert mutant is None or mutant in FWD_MUTANTS
    sd = {k: v.double() for k, v in sd.items()}
    x, arch = x.double(), arch.detach().double()
    r16, r32 = _rounders(store)
    D = num_downs
    N, _, H, W = x.shape
    nm = block_names(D)
    levels, ups, Ls, skips = {}, {}, {0: x}, {}
    for k in range(1, D + 1):
        conv = nm[k - 1]["conv"]
        w, b = sd[conv + ".weight"], sd[conv + ".bias"]
        normed = 1 < k < D
        add = (not normed or store is None) and not (k == D and mutant == "innermost_bias_not_added")
        yfull = F.conv2d(Ls[k - 1], w if k == 1 else r16(w), b if add else None, stride=2, padding=1)
        lv = dict(y=r16(yfull), w=w, wd=r16(w), b=b, inp=Ls[k - 1], wkey=conv + ".weight", bkey=conv + ".bias", normed=normed,
                  mean=None, invstd=None)
        v = lv["y"]
        if normed:
            lv["mean"], lv["invstd"] = _stats(lv["y"], r32, mutant)
            v = (lv["y"] - _pl(lv["mean"])) * _pl(lv["invstd"])
        levels[k] = lv
        Ls[k], skips[k] = r16(F.leaky_relu(v, 0.2)), r16(v.clamp_min(0))
    rin, out = skips[D], None
    for d in range(D - 1, -1, -1):
        cell = nm[d]["cell"]
        li = D - 1 - d
        sm = r32(torch.softmax(arch[li] if store is None else arch[li].float(), -1).double())
        prims = [cell + f"._ops._ops.{j}.op" for j in range(3)]
        normed = d > 0
        rec = dict(keep=None, kscale=1.0, sm=sm, li=li, w=[sd[p + ".weight"] for p in prims], b=[sd[p + ".bias"] for p in prims],
                   rin=rin, wkeys=[p + ".weight" for p in prims], bkeys=[p + ".bias" for p in prims], normed=normed,
                   mean=None, invstd=None)
        bias = sum(sm[j] * rec["b"][j] for j in range(3)) if (not normed or store is None) else None
        ufull = F.conv_transpose2d(rin, r16(merged_kernel(rec)), bias, stride=2, padding=3)
        rec["u"] = r16(ufull)
        ups[d] = rec
        if d == 0:
            out = torch.tanh(ufull)
            break
        rec["mean"], rec["invstd"] = _stats(rec["u"], r32, mutant)
        if 1 <= li <= D - 5 and dropout_masks is not None:
            rec["keep"], rec["kscale"] = dropout_masks[li - 1].double(), 2.0
        up = in_act_apply64(rec["u"], rec["mean"], rec["invstd"], "relu", rec["keep"], rec["kscale"])
        rin = torch.cat([skips[d], r16(up)], 1)
    return dict(kind="pix2pix_g_in", N=N, H=H, W=W, D=D, arch_shape=tuple(arch.shape), levels=levels, ups=ups), out


def discriminator_forward_state(sd, x, store=None, mutant=None):
    """networks.NLayerDiscriminator under InstanceNorm on the CPU -> (plain state, logits); n_layers from the keys of sd"""
    sd = {k: v.double() for k, v in sd.items()}
    x = x.double()
    r16, r32 = _rounders(store)
    convs = sorted(int(k.split(".")[1]) for k in sd if k.endswith(".weight"))
    n_layers = len(convs) - 2
    N, _, H, W = x.shape
    w, b = sd["model.0.weight"], sd["model.0.bias"]
    z = r16(F.leaky_relu(F.conv2d(x, w, b, stride=2, padding=1), 0.2))
    recs = [dict(kind="first", name="model.0", k=4, s=2, p=1, w=w, b=b, x=x, z=z)]
    cur = z
    for n, i in enumerate(convs[1:-1], 1):
        s = 2 if n < n_layers else 1
        w, b = sd[f"model.{i}.weight"], sd[f"model.{i}.bias"]
        yfull = F.conv2d(cur, r16(w), b if store is None else None, stride=s, padding=1)
        if yfull.shape[2] * yfull.shape[3] < 2:
            raise ValueError(f"Expected more than 1 spatial element when training, got input size {list(yfull.shape)}")
        rec = dict(kind="mid", name=f"model.{i}", k=4, s=s, p=1, w=w, b=b, inp=cur, y=r16(yfull), wd=r16(w))
        rec["mean"], rec["invstd"] = _stats(rec["y"], r32, mutant)
        recs.append(rec)
        cur = r16(in_act_apply64(rec["y"], rec["mean"], rec["invstd"], "leaky"))
    i = convs[-1]
    w, b = sd[f"model.{i}.weight"], sd[f"model.{i}.bias"]
    recs.append(dict(kind="last", name=f"model.{i}", k=4, s=1, p=1, w=w, b=b, inp=cur))
    return dict(kind="pix2pix_d_in", N=N, H=H, W=W, recs=recs), F.conv2d(cur, w, b, stride=1, padding=1)


# ------------------------------------------------------------------------------------------------ adapters (GPU ctx -> plain state)
def _mi(inorm):
    return (None, None) if inorm is None else (d64(inorm[0]), d64(inorm[1]))


def state_from_generator_ctx(engine, ctx, arch):
    dt = engine.tdt
    names = {id(p): n for n, p in zip(engine.param_names(), engine.param_list())}
    N, D, parts, R, L = ctx["N"], ctx["D"], ctx["parts"], ctx["R"], ctx["L"]
    levels, ups = {}, {}
    for k in range(1, D + 1):
        lv, conv = ctx["levels"][k], parts[k - 1][0]
        w = d64(conv.weight)
        mean, invstd = _mi(lv.get("inorm"))
        levels[k] = dict(y=nchw(lv["y"]), w=w, wd=w.to(dt).double(), b=d64(conv.bias), wkey=names[id(conv.weight)],
                         bkey=names[id(conv.bias)], inp=d64(ctx["x"]) if k == 1 else nchw(L[k - 1]), normed=mean is not None,
                         mean=mean, invstd=invstd)
    for d in range(D):
        info, cell = ctx["ups"][d], parts[d][2]
        prims = [cell._ops._ops[j].op for j in range(3)]
        keep = info.get("keep")
        mean, invstd = _mi(info.get("inorm"))
        ups[d] = dict(u=nchw(info["u"], info["cout"]), keep=None if keep is None else nchw(keep), kscale=float(info.get("kscale", 1.0)),
                      sm=d64(info["sm"]), li=int(info["li"]), w=[d64(o.weight) for o in prims], b=[d64(o.bias) for o in prims],
                      rin=nchw(R[d + 1]), wkeys=[names[id(o.weight)] for o in prims], bkeys=[names[id(o.bias)] for o in prims],
                      normed=mean is not None, mean=mean, invstd=invstd)
    return dict(kind="pix2pix_g_in", N=N, H=ctx["hs"][0], W=ctx["ws"][0], D=D, arch_shape=tuple(arch.shape), levels=levels, ups=ups)


def state_from_discriminator_ctx(engine, ctx):
    dt = engine.tdt
    recs = []
    for r in ctx["recs"]:
        conv = r["conv"]
        w = d64(conv.weight)
        rec = dict(kind=r["kind"], name=r["name"], k=r["k"], s=r["s"], p=r["p"], w=w, b=d64(conv.bias))
        if r["kind"] == "first":
            rec.update(x=d64(r["x"]), z=nchw(r["z"]))
        elif r["kind"] == "mid":
            mean, invstd = _mi(r["inorm"])
            rec.update(inp=nchw(r["inp"]), y=nchw(r["y"]), wd=w.to(dt).double(), mean=mean, invstd=invstd)
        else:
            rec.update(inp=nchw(r["inp"]))
        recs.append(rec)
    return dict(kind="pix2pix_d_in", N=ctx["N"], H=ctx["H"], W=ctx["W"], recs=recs)


# ------------------------------------------------------------------------------------------------ the backward
def _xh(rec, y):
    return (y - _pl(rec["mean"])) * _pl(rec["invstd"])


def replay_generator(state, dout, need_dx, store=None, S=None, mutant=None, force=None):
    """generator_backward under InstanceNorm in fp64 -> ({state-dict name: gradient}, darch, dx or None, bias_scale)"""
    assert mutant is None or mutant in BWD_MUTANTS
    N, H, W, D = state["N"], state["H"], state["W"], state["D"]
    S = loss_scale(N, H, W) if S is None else S
    levels, ups = state["levels"], state["ups"]
    grads, bias_scale = {}, {}
    darch = torch.zeros(state["arch_shape"], dtype=torch.float64)
    rnd = (lambda t: t) if store is None else (lambda t: (t * S).to(store).double() / S)
    mut_level = D - 1

    def upconv_bwd(d, du):
        rec = ups[d]
        rin, sm = rec["rin"], rec["sm"]
        w4, w6, w8 = rec["w"]
        dwm = G.conv2d_weight(du, w8.shape, rin, stride=2, padding=3)
        grads[rec["wkeys"][0]] = sm[0] * dwm[:, :, 2:6, 2:6]
        grads[rec["wkeys"][1]] = sm[1] * dwm[:, :, 1:7, 1:7]
        grads[rec["wkeys"][2]] = sm[2] * dwm
        dots = torch.stack([(dwm[:, :, 2:6, 2:6] * w4).sum(), (dwm[:, :, 1:7, 1:7] * w6).sum(), (dwm * w8).sum()])
        dbm = du.sum((0, 2, 3))
        for j in range(3):
            grads[rec["bkeys"][j]] = sm[j] * dbm
            if rec["normed"]:
                bias_scale[rec["bkeys"][j]] = float(sm[j] * du.abs().sum())
            elif mutant == "no_bias_grad":
                grads[rec["bkeys"][j]] = torch.zeros_like(dbm)
        dots = dots + torch.stack([(dbm * rec["b"][j]).sum() for j in range(3)])       # (zero up to rounding in front of a norm)
        darch[rec["li"]] = sm * (dots - (sm * dots).sum())
        wm = merged_kernel(rec)
        if store is not None:
            wm = wm.to(store).double()
        return rnd(F.conv2d(du, wm, None, stride=2, padding=3))

    dtl = rnd(dout.double())
    du = rnd(dtl * (1.0 - torch.tanh(ups[0]["u"]) ** 2))
    dR = {1: upconv_bwd(0, du)}
    for d in range(1, D):
        rec = ups[d]
        cd = dR[d].shape[1] // 2
        v = _forced(_xh(rec, rec["u"]), force, ("up", d))
        du = rnd(in_act_bwd64(rec["u"], rec["mean"], rec["invstd"], dR[d][:, cd:], "relu", keep=rec["keep"], kscale=rec["kscale"],
                              mutant=mutant if mutant == "keep_not_in_means" else None, v=v)[0])
        dR[d + 1] = upconv_bwd(d, du)

    dL = dx = None
    for k in range(D, 0, -1):
        lv = levels[k]
        y = lv["y"]
        if lv["normed"]:
            v = _forced(_xh(lv, y), force, ("down", k))
            ck = dR[k].shape[1] // 2
            dy = rnd(in_act_bwd64(y, lv["mean"], lv["invstd"], dR[k][:, :ck], "relu", dz_b=dL, act_b="leaky",
                                  mutant=mutant if k == mut_level else None, v=v)[0])
        elif k == D:
            dy = rnd(act_bwd64(dR[k], y, "relu"))
        else:                                                              # level 1: no norm, both consumers
            ck = dR[k].shape[1] // 2
            dy = rnd(act_bwd64(dR[k][:, :ck], y, "relu") + act_bwd64(dL, y, "leaky"))
        grads[lv["wkey"]] = G.conv2d_weight(lv["inp"], lv["w"].shape, dy, stride=2, padding=1)
        grads[lv["bkey"]] = dy.sum((0, 2, 3))
        if lv["normed"]:
            bias_scale[lv["bkey"]] = float(dy.abs().sum())
        elif mutant == "no_bias_grad":
            grads[lv["bkey"]] = torch.zeros_like(grads[lv["bkey"]])
        if k > 1:
            dL = rnd(G.conv2d_input(lv["inp"].shape, lv["wd"], dy, stride=2, padding=1))
        elif need_dx:
            dx = G.conv2d_input(lv["inp"].shape, lv["w"], dy, stride=2, padding=1)
    return grads, darch, dx, bias_scale


def replay_discriminator(state, dlogits, need_dx, store=None, S=None, mutant=None, force=None):
    """DiscriminatorEngine.backward under InstanceNorm in fp64 -> ({name: gradient}, dx or None, bias_scale)"""
    assert mutant is None or mutant in BWD_MUTANTS
    dl = dlogits.double()
    S = float(2 ** round(math.log2(max(dl.numel(), 1)))) if S is None else S
    rnd = (lambda t: t) if store is None else (lambda t: (t * S).to(store).double() / S)
    recs = state["recs"]
    grads, bias_scale = {}, {}
    last = recs[-1]
    grads[last["name"] + ".weight"] = G.conv2d_weight(last["inp"], last["w"].shape, dl, stride=last["s"], padding=last["p"])
    grads[last["name"] + ".bias"] = dl.sum((0, 2, 3))
    dz = rnd(G.conv2d_input(last["inp"].shape, last["w"], dl, stride=last["s"], padding=last["p"]))
    mut_i = len(recs) - 2                                                  # the last normed stage: the smallest plane
    for i in range(len(recs) - 2, 0, -1):
        rec = recs[i]
        v = _forced(_xh(rec, rec["y"]), force, ("mid", i))
        dy = rnd(in_act_bwd64(rec["y"], rec["mean"], rec["invstd"], dz, "leaky", mutant=mutant if i == mut_i else None, v=v)[0])
        grads[rec["name"] + ".weight"] = G.conv2d_weight(rec["inp"], rec["w"].shape, dy, stride=rec["s"], padding=rec["p"])
        grads[rec["name"] + ".bias"] = dy.sum((0, 2, 3))
        bias_scale[rec["name"] + ".bias"] = float(dy.abs().sum())
        dz = rnd(G.conv2d_input(rec["inp"].shape, rec["wd"], dy, stride=rec["s"], padding=rec["p"]))
    first = recs[0]
    dy = rnd(act_bwd64(dz, first["z"], "leaky"))
    grads[first["name"] + ".weight"] = G.conv2d_weight(first["x"], first["w"].shape, dy, stride=first["s"], padding=first["p"])
    grads[first["name"] + ".bias"] = dy.sum((0, 2, 3))
    if mutant == "no_bias_grad":
        for r in (first, last):
            grads[r["name"] + ".bias"] = torch.zeros_like(grads[r["name"] + ".bias"])
    dx = G.conv2d_input(first["x"].shape, first["w"], dy, stride=first["s"], padding=first["p"]) if need_dx else None
    return grads, dx, bias_scale


# ------------------------------------------------------------------------------------------------ undecided signs, replays
def undecided(state):
    """{stage key: mask} of the elements whose sign of y - mean fp32 cannot decide (SIGN_MARGIN of |y| + |mean|), and their count.
    Stages without a norm read the stored sign."""
    if state["kind"] == "pix2pix_g_in":
        items = [(("down", k), lv, lv["y"]) for k, lv in state["levels"].items() if lv["normed"]]
        items += [(("up", d), u, u["u"]) for d, u in state["ups"].items() if u["normed"]]
    else:
        items = [(("mid", i), r, r["y"]) for i, r in enumerate(state["recs"]) if r["kind"] == "mid"]
    masks, n = {}, 0
    for key, rec, y in items:
        mu = _pl(rec["mean"])
        m = (y - mu).abs() < SIGN_MARGIN * (y.abs() + mu.abs())
        if bool(m.any()):
            masks[key] = m
            n += int(m.sum())
    return masks, n


def flat_in(res):
    """(grads, darch, dx, bias_scale) / (grads, dx, bias_scale) as one dict plus the bias scales"""
    return flat(res[:-1]), res[-1]


def replays(state, dout, need_dx, store, S=None):
    """(R64, R16, d_U per tensor, count of undecided elements, bias_scale): what compare3d() needs"""
    fn = replay_generator if state["kind"] == "pix2pix_g_in" else replay_discriminator
    r64, bias_scale = flat_in(fn(state, dout, need_dx, None, S))
    r16, _ = flat_in(fn(state, dout, need_dx, store, S))
    masks, n_und = undecided(state)
    d_u = {k: 0.0 for k in r64}
    if n_und:
        d_u = _d_u(r64, flat_in(fn(state, dout, need_dx, None, S, force=(masks, True)))[0],
                   flat_in(fn(state, dout, need_dx, None, S, force=(masks, False)))[0])
    return r64, r16, d_u, n_und, bias_scale


def hold(got, rp, dt):
    """compare3d of a result with replays(): (report, failures)"""
    r64, r16, d_u, _, bias_scale = rp
    return compare3d(got, r64, r16, d_u, bias_scale, dt)


def rel_err(a, ref):
    return float((a.double() - ref).norm()) / float(ref.norm())


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
# Shared with the CPU tests, which prove on these very seeds that the bound tells every mutant from a right implementation.
# fixture: weights, image and arch of tests/golden/pix2pix_instance_{a,b}.npz (golden_util_instance.FIXTURES); otherwise seeded here.
G_CASES = {
    "g5_32": dict(cin=1, cout=1, D=5, N=3, H=32, W=32, dtype="f16", seed=11, fixture=None),
    "g6_64_a": dict(cin=1, cout=1, D=6, N=2, H=64, W=64, dtype="f16", seed=11, fixture="pix2pix_instance_a"),
    "g5_32x64_b": dict(cin=3, cout=3, D=5, N=3, H=32, W=64, dtype="f16", seed=11, fixture="pix2pix_instance_b"),
    "g5_32_bf16": dict(cin=1, cout=1, D=5, N=3, H=32, W=32, dtype="bf16", seed=16, fixture=None),
}
D_CASES = {
    "d2_32": dict(cin=2, n_layers=2, N=2, H=32, W=32, dtype="f16", seed=11, fixture=None),
    "d3_32": dict(cin=2, n_layers=3, N=2, H=32, W=32, dtype="f16", seed=11, fixture=None),
    "d3_64_a": dict(cin=2, n_layers=3, N=2, H=64, W=64, dtype="f16", seed=11, fixture="pix2pix_instance_a"),
}
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def generator_case(c):
    """(state dict, image x, arch, dout, keep masks [NCHW, the block next to the innermost first]) of a generator case"""
    from golden_util_instance import FIXTURES, fixture_inputs, seeded_generator_state_dict_instance
    _, dout, arch, masks = gen_inputs(c["cin"], c["cout"], c["D"], c["N"], c["H"], c["W"], c["seed"])
    if c["fixture"]:
        f = FIXTURES[c["fixture"]]
        sd = seeded_generator_state_dict_instance(f["seed_g"], c["cin"], c["cout"], c["D"], 64)
        x, _, arch = fixture_inputs(f)
    else:
        sd = seeded_generator_state_dict_instance(c["seed"], c["cin"], c["cout"], c["D"], 64)
        x = gen_inputs(c["cin"], c["cout"], c["D"], c["N"], c["H"], c["W"], c["seed"])[0]
    return sd, x, arch, dout, masks


def discriminator_case(c, golden=None):
    """(state dict, input x) of a discriminator case; a fixture case reads cat(input, image) of the loaded fixture `golden`"""
    from golden_util_instance import FIXTURES, INPUT_STD, seeded_discriminator_state_dict_instance
    if c["fixture"]:
        f = FIXTURES[c["fixture"]]
        sd = seeded_discriminator_state_dict_instance(f["seed_d"], c["cin"], 64, c["n_layers"])
        x = torch.cat((torch.from_numpy(golden["input"]), torch.from_numpy(golden["image"])), 1).float()
    else:
        sd = seeded_discriminator_state_dict_instance(c["seed"], c["cin"], 64, c["n_layers"])
        x = INPUT_STD * torch.randn((c["N"], c["cin"], c["H"], c["W"]), generator=torch.Generator().manual_seed(c["seed"]))
    return sd, x


def dlogits_of(logits, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return (torch.rand(logits.shape, generator=g, dtype=torch.float64) * 2 - 1) / logits.numel()
