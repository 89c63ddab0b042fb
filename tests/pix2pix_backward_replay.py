"""fp64 replay of the Pix2Pix engines' backward plans from the state their forward saved.

`generator_backward(engine, ctx, arch, dout, need_dx)` (models_pix2pix/pix2pix_backward.py) and `DiscriminatorEngine.backward(ctx,
dlogits, need_dx)` (discriminator_engine.py) are pure functions of `ctx` and the incoming gradient, and linear in it.  This module
restates both on the CPU in torch fp64, in the order of those functions, from a PLAIN state (NCHW fp64 tensors: no NHWC, no concat
offsets, no padded image channels, no uint8 masks), as backward_replay.py does for the U-Net engines, and is held with that
module's compare().

  state_from_generator_ctx / state_from_discriminator_ctx     GPU ctx -> plain state (only read tensors)
  generator_forward_state / discriminator_forward_state       the same plain state made on the CPU from a state dict and an image
                                                              (fp64, or with the engines' 16-bit stores when store=dt)
  replay_generator / replay_discriminator                     the backward: every parameter gradient by state-dict name, darch, dx
  undecided / replays / replays_chain                         elements whose activation sign fp32 cannot decide, and what compare()
                                                              needs: R64, R16 and d_U per tensor

The generator's plan, level k = 1..D counted from the image (c_k channels at H / 2^k), block depth d = 0..D-1 from the outside:
  L[k] = leaky(bn(y_k)) feeds down-conv k+1; R[k] = [relu(bn(y_k)) | relu(bn(u_k)) * keep * kscale] feeds the merged transposed conv
  of block k-1, whose output u_{k-1} has the channels of level k-1 (the image at d = 0, then tanh).  R[D] is relu(y_D) alone.
Backward: tanh' from u_0; per block d the merged 8x8 weight gradient dWm, split into dW4 = sm0 * centre 4x4, dW6 = sm1 * centre
6x6, dW8 = sm2 * dWm, the dots <dWm, pad_j(W_j)> (+ <db_m, b_j>), darch[li] = sm * (dots - sum sm * dots), and the data gradient, a
stride-2 conv of du with the un-flipped merged kernel; BatchNorm backward dy = scale * (gh - c1 - xh * c2), c1 = s1 / M, c2 = s2 / M,
both zero for running statistics, where gh sums the ReLU consumer (times keep * kscale on the up path) and, on the down path below
the innermost level, the LeakyReLU consumer.  ReLU'(0) = 0 and leaky'(0) = 0.2 (exact_reference.act_bwd64); tanh' = 1 - tanh(u)^2.
store=dt rounds what the engines keep in 16 bits between launches, as S * value: dt (the incoming gradient), every du, dy, dR and
dL, and the weights of the data gradients (the merged kernel and the down convs, packed in 16 bits).  Never rounded: the fp32 weight
gradients, dots and darch, the bias gradients, dx, and the discriminator's dlogits.  S and 1/S are powers of two."""
import math

import torch
import torch.nn.functional as F
from torch.nn import grad as G

from tests.backward_replay import BN_EPS, DT, FLOOR32, SIGN_MARGIN, compare, d64, loss_scale, nchw, record  # noqa: F401
from tests.exact_reference import act_bwd64

MUTANTS_G = ("drop_leaky_consumer", "leaky_as_relu", "swap_halves", "drop_keep_scale", "ignore_keep", "softmax_no_mean",
             "arch_no_bias_dot", "w6_offset", "flipped_dgrad", "drop_c2", "eval_keeps_c12", "innermost_two_consumers")
MUTANTS_D = ("d_first_bias_border", "d_dx_class_swapped")
MUT_LEVEL, MUT_BLOCK = 2, 1        # the down level / up block at which a mutant that lives at one place is wrong


def _col(t):
    return t.view(1, -1, 1, 1)


def _coef(coef):
    """scale / shift / mean / invstd of a saved coefficient block ([4, C] fp32), or four Nones where the stage has no norm"""
    if coef is None:
        return dict(scale=None, shift=None, mean=None, invstd=None)
    return dict(scale=d64(coef[0]), shift=d64(coef[1]), mean=d64(coef[2]), invstd=d64(coef[3]))


def merged_kernel(rec):
    """sm2 * W8 + sm1 * pad1(W6) + sm0 * pad2(W4): the one k8 / s2 / p3 transposed-conv kernel [cin, cout, 8, 8]"""
    sm, (w4, w6, w8) = rec["sm"], rec["w"]
    return sm[2] * w8 + sm[1] * F.pad(w6, [1, 1, 1, 1]) + sm[0] * F.pad(w4, [2, 2, 2, 2])


def block_names(D):
    """per block depth (0 = outermost) the state-dict prefixes of networks.UnetGenerator: conv, downnorm, cell, upnorm"""
    out, prefix = [], "model"
    for d in range(D):
        p = prefix + ".model"
        if d == 0:
            out.append(dict(conv=p + ".0", downnorm=None, cell=p + ".3", upnorm=None))
            prefix = p + ".1"
        elif d == D - 1:
            out.append(dict(conv=p + ".1", downnorm=None, cell=p + ".3", upnorm=p + ".4"))
        else:
            out.append(dict(conv=p + ".1", downnorm=p + ".2", cell=p + ".5", upnorm=p + ".6"))
            prefix = p + ".3"
    return out


# ------------------------------------------------------------------------------------------------ inputs of a case
def perturb_running(sd, seed=9):
    """running statistics that are not the initial 0 / 1"""
    g = torch.Generator().manual_seed(seed)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
        elif k.endswith("running_var"):
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    return sd


def gen_inputs(cin, cout, D, N, H, W, seed, ngf=64):
    """image, dense dout of magnitude 1 / (N H W), arch [D, 3], NCHW keep masks of the D - 5 dropout blocks (innermost first)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, cin, H, W), generator=g)
    dout = (torch.rand((N, cout, H, W), generator=g, dtype=torch.float64) * 2 - 1) / (N * H * W)
    arch = torch.randn((D, 3), generator=g) * 0.5
    masks = [(torch.rand((N, ngf * 8, H >> (D - 1 - li), W >> (D - 1 - li)), generator=g) >= 0.5).double()
             for li in range(1, D - 4)]
    return x, dout, arch, masks


# ------------------------------------------------------------------------------------------------ adapters
def state_from_generator_ctx(engine, ctx, arch):
    """The saved forward of GeneratorEngine.forward as a plain state."""
    dt = engine.tdt
    names = {id(p): n for n, p in zip(engine.param_names(), engine.param_list())}
    N, D, parts, R, L = ctx["N"], ctx["D"], ctx["parts"], ctx["R"], ctx["L"]
    levels, ups = {}, {}
    for k in range(1, D + 1):
        lv = ctx["levels"][k]
        conv, downnorm = parts[k - 1][0], parts[k - 1][1]
        w = d64(conv.weight)
        levels[k] = dict(y=nchw(lv["y"]), train_stats=bool(lv["stats"]), w=w, wd=w.to(dt).double(),
                         inp=d64(ctx["x"]) if k == 1 else nchw(L[k - 1]), wkey=names[id(conv.weight)],
                         bnkey=None if downnorm is None else names[id(downnorm.weight)][:-len(".weight")], **_coef(lv["coef"]))
    for d in range(D):
        info = ctx["ups"][d]
        cell, upnorm = parts[d][2], parts[d][3]
        prims = [cell._ops._ops[j].op for j in range(3)]
        keep = info.get("keep")
        ups[d] = dict(u=nchw(info["u"], info["cout"]), train_stats=bool(info.get("stats", False)),
                      keep=None if keep is None else nchw(keep), kscale=float(info.get("kscale", 1.0)), sm=d64(info["sm"]),
                      li=int(info["li"]), w=[d64(o.weight) for o in prims],
                      b=None if prims[0].bias is None else [d64(o.bias) for o in prims], rin=nchw(R[d + 1]),
                      wkeys=[names[id(o.weight)] for o in prims],
                      bkeys=None if prims[0].bias is None else [names[id(o.bias)] for o in prims],
                      bnkey=None if upnorm is None else names[id(upnorm.weight)][:-len(".weight")], **_coef(info.get("coef")))
    return dict(kind="pix2pix_g", N=N, H=ctx["hs"][0], W=ctx["ws"][0], D=D, arch_shape=tuple(arch.shape), levels=levels, ups=ups)


def state_from_discriminator_ctx(engine, ctx):
    """The saved forward of DiscriminatorEngine.forward as a plain state: the first / mid / last records in their order."""
    dt = engine.tdt
    recs = []
    for r in ctx["recs"]:
        conv = r["conv"]
        w = d64(conv.weight)
        rec = dict(kind=r["kind"], name=r["name"], k=r["k"], s=r["s"], p=r["p"], w=w,
                   b=None if conv.bias is None else d64(conv.bias))
        if r["kind"] == "first":
            rec.update(x=d64(r["x"]), z=nchw(r["z"]))          # z = leaky(conv + bias): its sign alone gives the activation gradient
        elif r["kind"] == "mid":
            rec.update(inp=nchw(r["inp"]), y=nchw(r["y"]), train_stats=bool(r["stats"]), wd=w.to(dt).double(),
                       bnname=r["bnname"], **_coef(r["coef"]))
        else:
            rec.update(inp=nchw(r["inp"]))
        recs.append(rec)
    return dict(kind="pix2pix_d", N=ctx["N"], H=ctx["H"], W=ctx["W"], recs=recs)


# ------------------------------------------------------------------------------------------------ CPU forward states
def _rounders(store):
    if store is None:
        return (lambda t: t), (lambda t: t)
    return (lambda t: t.to(store).double()), (lambda t: t.float().double())


def _bn_coef(sd, bn, y, train, r32):
    """coefficients from the unrounded conv output, as the conv epilogues take the statistics"""
    if train:
        mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    else:
        mean, var = sd[bn + ".running_mean"], sd[bn + ".running_var"]
    invstd = torch.rsqrt(var + BN_EPS)
    scale = sd[bn + ".weight"] * invstd
    return dict(scale=r32(scale), shift=r32(sd[bn + ".bias"] - mean * scale), mean=r32(mean), invstd=r32(invstd))


def generator_forward_state(sd, arch, x, train, dropout_masks, num_downs, store=None):
    """networks.UnetGenerator's forward on the CPU in fp64 as a plain state.  store=None: nothing is rounded and the statistics are
    exact, so replay_generator() of it must be torch.autograd through the oracle.  store=dt: y, u, L, R and the conv weights
    rounded to dt where the engine stores them, the coefficients and the softmax to fp32.  dropout_masks: NCHW keep masks {0,1},
    the block next to the innermost first (the oracle's order), applied with kscale = 2 in train mode.  Returns (state, image)."""
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x, arch = x.double(), arch.detach().double()
    r16, r32 = _rounders(store)
    D = num_downs
    N, _, H, W = x.shape
    nm = block_names(D)
    levels, ups, Ls, skips = {}, {}, {0: x}, {}
    for k in range(1, D + 1):
        b = nm[k - 1]
        w = sd[b["conv"] + ".weight"]
        yfull = F.conv2d(Ls[k - 1], w if k == 1 else r16(w), None, stride=2, padding=1)       # the image conv reads fp32 weights
        lv = dict(y=r16(yfull), train_stats=False, w=w, wd=r16(w), inp=Ls[k - 1], wkey=b["conv"] + ".weight",
                  bnkey=b["downnorm"], **_coef(None))
        v = lv["y"]
        if b["downnorm"] is not None:
            lv.update(_bn_coef(sd, b["downnorm"], yfull, train, r32), train_stats=bool(train))
            v = lv["y"] * _col(lv["scale"]) + _col(lv["shift"])
        levels[k] = lv
        Ls[k], skips[k] = r16(F.leaky_relu(v, 0.2)), r16(v.clamp_min(0))
    rin, out = skips[D], None
    for d in range(D - 1, -1, -1):
        b = nm[d]
        li = D - 1 - d
        sm = r32(torch.softmax(arch[li] if store is None else arch[li].float(), -1).double())
        prims = [b["cell"] + f"._ops._ops.{j}.op" for j in range(3)]
        has_b = prims[0] + ".bias" in sd
        rec = dict(train_stats=False, keep=None, kscale=1.0, sm=sm, li=li, w=[sd[p + ".weight"] for p in prims],
                   b=[sd[p + ".bias"] for p in prims] if has_b else None, rin=rin, wkeys=[p + ".weight" for p in prims],
                   bkeys=[p + ".bias" for p in prims] if has_b else None, bnkey=b["upnorm"], **_coef(None))
        bias = sum(sm[j] * rec["b"][j] for j in range(3)) if has_b else None
        ufull = F.conv_transpose2d(rin, r16(merged_kernel(rec)), bias, stride=2, padding=3)
        rec["u"] = r16(ufull)
        ups[d] = rec
        if d == 0:
            out = torch.tanh(ufull)
            break
        rec.update(_bn_coef(sd, b["upnorm"], ufull, train, r32), train_stats=bool(train))
        up = (rec["u"] * _col(rec["scale"]) + _col(rec["shift"])).clamp_min(0)
        if 1 <= li <= D - 5 and dropout_masks is not None and train:
            rec["keep"], rec["kscale"] = dropout_masks[li - 1].double(), 2.0
            up = up * rec["keep"] * 2.0
        rin = torch.cat([skips[d], r16(up)], 1)
    state = dict(kind="pix2pix_g", N=N, H=H, W=W, D=D, arch_shape=tuple(arch.shape), levels=levels, ups=ups)
    return state, out


def discriminator_forward_state(sd, x, train, store=None):
    """networks.NLayerDiscriminator's forward on the CPU as a plain state (n_layers from the keys of sd).  Returns (state, logits)."""
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x = x.double()
    r16, r32 = _rounders(store)
    convs = sorted(int(k.split(".")[1]) for k in sd if k.endswith(".weight") and sd[k].dim() == 4)
    n_layers = len(convs) - 2
    N, _, H, W = x.shape
    w, b = sd["model.0.weight"], sd["model.0.bias"]
    z = r16(F.leaky_relu(F.conv2d(x, w, b, stride=2, padding=1), 0.2))
    recs = [dict(kind="first", name="model.0", k=4, s=2, p=1, w=w, b=b, x=x, z=z)]
    cur = z
    for n, i in enumerate(convs[1:-1], 1):
        s = 2 if n < n_layers else 1
        w = sd[f"model.{i}.weight"]
        yfull = F.conv2d(cur, r16(w), None, stride=s, padding=1)
        rec = dict(kind="mid", name=f"model.{i}", k=4, s=s, p=1, w=w, b=None, inp=cur, y=r16(yfull), train_stats=bool(train),
                   wd=r16(w), bnname=f"model.{i + 1}", **_bn_coef(sd, f"model.{i + 1}", yfull, train, r32))
        recs.append(rec)
        cur = r16(F.leaky_relu(rec["y"] * _col(rec["scale"]) + _col(rec["shift"]), 0.2))
    i = convs[-1]
    w, b = sd[f"model.{i}.weight"], sd[f"model.{i}.bias"]
    recs.append(dict(kind="last", name=f"model.{i}", k=4, s=1, p=1, w=w, b=b, inp=cur))
    return dict(kind="pix2pix_d", N=N, H=H, W=W, recs=recs), F.conv2d(cur, w, b, stride=1, padding=1)


# ------------------------------------------------------------------------------------------------ the backward
def _pre_act(rec, y):
    return y if rec["scale"] is None else y * _col(rec["scale"]) + _col(rec["shift"])


def _forced(v, force, key):
    """the pre-activation with the undecided elements of stage `key` taken as positive / negative"""
    if force is None or key not in force[0]:
        return v
    return torch.where(force[0][key], torch.full_like(v, 1.0 if force[1] else -1.0), v)


def _bn_bwd(rec, y, gh, grads, c12_always=False, drop_c2=False):
    """dy from the activation gradient gh; records dgamma / dbeta under rec['bnkey'] (bnname for the discriminator)"""
    if rec["scale"] is None:
        return gh
    xh = (y - _col(rec["mean"])) * _col(rec["invstd"])
    s1, s2 = gh.sum((0, 2, 3)), (gh * xh).sum((0, 2, 3))
    bn = rec.get("bnkey") or rec.get("bnname")
    grads[bn + ".weight"], grads[bn + ".bias"] = s2, s1
    M = y.shape[0] * y.shape[2] * y.shape[3]
    c1, c2 = (s1 / M, s2 / M) if (rec["train_stats"] or c12_always) else (torch.zeros_like(s1), torch.zeros_like(s2))
    if drop_c2:
        c2 = torch.zeros_like(c2)
    return _col(rec["scale"]) * (gh - _col(c1) - xh * _col(c2))


def replay_generator(state, dout, need_dx, store=None, S=None, mutant=None, force=None):
    """generator_backward in fp64 -> ({state-dict name: gradient}, darch [rows of arch, 3], dx or None).
    mutant: one of MUTANTS_G, a backward wrong in one stated way (at down level MUT_LEVEL / up block MUT_BLOCK where it lives at one
    place).  force: (masks from undecided(), bool): the sign of those pre-activations taken as + / -, for both consumers."""
    assert mutant is None or mutant in MUTANTS_G
    N, H, W, D = state["N"], state["H"], state["W"], state["D"]
    S = loss_scale(N, H, W) if S is None else S
    levels, ups = state["levels"], state["ups"]
    grads = {}
    darch = torch.zeros(state["arch_shape"], dtype=torch.float64)
    rnd = (lambda t: t) if store is None else (lambda t: (t * S).to(store).double() / S)

    def upconv_bwd(d, du):
        rec = ups[d]
        rin, sm = rec["rin"], rec["sm"]
        w4, w6, w8 = rec["w"]
        # the transposed conv seen from its output side is a stride-2 / pad-3 conv du -> rin with the same [cin, cout, 8, 8] kernel
        dwm = G.conv2d_weight(du, w8.shape, rin, stride=2, padding=3)
        o6 = 0 if (mutant == "w6_offset" and d == MUT_BLOCK) else 1
        grads[rec["wkeys"][0]] = sm[0] * dwm[:, :, 2:6, 2:6]
        grads[rec["wkeys"][1]] = sm[1] * dwm[:, :, o6:o6 + 6, o6:o6 + 6]
        grads[rec["wkeys"][2]] = sm[2] * dwm
        dots = torch.stack([(dwm[:, :, 2:6, 2:6] * w4).sum(), (dwm[:, :, 1:7, 1:7] * w6).sum(), (dwm * w8).sum()])
        if rec["b"] is not None:
            dbm = du.sum((0, 2, 3))
            for j in range(3):
                grads[rec["bkeys"][j]] = sm[j] * dbm
            if mutant != "arch_no_bias_dot":
                dots = dots + torch.stack([(dbm * rec["b"][j]).sum() for j in range(3)])
        # (in front of a batch-statistics BatchNorm the loss does not change with the scale of Wm, so sum sm * dots = <dWm, Wm> is
        # zero up to rounding there: this mutant lives at every block, and the image layer is where it shows)
        mean = 0.0 if mutant == "softmax_no_mean" else (sm * dots).sum()
        darch[rec["li"]] = sm * (dots - mean)
        wm = merged_kernel(rec)
        if store is not None:
            wm = wm.to(store).double()
        if mutant == "flipped_dgrad" and d == MUT_BLOCK:
            wm = wm.flip(2, 3)
        return rnd(F.conv2d(du, wm, None, stride=2, padding=3))

    # ---- outermost: out = tanh(u0)
    dtl = rnd(dout.double())
    du = rnd(dtl * (1.0 - torch.tanh(ups[0]["u"]) ** 2))
    dR = {1: upconv_bwd(0, du)}

    # ---- inwards through the up path: the second half of dR[d] belongs to block d
    for d in range(1, D):
        rec = ups[d]
        cd = dR[d].shape[1] // 2
        g = dR[d][:, :cd] if (mutant == "swap_halves" and d == MUT_LEVEL) else dR[d][:, cd:]
        gh = act_bwd64(g, _forced(_pre_act(rec, rec["u"]), force, ("up", d)), "relu")
        if rec["keep"] is not None:
            if mutant != "ignore_keep":
                gh = gh * rec["keep"]
            if mutant != "drop_keep_scale":
                gh = gh * rec["kscale"]
        du = rnd(_bn_bwd(rec, rec["u"], gh, grads, c12_always=(mutant == "eval_keeps_c12" and d == MUT_BLOCK)))
        dR[d + 1] = upconv_bwd(d, du)

    # ---- the down path, innermost first
    dL = dx = None
    for k in range(D, 0, -1):
        lv = levels[k]
        y = lv["y"]
        v = _forced(_pre_act(lv, y), force, ("down", k))
        if k == D:
            gh = act_bwd64(dR[k], v, "relu")                               # the innermost level: the ReLU consumer alone
            if mutant == "innermost_two_consumers":
                gh = gh + act_bwd64(dR[k], v, "leaky")
        else:
            ck = dR[k].shape[1] // 2
            g = dR[k][:, ck:] if (mutant == "swap_halves" and k == MUT_LEVEL) else dR[k][:, :ck]
            gh = act_bwd64(g, v, "relu")
            if not (mutant == "drop_leaky_consumer" and k == MUT_LEVEL):
                gh = gh + act_bwd64(dL, v, "relu" if (mutant == "leaky_as_relu" and k == MUT_LEVEL) else "leaky")
        dy = rnd(_bn_bwd(lv, y, gh, grads, c12_always=(mutant == "eval_keeps_c12" and k == MUT_LEVEL),
                         drop_c2=(mutant == "drop_c2" and k == MUT_LEVEL)))
        grads[lv["wkey"]] = G.conv2d_weight(lv["inp"], lv["w"].shape, dy, stride=2, padding=1)
        if k > 1:
            dL = rnd(G.conv2d_input(lv["inp"].shape, lv["wd"], dy, stride=2, padding=1))
        elif need_dx:
            dx = G.conv2d_input(lv["inp"].shape, lv["w"], dy, stride=2, padding=1)        # fp32 weights, fp32 image gradient
    return grads, darch, dx


def replay_discriminator(state, dlogits, need_dx, store=None, S=None, mutant=None, force=None):
    """DiscriminatorEngine.backward in fp64 -> ({state-dict name: gradient}, dx or None)"""
    assert mutant is None or mutant in MUTANTS_D
    dl = dlogits.double()
    S = float(2 ** round(math.log2(max(dl.numel(), 1)))) if S is None else S
    rnd = (lambda t: t) if store is None else (lambda t: (t * S).to(store).double() / S)
    recs = state["recs"]
    grads = {}
    last = recs[-1]
    grads[last["name"] + ".weight"] = G.conv2d_weight(last["inp"], last["w"].shape, dl, stride=last["s"], padding=last["p"])
    if last["b"] is not None:
        grads[last["name"] + ".bias"] = dl.sum((0, 2, 3))
    dz = rnd(G.conv2d_input(last["inp"].shape, last["w"], dl, stride=last["s"], padding=last["p"]))      # fp32 weights
    for i in range(len(recs) - 2, 0, -1):
        rec = recs[i]
        gh = act_bwd64(dz, _forced(_pre_act(rec, rec["y"]), force, ("mid", i)), "leaky")
        dy = rnd(_bn_bwd(rec, rec["y"], gh, grads))
        grads[rec["name"] + ".weight"] = G.conv2d_weight(rec["inp"], rec["w"].shape, dy, stride=rec["s"], padding=rec["p"])
        dz = rnd(G.conv2d_input(rec["inp"].shape, rec["wd"], dy, stride=rec["s"], padding=rec["p"]))
    first = recs[0]
    dy = rnd(act_bwd64(dz, first["z"], "leaky"))
    grads[first["name"] + ".weight"] = G.conv2d_weight(first["x"], first["w"].shape, dy, stride=first["s"], padding=first["p"])
    if first["b"] is not None:
        grads[first["name"] + ".bias"] = (dy[:, :, :-1, :-1] if mutant == "d_first_bias_border" else dy).sum((0, 2, 3))
    dx = None
    if need_dx:
        dx = G.conv2d_input(first["x"].shape, first["w"], dy, stride=first["s"], padding=first["p"])
        if mutant == "d_dx_class_swapped":
            dx = dx.clone()
            a, b = dx[:, :, 0::2, 1::2].clone(), dx[:, :, 1::2, 0::2].clone()
            dx[:, :, 0::2, 1::2], dx[:, :, 1::2, 0::2] = b, a
    return grads, dx


# ------------------------------------------------------------------------------------------------ undecided signs, replays
def undecided(state):
    """{stage key: mask} of the elements whose sign of scale * y + shift fp32 cannot decide (SIGN_MARGIN), and their count.  ReLU
    and LeakyReLU of one level share that sign: one mask forces both consumers.  Stages without a norm read the stored sign."""
    if state["kind"] == "pix2pix_g":
        items = [(("down", k), lv, lv["y"]) for k, lv in state["levels"].items()]
        items += [(("up", d), u, u["u"]) for d, u in state["ups"].items()]
    else:
        items = [(("mid", i), r, r["y"]) for i, r in enumerate(state["recs"]) if r["kind"] == "mid"]
    masks, n = {}, 0
    for key, rec, y in items:
        if rec["scale"] is None:
            continue
        sy, sh = y * _col(rec["scale"]), _col(rec["shift"])
        m = (sy + sh).abs() < SIGN_MARGIN * (sy.abs() + sh.abs())
        if bool(m.any()):
            masks[key] = m
            n += int(m.sum())
    return masks, n


def flat(res):
    """(grads, darch, dx) / (grads, dx) as one dict, the keys 'darch' and 'dx' beside the state-dict names"""
    out = dict(res[0])
    if len(res) == 3:
        out["darch"] = res[1]
    if res[-1] is not None:
        out["dx"] = res[-1]
    return out


def _d_u(r64, on, off):
    return {k: float((on[k] - off[k]).norm()) / max(float(r64[k].norm()), 1e-300) for k in r64}


def replays(state, dout, need_dx, store, S=None):
    """(R64, R16, d_U per tensor, count of undecided elements) of either engine's state: what compare() needs"""
    fn = replay_generator if state["kind"] == "pix2pix_g" else replay_discriminator
    r64 = flat(fn(state, dout, need_dx, None, S))
    r16 = flat(fn(state, dout, need_dx, store, S))
    masks, n_und = undecided(state)
    d_u = {k: 0.0 for k in r64}
    if n_und:
        d_u = _d_u(r64, flat(fn(state, dout, need_dx, None, S, force=(masks, True))),
                   flat(fn(state, dout, need_dx, None, S, force=(masks, False))))
    return r64, r16, d_u, n_und


def replays_chain(state_d, state_g, dlogits, store, image_channels):
    """the generator step's chain: the discriminator's replay with need_dx, then the generator's on the last image_channels
    channels of that dx (the fake image behind the mask in cat(mask, fake)).  As replays(), for the generator's gradients."""
    def chain(st, force_d=None, force_g=None):
        _, dxd = replay_discriminator(state_d, dlogits, True, st, force=force_d)
        return flat(replay_generator(state_g, dxd[:, -image_channels:], False, st, force=force_g))
    r64, r16 = chain(None), chain(store)
    (md, nd), (mg, ng) = undecided(state_d), undecided(state_g)
    d_u = {k: 0.0 for k in r64}
    if nd + ng:
        d_u = _d_u(r64, chain(None, (md, True), (mg, True)), chain(None, (md, False), (mg, False)))
    return r64, r16, d_u, nd + ng
