"""fp64 statement of the ResNet generator (reference models_pix2pix/networks.py:321-439) and of the backward plan of
models_pix2pix/resnet_engine.py, replayed from the state the engine's own forward saved.

  forward_state        the forward on the CPU from a state dict and an image as a PLAIN state (NCHW fp64 tensors: no NHWC, no padded
                       buffers, no uint8 masks) and the image.  store=None: nothing is rounded, so replay() of it must be
                       torch.autograd through the reference module.  store=dt: every tensor the engine keeps in 16 bits (conv
                       outputs, activations, MFMA weights) rounded where it is stored, coefficients to fp32.
  state_from_ctx       the same plain state read from the engine's ctx: padded NHWC buffers become their interior views in NCHW
  replay               the hand-derived backward: every parameter gradient by state-dict name and dx
  undecided / replays  elements whose ReLU sign fp32 cannot decide, and what backward_replay.compare() needs: R64, R16, d_U
  FWD_MUTANTS / BWD_MUTANTS   the stated wrong implementations, each of which the bounds of the GPU tests must catch

The plan.  x -> pad3 -> conv7 (fp32 weights) -> n+ReLU -> conv3/s2 -> n+ReLU -> conv3/s2 -> n+ReLU = a_0; block b: q = [ReLU(n(conv3(
pad1(a_b)))) * keep * kscale]; a_{b+1} = a_b + n(conv3(pad1(q))); convT3/s2 -> n+ReLU, twice; pad3 -> conv7 + bias -> tanh.
ReflectionPad2d excludes the edge (index -1 is pixel 1).  n is BatchNorm2d (batch statistics in train mode, taken from the unrounded
conv output as the conv epilogues do; running statistics in eval) or InstanceNorm2d (biased plane statistics of the STORED output in
both modes).  A conv bias in front of an InstanceNorm cancels: never added, gradient zero; replay() reports sum(dy), which is zero up
to rounding, with its scale sum|dy| so that a test can hold the engine's exact zeros to it.
Backward: d = S * dout * (1 - t^2); the data gradient of a conv behind a pad is taken on the padded grid and folded: every border
element is added to the pixel it mirrors (fold64: rows, then columns -- the adjoint of the pad); d a_b = fold(d pad1(a_b)) + d a_{b+1}.
BatchNorm: dy = scale * (g - c1 - xh * c2), c1 = mean(g), c2 = mean(g * xh), both zero under running statistics.  InstanceNorm:
dy = invstd * (g - mean_plane(g) - xh * mean_plane(g * xh)).  ReLU'(0) = 0.
store=dt rounds, as S * value, what the engine keeps in 16 bits between launches: every dy, every data gradient (on the padded grid,
before the fold) and every fold's result.  Never rounded: d, the fp32 weight / bias gradients and dx."""
import math

import torch
import torch.nn.functional as F
from torch.nn import grad as G

from tests.backward_replay import BN_EPS, DT, FLOOR32, SIGN_MARGIN, compare, d64, loss_scale, nchw  # noqa: F401

FWD_MUTANTS = ("replicate_pad", "symmetric_pad", "zero_pad", "border_in_stats", "residual_before_norm", "ignore_keep", "keep_no_scale",
               "output_padding_leading", "unflipped_convT", "classes_exchanged", "unbiased_var")
BWD_MUTANTS = ("fold_drops_diagonal", "no_fold_at_head", "drop_stream_grad", "drop_branch_grad", "ignore_keep_bwd", "keep_no_scale_bwd",
               "no_tanh_derivative", "eval_keeps_c12")


def _col(t):
    return t.view(1, -1, 1, 1)


def _pl(t):
    return t.view(t.shape[0], t.shape[1], 1, 1)


def _rounders(store):
    if store is None:
        return (lambda t: t), (lambda t: t)
    return (lambda t: t.to(store).double()), (lambda t: t.float().double())


def pad64(t, p, mode="reflect"):
    if p == 0:
        return t
    if mode == "zero_pad":
        return F.pad(t, [p] * 4)
    if mode == "replicate_pad":
        return F.pad(t, [p] * 4, mode="replicate")
    if mode == "symmetric_pad":                                       # edge included: index -1 is pixel 0
        H, W = t.shape[2:]
        iy = torch.tensor([(-1 - i if i < 0 else (2 * H - 1 - i if i >= H else i)) for i in range(-p, H + p)])
        ix = torch.tensor([(-1 - i if i < 0 else (2 * W - 1 - i if i >= W else i)) for i in range(-p, W + p)])
        return t[:, :, iy][:, :, :, ix]
    return F.pad(t, [p] * 4, mode="reflect")


def fold64(d, p, drop_diagonal=False):
    """adjoint of ReflectionPad2d(p): d [N,C,H+2p,W+2p] -> [N,C,H,W].  Rows first (over the full padded width), then columns; border
    row -i (i = 1..p) lands on row i, border row H-1+i on row H-1-i.  drop_diagonal (a mutant): the corner blocks are lost."""
    if p == 0:
        return d
    if drop_diagonal:
        d = d.clone()
        for ys in (slice(0, p), slice(-p, None)):
            for xs in (slice(0, p), slice(-p, None)):
                d[:, :, ys, xs] = 0
    H = d.shape[2] - 2 * p
    r = d[:, :, p:p + H].clone()
    r[:, :, 1:p + 1] += d[:, :, :p].flip(2)
    r[:, :, H - 1 - p:H - 1] += d[:, :, p + H:].flip(2)
    W = r.shape[3] - 2 * p
    o = r[:, :, :, p:p + W].clone()
    o[:, :, :, 1:p + 1] += r[:, :, :, :p].flip(3)
    o[:, :, :, W - 1 - p:W - 1] += r[:, :, :, p + W:].flip(3)
    return o


# ------------------------------------------------------------------------------------------------ layout of the key names
def layout(n_blocks, use_dropout):
    """state-dict prefixes (conv, norm) of the normed convs in forward order, and the head's"""
    j = 6 if use_dropout else 5
    names = dict(stem=("model.1", "model.2"), downs=[("model.4", "model.5"), ("model.7", "model.8")], blocks=[], ups=[])
    for b in range(n_blocks):
        p = "model.%d.conv_block" % (10 + b)
        names["blocks"].append(((p + ".1", p + ".2"), (p + ".%d" % j, p + ".%d" % (j + 1))))
    i = 10 + n_blocks
    names["ups"] = [("model.%d" % i, "model.%d" % (i + 1)), ("model.%d" % (i + 3), "model.%d" % (i + 4))]
    names["head"] = "model.%d" % (i + 7)
    return names


# ------------------------------------------------------------------------------------------------ the forward
def _coefs(sd, nname, norm, yfull, y, train, r32, mutant, pad_for_stats=0):
    """coefficients of the norm behind a conv: BatchNorm from the unrounded output (train) or the running statistics, InstanceNorm
    from the stored output"""
    unb = mutant == "unbiased_var"
    if norm == "instance":
        src = pad64(y, pad_for_stats) if mutant == "border_in_stats" else y
        mean, var = src.mean((2, 3)), src.var((2, 3), unbiased=unb)
        return dict(norm="in", mean=r32(mean), invstd=r32(torch.rsqrt(var + BN_EPS)), train_stats=True)
    if train:
        src = pad64(yfull, pad_for_stats) if mutant == "border_in_stats" else yfull
        mean, var = src.mean((0, 2, 3)), src.var((0, 2, 3), unbiased=unb)
    else:
        mean, var = sd[nname + ".running_mean"], sd[nname + ".running_var"]
    invstd = torch.rsqrt(var + BN_EPS)
    scale = sd[nname + ".weight"] * invstd
    return dict(norm="bn", scale=r32(scale), shift=r32(sd[nname + ".bias"] - mean * scale), mean=r32(mean), invstd=r32(invstd),
                train_stats=bool(train))


def pre_act(rec, y=None):
    y = rec["y"] if y is None else y
    if rec["norm"] == "in":
        return (y - _pl(rec["mean"])) * _pl(rec["invstd"])
    return y * _col(rec["scale"]) + _col(rec["shift"])


def convT64(x, w, mutant=None):
    """ConvTranspose2d(3, stride 2, padding 1, output_padding 1) and its stated wrong forms"""
    if mutant == "unflipped_convT":
        w = w.flip(2, 3)
    if mutant == "output_padding_leading":
        return F.pad(F.conv_transpose2d(x, w, None, stride=2, padding=1), [1, 0, 1, 0])
    y = F.conv_transpose2d(x, w, None, stride=2, padding=1, output_padding=1)
    if mutant == "classes_exchanged":
        y = torch.stack((y[:, :, 1::2], y[:, :, 0::2]), 3).reshape(y.shape)
    return y


def forward_state(sd, cfg, x, train, masks=None, store=None, mutant=None):
    """cfg: dict(n_blocks, norm 'batch' | 'instance', use_dropout).  masks: NCHW keep masks {0,1} [N,4ngf,H/4,W/4], one per block,
    first block first; applied in train mode with kscale = 2 (nn.Dropout(0.5)).  Returns (state, image)."""
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x = x.double()
    r16, r32 = _rounders(store)
    nm = layout(cfg["n_blocks"], cfg["use_dropout"])
    norm = cfg["norm"]
    N, _, H, W = x.shape
    mode = mutant if mutant in ("replicate_pad", "symmetric_pad", "zero_pad") else "reflect"

    def stage(names, inp, kind, act, p_in, res=None, keep=None, next_pad=0):
        cname, nname = names
        w = sd[cname + ".weight"]
        wd = w if kind == "stem" else r16(w)                          # the direct 7x7 conv reads the fp32 weights
        if kind == "up":
            yfull = convT64(inp, wd, mutant)
        else:
            yfull = F.conv2d(pad64(inp, p_in, mode), wd, None, stride=2 if kind == "down" else 1, padding=1 if kind == "down" else 0)
        rec = dict(kind=kind, name=cname, nname=None if norm == "instance" else nname, w=w, wd=wd, inp=inp, y=r16(yfull), act=act,
                   p_in=p_in, keep=None, kscale=1.0, has_bias=cname + ".bias" in sd)
        rec.update(_coefs(sd, nname, norm, yfull, rec["y"], train, r32, mutant, next_pad))
        if mutant == "residual_before_norm" and res is not None:
            v = pre_act(rec, rec["y"] + res)
            res = None
        else:
            v = pre_act(rec)
        if act == "relu":
            v = v.clamp_min(0)
        if keep is not None:
            rec["keep"], rec["kscale"] = keep, 2.0
            if mutant != "ignore_keep":
                v = v * keep * (1.0 if mutant == "keep_no_scale" else 2.0)
        if res is not None:
            v = v + res
        return rec, r16(v)

    state = dict(kind="pix2pix_resnet", N=N, H=H, W=W, x=x, norm=norm, downs=[], blocks=[], ups=[])
    state["stem"], a = stage(nm["stem"], x, "stem", "relu", 3)
    for i, names in enumerate(nm["downs"]):
        rec, a = stage(names, a, "down", "relu", 0, next_pad=1 if i == 1 else 0)
        state["downs"].append(rec)
    for b, (n1, n2) in enumerate(nm["blocks"]):
        keep = masks[b].double() if (masks is not None and train and cfg["use_dropout"]) else None
        r1, q = stage(n1, a, "block", "relu", 1, keep=keep, next_pad=1)
        r2, a = stage(n2, q, "block", "none", 1, res=a, next_pad=0 if b == cfg["n_blocks"] - 1 else 1)
        state["blocks"].append((r1, r2))
    for i, names in enumerate(nm["ups"]):
        rec, a = stage(names, a, "up", "relu", 0, next_pad=3 if i == 1 else 0)
        state["ups"].append(rec)
    hw, hb = sd[nm["head"] + ".weight"], sd[nm["head"] + ".bias"]
    image = torch.tanh(F.conv2d(pad64(a, 3, mode), hw, hb))
    state["head"] = dict(name=nm["head"], w=hw, b=hb, inp=a, t=r32(image))
    return state, image


# ------------------------------------------------------------------------------------------------ adapter
def state_from_ctx(engine, ctx):
    """The saved forward of ResnetGeneratorEngine.forward as the plain state above: a tensor padded by p becomes its interior."""
    dt = engine.tdt

    def inner(t, p):
        return nchw(t[:, p:t.shape[1] - p, p:t.shape[2] - p] if p else t)

    def coefs(nc):
        if nc["inorm"] is not None:
            return dict(norm="in", mean=d64(nc["inorm"][0]), invstd=d64(nc["inorm"][1]), train_stats=True)
        c = nc["coef"]
        return dict(norm="bn", scale=d64(c[0]), shift=d64(c[1]), mean=d64(c[2]), invstd=d64(c[3]), train_stats=bool(nc["stats"]))

    def rec_of(kind, name, nname, conv, inp, y, nc, act, p_in, keep=None, kscale=1.0):
        w = d64(conv.weight)
        rec = dict(kind=kind, name=name, nname=nname if nc["inorm"] is None else None, w=w,
                   wd=w if kind == "stem" else w.to(dt).double(), inp=inp, y=nchw(y), act=act, p_in=p_in,
                   keep=None if keep is None else nchw(keep), kscale=kscale, has_bias=conv.bias is not None)
        rec.update(coefs(nc))
        return rec

    def nxt(name):
        head, _, idx = name.rpartition(".")
        return "%s.%d" % (head, int(idx) + 1)

    st = ctx["stem"]
    state = dict(kind="pix2pix_resnet", N=ctx["N"], H=ctx["H"], W=ctx["W"], x=d64(ctx["x"]),
                 norm="instance" if st["nc"]["inorm"] is not None else "batch", downs=[], blocks=[], ups=[])
    state["stem"] = rec_of("stem", st["name"], nxt(st["name"]), st["conv"], d64(ctx["x"]), st["y"], st["nc"], "relu", 3)
    for r in ctx["downs"]:
        state["downs"].append(rec_of("down", r["name"], nxt(r["name"]), r["conv"], nchw(r["inp"]), r["y"], r["nc"], "relu", 0))
    for r in ctx["blocks"]:
        n1, n2 = r["name"] + ".1", "%s.%d" % (r["name"], r["j2"])
        r1 = rec_of("block", n1, nxt(n1), r["conv1"], inner(r["P"], 1), r["y1"], r["n1"], "relu", 1, r["keep"], r["kscale"])
        r2 = rec_of("block", n2, nxt(n2), r["conv2"], inner(r["Q"], 1), r["y2"], r["n2"], "none", 1)
        state["blocks"].append((r1, r2))
    for r in ctx["ups"]:
        state["ups"].append(rec_of("up", r["name"], nxt(r["name"]), r["conv"], nchw(r["inp"]), r["y"], r["nc"], "relu", 0))
    hd = ctx["head"]
    state["head"] = dict(name=hd["name"], w=d64(hd["conv"].weight), b=d64(hd["conv"].bias), inp=inner(hd["inp"], 3), t=d64(ctx["t"]))
    return state


# ------------------------------------------------------------------------------------------------ the backward
def _stages(state):
    out = [("stem", state["stem"])] + [(("down", i), r) for i, r in enumerate(state["downs"])]
    for b, (r1, r2) in enumerate(state["blocks"]):
        out += [(("b1", b), r1), (("b2", b), r2)]
    return out + [(("up", i), r) for i, r in enumerate(state["ups"])]


def replay(state, dout, need_dx, store=None, S=None, mutant=None, force=None):
    """(grads by state-dict name, dx or None, bias_scale): bias_scale[name] = sum|dy| / S for the cancelled biases"""
    S = loss_scale(state["N"], state["H"], state["W"]) if S is None else S
    rnd = (lambda t: t) if store is None else (lambda t: t.to(store).double())
    grads, bias_scale = {}, {}

    def norm_bwd(key, rec, dz):
        v = pre_act(rec)
        if force is not None and key in force[0]:
            v = torch.where(force[0][key], torch.full_like(v, 1.0 if force[1] else -1.0), v)
        g = dz * (v > 0).double() if rec["act"] == "relu" else dz
        if rec["keep"] is not None and mutant != "ignore_keep_bwd":
            g = g * rec["keep"] * (1.0 if mutant == "keep_no_scale_bwd" else rec["kscale"])
        if rec["norm"] == "in":
            xh = (rec["y"] - _pl(rec["mean"])) * _pl(rec["invstd"])
            dy = _pl(rec["invstd"]) * (g - g.mean((2, 3), keepdim=True) - xh * (g * xh).mean((2, 3), keepdim=True))
        else:
            xh = (rec["y"] - _col(rec["mean"])) * _col(rec["invstd"])
            s1, s2 = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
            grads[rec["nname"] + ".weight"], grads[rec["nname"] + ".bias"] = s2 / S, s1 / S
            M = g.shape[0] * g.shape[2] * g.shape[3]
            on = rec["train_stats"] or mutant == "eval_keeps_c12"
            c1, c2 = (s1 / M, s2 / M) if on else (torch.zeros_like(s1), torch.zeros_like(s2))
            dy = _col(rec["scale"]) * (g - _col(c1) - xh * _col(c2))
        dy = rnd(dy)
        if rec["has_bias"]:                                          # in front of an InstanceNorm: cancelled
            grads[rec["name"] + ".bias"] = dy.sum((0, 2, 3)) / S
            bias_scale[rec["name"] + ".bias"] = float(dy.abs().sum()) / S
        return dy

    def conv_bwd(rec, dy, need_dinp=True):
        """weight gradient, and the gradient w.r.t. the conv's (unpadded) input: taken on the padded grid, rounded, folded"""
        p = rec["p_in"]
        if rec["kind"] == "up":
            grads[rec["name"] + ".weight"] = G.conv2d_weight(dy, rec["w"].shape, rec["inp"], stride=2, padding=1) / S
            return rnd(F.conv2d(dy, rec["wd"], None, stride=2, padding=1))
        s, zp = (2, 1) if rec["kind"] == "down" else (1, 0)
        xin = pad64(rec["inp"], p)
        grads[rec["name"] + ".weight"] = G.conv2d_weight(xin, rec["w"].shape, dy, stride=s, padding=zp) / S
        if not need_dinp:
            return None
        dpad = G.conv2d_input(xin.shape, rec["wd"], dy, stride=s, padding=zp)
        if rec["kind"] == "stem":                                    # fp32 all the way: dx is never rounded
            return fold64(dpad, p) / S
        dpad = rnd(dpad)
        return dpad if p == 0 else fold64(dpad, p, mutant == "fold_drops_diagonal")

    hd = state["head"]
    t = hd["t"]
    d = S * dout.double() * (1.0 if mutant == "no_tanh_derivative" else (1 - t * t))
    tin = pad64(hd["inp"], 3)
    grads[hd["name"] + ".weight"] = G.conv2d_weight(tin, hd["w"].shape, d) / S
    grads[hd["name"] + ".bias"] = d.sum((0, 2, 3)) / S
    dT = rnd(G.conv2d_input(tin.shape, hd["w"], d))
    dz = rnd(dT[:, :, 3:-3, 3:-3].contiguous() if mutant == "no_fold_at_head" else fold64(dT, 3))
    for i in (1, 0):
        rec = state["ups"][i]
        dz = conv_bwd(rec, norm_bwd(("up", i), rec, dz))
    for b in range(len(state["blocks"]) - 1, -1, -1):
        r1, r2 = state["blocks"][b]
        dq = rnd(conv_bwd(r2, norm_bwd(("b2", b), r2, dz)))
        dbranch = conv_bwd(r1, norm_bwd(("b1", b), r1, dq))
        if mutant == "drop_stream_grad":
            dz = rnd(dbranch)
        elif mutant == "drop_branch_grad":
            pass
        else:
            dz = rnd(dbranch + dz)
    for i in (1, 0):
        rec = state["downs"][i]
        dz = conv_bwd(rec, norm_bwd(("down", i), rec, dz))
    dx = conv_bwd(state["stem"], norm_bwd("stem", state["stem"], dz), need_dx)
    return grads, (dx if need_dx else None), bias_scale


# ------------------------------------------------------------------------------------------------ undecided signs, replays
def undecided(state):
    """{stage key: mask} of the ReLU stages' elements whose sign fp32 cannot decide (SIGN_MARGIN), and their count"""
    masks, n = {}, 0
    for key, rec in _stages(state):
        if rec["act"] != "relu":
            continue
        if rec["norm"] == "in":
            mu = _pl(rec["mean"])
            m = (rec["y"] - mu).abs() < SIGN_MARGIN * (rec["y"].abs() + mu.abs())
        else:
            sy, sh = rec["y"] * _col(rec["scale"]), _col(rec["shift"])
            m = (sy + sh).abs() < SIGN_MARGIN * (sy.abs() + sh.abs())
        if bool(m.any()):
            masks[key] = m
            n += int(m.sum())
    return masks, n


def flat(res):
    """(grads, dx, bias_scale) -> (one dict with 'dx' beside the state-dict names, WITHOUT the cancelled biases; bias_scale)"""
    grads, dx, bias_scale = res
    out = {k: v for k, v in grads.items() if k not in bias_scale}
    if dx is not None:
        out["dx"] = dx
    return out, bias_scale


def replays(state, dout, need_dx, store, S=None):
    """(R64, R16, d_U per tensor, count of undecided elements, bias_scale, cancelled-bias sums of R64)"""
    res64 = replay(state, dout, need_dx, None, S)
    r64, bias_scale = flat(res64)
    r16, _ = flat(replay(state, dout, need_dx, store, S))
    masks, n_und = undecided(state)
    d_u = {k: 0.0 for k in r64}
    if n_und:
        on, _ = flat(replay(state, dout, need_dx, None, S, force=(masks, True)))
        off, _ = flat(replay(state, dout, need_dx, None, S, force=(masks, False)))
        d_u = {k: float((on[k] - off[k]).norm()) / max(float(r64[k].norm()), 1e-300) for k in r64}
    return r64, r16, d_u, n_und, bias_scale


def hold(got, rp, dt):
    """compare() of a result with replays(), and the cancelled biases: |got| <= 2 u16 sum|dy| (the engine writes exact zeros).
    Returns (report, failures)."""
    r64, r16, d_u, _, bias_scale = rp
    rep, bad = compare({k: got[k] for k in r64}, r64, r16, d_u)
    u16 = 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8
    for k, sc in bias_scale.items():
        worst = float(d64(got[k]).abs().max())
        ok = worst <= 2 * u16 * sc
        rep[k] = dict(err=worst, e16=0.0, ratio=0.0, d_u=0.0, bound=2 * u16 * sc, row_worst=0.0, ok=ok, absolute=True)
        if not ok:
            bad.append(k)
    return rep, bad


def rel_err(a, ref):
    return float((a.double() - ref).norm()) / float(ref.norm())


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
# Shared with the CPU tests, which prove on these very seeds that the bounds tell every mutant from a right implementation.
# fixture: weights and image of tests/golden/pix2pix_resnet_{a,b}.npz (golden_util_resnet.FIXTURES); otherwise seeded here.
CASES = {
    "r9_in_32_a": dict(cin=1, cout=1, ngf=64, n_blocks=9, norm="instance", use_dropout=True, N=2, H=32, W=32, dtype="f16", seed=71,
                       fixture="pix2pix_resnet_a"),
    "r6_bn_20x28_b": dict(cin=3, cout=3, ngf=16, n_blocks=6, norm="batch", use_dropout=False, N=3, H=20, W=28, dtype="f16", seed=72,
                          fixture="pix2pix_resnet_b"),
    "r2_bn_drop_16x24": dict(cin=1, cout=2, ngf=16, n_blocks=2, norm="batch", use_dropout=True, N=2, H=16, W=24, dtype="f16", seed=73,
                             fixture=None),
    "r2_in_8": dict(cin=1, cout=1, ngf=16, n_blocks=2, norm="instance", use_dropout=False, N=2, H=8, W=8, dtype="f16", seed=75,
                    fixture=None),
    "r6_bn_8": dict(cin=1, cout=1, ngf=16, n_blocks=6, norm="batch", use_dropout=False, N=2, H=8, W=8, dtype="f16", seed=76,
                    fixture=None),
    "r3_in_12x8_bf16": dict(cin=2, cout=1, ngf=16, n_blocks=3, norm="instance", use_dropout=False, N=3, H=12, W=8, dtype="bf16", seed=74,
                            fixture=None),
    # the 7x7 ends past one LDS load of weights: the canonical RGB generator's 3 -> 64 -> 3, and an ngf that is no 8 * 2^j
    "r2_bn_rgb64_16x12": dict(cin=3, cout=3, ngf=64, n_blocks=2, norm="batch", use_dropout=False, N=2, H=16, W=12, dtype="f16", seed=77,
                              fixture=None),
    "r2_in_4to2_ngf72_12x16": dict(cin=4, cout=2, ngf=72, n_blocks=2, norm="instance", use_dropout=False, N=2, H=12, W=16, dtype="f16",
                                   seed=78, fixture=None),
}


def case_inputs(c):
    """(state dict, x, dout [fp64, of the size of a mean-loss gradient], keep masks NCHW) of a case.
    dout is uniform in (-0.5, 1.5) / numel, NOT centred: the head's bias gradient is the plain sum of d = dout * (1 - t^2) over all
    pixels of one channel, and compare()'s floor under a tensor without a 16-bit store (FLOOR32, the relative error of an fp32 sum)
    is a statement about sums that do not cancel.  A centred dout makes that sum the end point of a random walk, of unbounded
    condition number sum|d| / |sum d| -- 516 in the fp64 statement of r6_bn_8 in eval mode, where fp32 roundings of the terms alone
    (three each) reach 3 * 516 * 2^-24 = 9e-5 of the sum in the worst case.  With the offset the condition number stays below 4
    (head_bias_condition, asserted by the CPU tests on every case), and 3 * 4 * 2^-24 is below FLOOR32."""
    from golden_util_resnet import FIXTURES, INPUT_STD, fixture_inputs, seeded_resnet_state_dict
    g = torch.Generator().manual_seed(c["seed"])
    if c["fixture"]:
        f = FIXTURES[c["fixture"]]
        sd = seeded_resnet_state_dict(f["seed_g"], c["cin"], c["cout"], c["ngf"], c["n_blocks"], c["norm"], c["use_dropout"])
        x = fixture_inputs(f)[0]
    else:
        sd = seeded_resnet_state_dict(c["seed"], c["cin"], c["cout"], c["ngf"], c["n_blocks"], c["norm"], c["use_dropout"])
        x = INPUT_STD * torch.randn((c["N"], c["cin"], c["H"], c["W"]), generator=g)
    dout = (torch.rand((c["N"], c["cout"], c["H"], c["W"]), generator=g, dtype=torch.float64) * 2 - 0.5) / (c["N"] * c["cout"] * c["H"] * c["W"])
    masks = [(torch.rand((c["N"], 4 * c["ngf"], c["H"] // 4, c["W"] // 4), generator=g) >= 0.5).to(torch.uint8)
             for _ in range(c["n_blocks"])]
    return sd, x, dout, masks


def head_bias_condition(image, dout):
    """sum|d| / |sum d| per output channel of d = dout * (1 - t^2): the condition number of the head's bias gradient"""
    d = dout.double() * (1 - image.double() ** 2)
    return d.abs().sum((0, 2, 3)) / d.sum((0, 2, 3)).abs()


def cfg_of(c):
    return dict(n_blocks=c["n_blocks"], norm=c["norm"], use_dropout=c["use_dropout"])
