"""fp64 replay of the U-Net engines' backward plans from the state their forward saved.

`UNetEngine.backward(ctx, params, dlogits, need_dx)` is a pure function of `ctx` and `dlogits`, and linear in `dlogits`; so is
`UNet3DEngine.backward(ctx, dlogits)` (second half of this file: state_from_unet3d_ctx, replay3d, compare3d).  This
module restates it on the CPU in torch fp64, in the order of that method, from a PLAIN state (a dict of NCHW fp64 tensors, no
strides, no pair planes, no padded channels), so that the engine's gradients can be held to what the saved tensors imply
instead of to a second network whose forward differs as well.

  state_from_unet_ctx   GPU ctx -> plain state (only reads tensors)
  unet_forward_state    the same plain state made on the CPU from a state dict and an image (fp64, or with 16-bit storage)
  replay                the backward: every parameter gradient by state-dict name, and dx.  store=dt rounds every tensor
                        the engine keeps in 16 bits between launches where it is stored, carrying the loss scale S
  undecided / d_u       elements whose ReLU sign fp32 cannot decide, and how far the gradients move with them
  compare               err(gpu) <= 4 * e16 + d_U per tensor and per output-channel row

The stage body is the one proven in exact_reference.py (bn_reference): ReLU'(0) = 0 (act_bwd64), the pooled gradient goes to
the first maximum of the 16-bit z in scan order (route_pool2), dy = scale * (gh - c1 - xh * c2) with c1 = s1 / M, c2 = s2 / M,
both zero for running statistics.  Neither S nor 1/S is applied to a result: both are powers of two.
"""
import json
import math
import os
from types import SimpleNamespace

import torch
import torch.nn.functional as F
from torch.nn import grad as G

from tests.exact_reference import act_bwd64, route_pool2

BN_EPS = 1e-5
SIGN_MARGIN = 2.0 ** -21          # |scale*y + shift| below this share of |scale*y| + |shift|: fp32 cannot decide the sign
FLOOR32 = 2.0 ** -20              # see compare()
MUTANTS = ("drop_pool", "swap_halves", "pad_side", "drop_c2", "bias_border", "unflipped", "eighth", "head_pre_relu")
DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def loss_scale(N, H, W):
    return float(2 ** round(math.log2(N * H * W)))


def d64(t):
    return t.detach().to("cpu", torch.float64)


def nchw(t, c=None):
    """a [N, h, w, stride] device tensor -> its first c channels as NCHW fp64: the hi plane of a pair buffer, the real channels
    of a zero-padded image, the two halves of a concat buffer in their order"""
    return d64(t if c is None else t[..., :c]).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ adapters
def _stage(name, wkey, bnkey, inp, y, coef, train_stats, w, wd, image, pooled, dt):
    st = dict(name=name, wkey=wkey, bnkey=bnkey, inp=inp, y=y, scale=d64(coef[0]), shift=d64(coef[1]), mean=d64(coef[2]),
              invstd=d64(coef[3]), train_stats=bool(train_stats), w=w, wd=wd, image=bool(image), z=None)
    if pooled:
        st["z"] = pool_z(st, dt)
    return st


def stage_y(st):
    """the conv output the backward sees: as stored, or re-formed from the image where the stem never stored it"""
    return st["y"] if st["y"] is not None else F.conv2d(st["inp"], st["w"], None, padding=1)


def pool_z(st, dt):
    """the 16-bit z whose maxima route a pooled gradient.  The BatchNorm backward does not read the stored z: it re-forms it
    from y as the forward did, scale * y + shift in one fp32 fma, ReLU, one rounding to the storage type.  (y is a 16-bit number
    and scale an fp32 one, so the fp64 product is exact and the fp64 sum rounded to fp32 is the fma.)"""
    v = stage_y(st) * st["scale"].view(1, -1, 1, 1) + st["shift"].view(1, -1, 1, 1)
    if dt is None:
        return v.clamp_min(0)
    return v.float().clamp_min(0).to(dt).double()


def state_from_unet_ctx(engine, ctx, params):
    """The saved forward of UNetEngine.forward / forward_precise as a plain state."""
    dt = engine.tdt
    from semantic_segmentation_amd.unet import unet_engine as ue
    stages, ups = {}, {}
    for r in ctx["recs"]:
        w = d64(params[r.wkey])
        wide = getattr(r, "wide", 0)
        if r.inp_is_image:
            inp = d64(r.inp)
        else:
            inp = nchw(r.inp, wide if wide else r.cin)           # hi plane / un-padded channels
        pooled = r.name in ("inc.3", "down1.maxpool_conv.1.3", "down2.maxpool_conv.1.3", "down3.maxpool_conv.1.3")
        st = _stage(r.name, r.wkey, r.bnkey, inp, None if r.y is None else nchw(r.y), r.coef, r.train_stats, w,
                    w.to(dt).double(), r.inp_is_image, pooled, dt)
        # the stem's BatchNorm backward and weight gradient in one pass: d(conv output) is never written
        st["fused_stem"] = bool(r.inp_is_image and r.cin == 1 and r.cout == 64 and (r.y is None or ue.FUSED_STEM_BWD))
        stages[r.name] = st
    for u in ctx["ups"]:
        tr = u.geom_bwd is not None
        w = d64(params[u.name + ".up.weight"]) if tr else None
        ups[u.name] = dict(zin=nchw(u.zin, u.cin), pt=u.pt, pl=u.pl, h=u.h, w_=u.w, H2=u.H2, W2=u.W2, transposed=tr, w=w,
                           wd=None if w is None else w.to(dt).double())
    wout = params["outc.conv.weight"]
    ncls = wout.shape[0]
    head = dict(z_last=None if ctx["z_last"] is None else nchw(ctx["z_last"]), w=d64(wout), b=d64(params["outc.conv.bias"]),
                dz_stored=not (ue.FUSED_HEAD_BWD and ncls <= 4))
    return dict(kind="unet", N=ctx["N"], H=ctx["H"], W=ctx["W"], stages=stages, ups=ups, head=head)


def _names():
    enc = [("inc" if i == 0 else f"down{i}.maxpool_conv.1") for i in range(5)]
    return enc


def unet_forward_state(sd, x, train=True, bilinear=False, store=None):
    """The plain state of the reference network's forward (unet_model.py:26-37) made on the CPU in fp64.  store=None: nothing is
    rounded and the statistics are exact, so replay() of it must be torch.autograd through the oracle.  store=dt: y, z and the
    data-gradient weights rounded to dt where the engine stores them, the coefficients to fp32, the statistics taken before the
    rounding as the conv epilogues take them.  Returns (state, logits)."""
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x = x.double()
    N, _, H, W = x.shape

    def r16(t):
        return t if store is None else t.to(store).double()

    def r32(t):
        return t if store is None else t.float().double()

    stages, ups = {}, {}

    def stage(prefix, idx, inp, pooled, image=False):
        wkey, bnkey = f"{prefix}.double_conv.{idx}.weight", f"{prefix}.double_conv.{idx + 1}"
        w = sd[wkey]
        y = F.conv2d(inp, w, None, padding=1)
        if train:
            mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        else:
            mean, var = sd[bnkey + ".running_mean"], sd[bnkey + ".running_var"]
        invstd = torch.rsqrt(var + BN_EPS)
        scale = sd[bnkey + ".weight"] * invstd
        coef = [r32(scale), r32(sd[bnkey + ".bias"] - mean * scale), r32(mean), r32(invstd)]
        st = _stage(f"{prefix}.{idx}", wkey, bnkey, inp, r16(y), coef, train, w, r16(w), image, False, store)
        st["fused_stem"] = bool(image and w.shape[1] == 1 and w.shape[0] == 64)
        z = r16((st["y"] * coef[0].view(1, -1, 1, 1) + coef[1].view(1, -1, 1, 1)).clamp_min(0))
        if pooled:
            st["z"] = pool_z(st, store)
        stages[st["name"]] = st
        return z

    skips, inp = [], (x if x.shape[1] <= 4 else r16(x))      # more than four channels: the image enters as a 16-bit tensor
    for i, prefix in enumerate(_names()):
        zmid = stage(prefix, 0, inp, False, image=(i == 0 and x.shape[1] <= 4))
        z = stage(prefix, 3, zmid, i < 4)
        if i < 4:
            skips.append(z)
            inp = F.max_pool2d(z, 2)
        else:
            inp = z
    for j in range(1, 5):
        skip = skips[4 - j]
        h, w_ = inp.shape[2:]
        H2, W2 = skip.shape[2:]
        pt, pl = (H2 - 2 * h) // 2, (W2 - 2 * w_) // 2
        u = dict(zin=inp, pt=pt, pl=pl, h=h, w_=w_, H2=H2, W2=W2, transposed=not bilinear, w=None, wd=None)
        if bilinear:
            up = F.interpolate(inp, scale_factor=2, mode="bilinear", align_corners=True)
        else:
            u["w"] = sd[f"up{j}.up.weight"]
            u["wd"] = r16(u["w"])
            up = F.conv_transpose2d(inp, u["w"], sd[f"up{j}.up.bias"], stride=2)
        ups[f"up{j}"] = u
        up = r16(F.pad(up, [pl, W2 - 2 * w_ - pl, pt, H2 - 2 * h - pt]))
        zmid = stage(f"up{j}.conv", 0, torch.cat([skip, up], 1), False)
        inp = stage(f"up{j}.conv", 3, zmid, False)
    wout = sd["outc.conv.weight"]
    logits = F.conv2d(inp, wout, sd["outc.conv.bias"])
    # as the engine: up to four classes the last activation is never stored and the head's data gradient never written
    fused = wout.shape[0] <= 4
    head = dict(z_last=None if fused else inp, w=wout, b=sd["outc.conv.bias"], dz_stored=not fused)
    return dict(kind="unet", N=N, H=H, W=W, stages=stages, ups=ups, head=head), logits


# ------------------------------------------------------------------------------------------------ the backward
def undecided(state):
    """{stage: mask} of the elements whose sign of scale*y + shift fp32 cannot decide (SIGN_MARGIN), and their count"""
    masks, n = {}, 0
    for name, st in state["stages"].items():
        sy = stage_y(st) * st["scale"].view(1, -1, 1, 1)
        sh = st["shift"].view(1, -1, 1, 1)
        m = (sy + sh).abs() < SIGN_MARGIN * (sy.abs() + sh.abs())
        if bool(m.any()):
            masks[name] = m
            n += int(m.sum())
    return masks, n


def replay(state, dlogits, need_dx, store=None, S=None, mutant=None, force=None):
    """UNetEngine.backward in fp64 -> ({state-dict name: gradient}, dx or None).
    store: the 16-bit type in which dy, dinp / dmid / dcat / dpool, the up steps' dz and the head's dz (where it is written at
    all) are rounded, as S * value; S: the loss scale (default 2^round(log2(N*H*W)), times the renormalisation factor under
    dynamic_loss_scale).  Never stored, hence never rounded: dl (fp32), the fused head's dz (formed inside the BatchNorm backward
    of the last stage), the fused stem's dy (consumed by the weight gradient in the same pass), the image gradient (fp32).
    mutant: one of MUTANTS, a backward that is wrong in one stated way.  force: (masks from undecided(), bool) -- ReLU' of those
    elements taken as 1 / 0."""
    assert mutant is None or mutant in MUTANTS
    N, H, W = state["N"], state["H"], state["W"]
    S = loss_scale(N, H, W) if S is None else S
    stages, ups, head = state["stages"], state["ups"], state["head"]
    grads = {}

    def rnd(t):
        return t if store is None else (t * S).to(store).double() / S

    def stage_bwd(st, g, dzp, need_dinp, g_stored=True):
        y = stage_y(st)
        col = lambda t: t.view(1, -1, 1, 1)                                               # noqa: E731
        scale, shift, mean, invstd = col(st["scale"]), col(st["shift"]), col(st["mean"]), col(st["invstd"])
        v = y * scale + shift
        if dzp is not None and not (mutant == "drop_pool" and st["name"] == "down1.maxpool_conv.1.3"):
            g = g + route_pool2(st["z"], dzp)[0]
        gh = act_bwd64(g, v, "relu")
        if force is not None and st["name"] in force[0]:
            gh = torch.where(force[0][st["name"]], g if force[1] else torch.zeros_like(g), gh)
        xh = (y - mean) * invstd
        s1, s2 = gh.sum((0, 2, 3)), (gh * xh).sum((0, 2, 3))
        grads[st["bnkey"] + ".weight"], grads[st["bnkey"] + ".bias"] = s2, s1
        M = y.shape[0] * y.shape[2] * y.shape[3]
        c1, c2 = (s1 / M, s2 / M) if st["train_stats"] else (torch.zeros_like(s1), torch.zeros_like(s2))
        if mutant == "drop_c2" and st["name"] == "up2.conv.0":
            c2 = torch.zeros_like(c2)
        dy = scale * (gh - col(c1) - xh * col(c2))
        fused = st["image"] and st.get("fused_stem") and not need_dinp
        if not fused:
            dy = rnd(dy)
        inp = st["inp"]
        dyw = dy
        if mutant == "eighth" and st["name"] == "up3.conv.3":
            dyw = dy.clone()
            dyw.view(dy.shape[0], dy.shape[1], -1)[:, :, ::8] = 0
        grads[st["wkey"]] = G.conv2d_weight(inp, st["w"].shape, dyw, padding=1)
        if not need_dinp:
            return None
        if st["image"]:
            return G.conv2d_input(inp.shape, st["w"], dy, padding=1)                     # fp32 weights, fp32 image gradient
        wd = st["wd"].flip(2, 3) if (mutant == "unflipped" and st["name"] == "up1.conv.3") else st["wd"]
        return rnd(G.conv2d_input(inp.shape, wd, dy, padding=1))

    # ---- head ----
    dl = dlogits.double()
    last = stages["up4.conv.3"]
    if head["z_last"] is not None:
        z_last = head["z_last"]
    else:
        z_last = (stage_y(last) * last["scale"].view(1, -1, 1, 1) + last["shift"].view(1, -1, 1, 1))
        if mutant != "head_pre_relu":
            z_last = z_last.clamp_min(0)
    if mutant == "head_pre_relu" and head["z_last"] is not None:
        z_last = stage_y(last) * last["scale"].view(1, -1, 1, 1) + last["shift"].view(1, -1, 1, 1)
    grads["outc.conv.weight"] = G.conv2d_weight(z_last, head["w"].shape, dl)
    grads["outc.conv.bias"] = dl.sum((0, 2, 3))
    dz = G.conv2d_input(z_last.shape, head["w"], dl)
    if head["dz_stored"]:
        dz = rnd(dz)

    # ---- decoder, reversed ----
    dcats = [None] * 4
    for j in range(4, 0, -1):
        lvl = 4 - j
        prefix = f"up{j}"
        dmid = stage_bwd(stages[prefix + ".conv.3"], dz, None, True)
        dcat = stage_bwd(stages[prefix + ".conv.0"], dmid, None, True)
        u = ups[prefix]
        C = dcat.shape[1] // 2
        skip_half, up_half = dcat[:, :C], dcat[:, C:]
        if mutant == "swap_halves" and j == 3:
            skip_half, up_half = up_half, skip_half
        dcats[lvl] = skip_half
        pt, pl = u["pt"], u["pl"]
        if mutant == "pad_side":
            # four floor halvings leave H2 - 2h in {0, 1}, so pt = pl = 0 in every U-Net and a dropped offset cannot show; the
            # same slip that can is the odd row / column of padding put in front of the patch instead of behind it
            pt, pl = u["H2"] - 2 * u["h"] - pt, u["W2"] - 2 * u["w_"] - pl
        dU = up_half[:, :, pt:pt + 2 * u["h"], pl:pl + 2 * u["w_"]]                       # the un-padded patch only
        if not u["transposed"]:
            # the transposed interpolation: the vector-Jacobian product of the reference's own up-sampling call
            zin = u["zin"].detach().clone().requires_grad_(True)
            up = F.interpolate(zin, scale_factor=2, mode="bilinear", align_corners=True)
            dz = rnd(torch.autograd.grad(up, zin, dU.contiguous())[0])
            continue
        grads[prefix + ".up.bias"] = (up_half if mutant == "bias_border" else dU).sum((0, 2, 3))
        # ConvTranspose2d(k2, s2) seen from its output side is a stride-2 conv dU -> x with the same [cin, cout, 2, 2] weight
        grads[prefix + ".up.weight"] = G.conv2d_weight(dU, u["w"].shape, u["zin"], stride=2)
        dz = rnd(F.conv2d(dU, u["wd"], None, stride=2))

    # ---- encoder, reversed ----
    dpool = None
    for i in range(4, -1, -1):
        prefix = _names()[i]
        if i == 4:
            dmid = stage_bwd(stages[prefix + ".3"], dz, None, True)
        else:
            dmid = stage_bwd(stages[prefix + ".3"], dcats[i], dpool, True)
        dinp = stage_bwd(stages[prefix + ".0"], dmid, None, i > 0 or need_dx)
        dpool = dinp
    return grads, (dinp if need_dx else None)


# ------------------------------------------------------------------------------------------------ comparer
def _err(a, ref):
    n = float(ref.norm())
    d = float((a - ref).norm())
    return d / n if n > 0 else (0.0 if d == 0 else float("inf"))


def replays(state, dlogits, need_dx, store, S=None):
    """(R64, R16, d_U per tensor, count of undecided elements): what compare() needs besides the result under test"""
    def flat(gd):
        g, dx = gd
        out = dict(g)
        if dx is not None:
            out["dx"] = dx
        return out
    r64 = flat(replay(state, dlogits, need_dx, None, S))
    r16 = flat(replay(state, dlogits, need_dx, store, S))
    masks, n_und = undecided(state)
    d_u = {k: 0.0 for k in r64}
    if n_und:
        on = flat(replay(state, dlogits, need_dx, None, S, force=(masks, True)))
        off = flat(replay(state, dlogits, need_dx, None, S, force=(masks, False)))
        d_u = {k: float((on[k] - off[k]).norm()) / max(float(r64[k].norm()), 1e-300) for k in r64}
    return r64, r16, d_u, n_und


def compare(got, r64, r16, d_u):
    """err(a) = |a - R64|_2 / |R64|_2, e16 = err(R16).  Per tensor:
        err(got) <= 4 * e16 + d_U
    (four times the reference's own 16-bit error: fp32 accumulation order and coefficients, an equally valid rounding point).
    One floor under e16, FLOOR32 / 4 with FLOOR32 = 2^-20: a tensor with no 16-bit store between dlogits and itself (the head's
    bias gradient, its weight gradient over the never-stored last activation) has e16 = 0 exactly, while the engine sums it in
    fp32; 2^-20 is 16 fp32 unit roundoffs, the relative L2 error of an fp32 sum of a few thousand to a million terms in any
    order, and 500 times below a 16-bit roundoff, so no fault this comparer is for hides under it.
    Per output-channel row of a weight of two or more dimensions, in absolute terms:
        |got - R64|_row <= max(4 * |R16 - R64|_row + d_U * |R64|_row,  bound of the tensor * RMS row norm * sqrt(2 ln 2R)).
    A row's own 16-bit error is made by as few roundings as its channel has pixels (four at a 2 x 2 level): it is near zero by
    chance for some rows and no stable figure, so the tensor's takes over there; the largest of R independent row errors of
    one RMS is sqrt(2 ln 2R) of that RMS (3.9 at R = 1024).  Rows of small norm need no rule of their own.
    Returns ({name: dict(err, e16, ratio, d_u, bound, row_worst, ok)}, [failures]); ratio = err / max(e16, FLOOR32 / 4),
    row_worst = the largest row error as a share of its bound."""
    rep, bad = {}, []
    for k, ref in r64.items():
        a = d64(got[k]).reshape(ref.shape)
        e16, du = _err(r16[k], ref), d_u.get(k, 0.0)
        bound = 4 * max(e16, FLOOR32 / 4) + du
        err = _err(a, ref)
        row_worst = 0.0
        if ref.dim() >= 2:
            rn = ref.reshape(ref.shape[0], -1).norm(dim=1)
            dn = (a - ref).reshape(ref.shape[0], -1).norm(dim=1)
            e16r = (r16[k] - ref).reshape(ref.shape[0], -1).norm(dim=1)
            rms = float(rn.pow(2).mean().sqrt())
            tail = math.sqrt(2 * math.log(2 * ref.shape[0]))
            rr = dn / (torch.maximum(4 * e16r + du * rn, torch.full_like(rn, bound * rms * tail))).clamp_min(1e-300)
            row_worst = float(rr.max())
        ok = err <= bound and row_worst <= 1.0
        rep[k] = dict(err=err, e16=e16, ratio=err / max(e16, FLOOR32 / 4), d_u=du, bound=bound, row_worst=row_worst, ok=bool(ok))
        if not ok:
            bad.append(k)
    return rep, bad


def engine_like(dtype="f16", n_classes=2):
    """what the adapters read of an engine, for CPU tensors laid out as the engine lays its own out"""
    return SimpleNamespace(tdt=DT[dtype], dtype=dtype, net=SimpleNamespace(n_classes=n_classes))


REPORT = {}


def record(key, rep, n_und):
    """the ratios err(gpu) / e16 of one configuration into parity_reports/backward_replay.json (every configuration of the
    session so far: the file is rewritten each time)"""
    REPORT[key] = dict(undecided=n_und, worst_ratio=max(r["ratio"] for r in rep.values() if not r.get("absolute")),
                       tensors={k: {f: r[f] for f in ("err", "e16", "ratio", "d_u", "row_worst")} for k, r in rep.items()})
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parity_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "backward_replay.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


# ================================================================================================ UNet3D
# The same replay for UNet3DEngine.backward(ctx, dlogits): [NB*D, H, W, C] buffers become NCDHW; the concat buffers hold the
# up-sampled channels FIRST ([up | residual], unet3d.py:77); a decoder block's two stages share one BatchNorm3d, whose two
# gradient contributions are summed; the convs carry a bias the kernels never add (it cancels in front of batch statistics and
# sits in the shift in eval mode), so y is the conv output without it.
MUTANTS3D = ("shared_bn_replace", "swap_halves", "drop_pool")
A_BLOCKS = ("a_block1", "a_block2", "a_block3")


def ncdhw(t, NB, c0=0, c1=None):
    """[NB*D, H, W, stride] -> channels [c0, c1) as [NB, C, D, H, W] fp64"""
    t = t[..., c0:c1]
    return d64(t).view(NB, t.shape[0] // NB, t.shape[1], t.shape[2], t.shape[3]).permute(0, 4, 1, 2, 3).contiguous()


def _stage3(name, inp, y, coef, train_stats, w, wd, b_name, first):
    blk, conv = name.split(".")
    bn = blk + (".bn" if blk.startswith("s_block") else ".bn" + conv[-1])
    return dict(name=name, wkey=name + ".weight", bkey=b_name, bnkey=bn, inp=inp, y=y, scale=d64(coef[0]), shift=d64(coef[1]),
                mean=d64(coef[2]), invstd=d64(coef[3]), train_stats=bool(train_stats), w=w, wd=wd, first=bool(first))


def state_from_unet3d_ctx(engine, ctx):
    """The saved forward of UNet3DEngine.forward / forward_pair as a plain state."""
    dt, NB = engine.tdt, ctx["NB"]
    names = {id(p): n for n, p in engine.param_items()}
    pair = bool(ctx.get("pair"))
    stages = {}
    for s in ctx["stages"]:
        wname = names[id(s.conv.weight)]
        w = d64(s.conv.weight)
        if s.first:
            inp = d64(s.inp)                                          # the fp32 volume [NB, 1, D, H, W]
        else:
            c0 = s.in_coff
            inp = ncdhw(s.inp, NB, c0, c0 + (s.wide if s.wide else s.cin))      # hi plane / un-padded channels
        stages[wname[:-7]] = _stage3(wname[:-7], inp, ncdhw(s.y, NB), s.coef, s.stats, w, w.to(dt).double(),
                                     None if s.conv.bias is None else names[id(s.conv.bias)], s.first)
    ups, pool_z3 = {}, {}
    for k, u in ctx["ups"].items():
        up = engine.submodule(f"s_block{k}.upconv1")
        w = d64(up.weight)
        ups[k] = dict(zin=ncdhw(u["zin"], NB, 0, u["cin"]), cup=u["cup"], w=w, wd=w.to(dt).double())
        cat = ctx["cats"][k]
        ctot = cat.shape[3] // 2 if pair else cat.shape[3]
        pool_z3[k] = ncdhw(cat, NB, u["cup"], ctot)                   # the stored residual z (hi plane) the pool routing reads
    head = engine.submodule("s_block1.conv3")
    hd = dict(z_last=ncdhw(ctx["z_last"], NB), w=d64(head.weight), b=d64(head.bias))
    return dict(kind="unet3d", NB=NB, dims=[tuple(d) for d in ctx["dims"]], stages=stages, ups=ups, pool_z=pool_z3, head=hd)


def unet3d_forward_state(sd, x, train=True, store=None):
    """unet3d.py:111-123 on the CPU in fp64 as a plain state (store as in unet_forward_state).  Returns (state, logits)."""
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x = x.double()
    NB, cin0, D0, H0, W0 = x.shape
    r16 = (lambda t: t) if store is None else (lambda t: t.to(store).double())
    r32 = (lambda t: t) if store is None else (lambda t: t.float().double())
    stages, ups, pool_z3 = {}, {}, {}

    def stage(name, inp, first=False):
        w, b = sd[name + ".weight"], sd[name + ".bias"]
        y = F.conv3d(inp, w, None, padding=1)
        st = _stage3(name, inp, None, [w.new_zeros(1)] * 4, train, w, r16(w), name + ".bias", first)
        bn = st["bnkey"]
        if train:
            mean, var = y.mean((0, 2, 3, 4)), y.var((0, 2, 3, 4), unbiased=False)
        else:
            mean, var = sd[bn + ".running_mean"] - b, sd[bn + ".running_var"]
        invstd = torch.rsqrt(var + BN_EPS)
        scale = sd[bn + ".weight"] * invstd
        st.update(y=r16(y), scale=r32(scale), shift=r32(sd[bn + ".bias"] - mean * scale), mean=r32(mean), invstd=r32(invstd))
        stages[name] = st
        col = lambda t: t.view(1, -1, 1, 1, 1)                                            # noqa: E731
        return r16((st["y"] * col(st["scale"]) + col(st["shift"])).clamp_min(0))

    res, inp = {}, (x if cin0 == 1 else r16(x))
    for k, p in enumerate(A_BLOCKS + ("bottleNeck",), 1):
        z = stage(p + ".conv2", stage(p + ".conv1", inp, first=(k == 1 and cin0 == 1)))
        if k <= 3:
            res[k] = pool_z3[k] = z
            inp = F.max_pool3d(z, 2)
        else:
            inp = z
    for k in (3, 2, 1):
        p = f"s_block{k}"
        w = sd[p + ".upconv1.weight"]
        ups[k] = dict(zin=inp, cup=w.shape[1], w=w, wd=r16(w))
        up = r16(F.conv_transpose3d(inp, w, sd[p + ".upconv1.bias"], stride=2))
        inp = stage(p + ".conv2", stage(p + ".conv1", torch.cat((up, res[k]), 1)))
    w, b = sd["s_block1.conv3.weight"], sd["s_block1.conv3.bias"]
    logits = F.conv3d(inp, w, b)
    state = dict(kind="unet3d", NB=NB, dims=[(D0 >> k, H0 >> k, W0 >> k) for k in range(4)], stages=stages, ups=ups,
                 pool_z=pool_z3, head=dict(z_last=inp, w=w, b=b))
    return state, logits


def replay3d(state, dlogits, store=None, S=None, mutant=None, force=None):
    """UNet3DEngine.backward in fp64 -> {state-dict name: gradient}.  Every tensor between two launches is stored in 16 bits
    there (no fused head or stem): dy, dmid / dcat / dpool, the up steps' dz, the head's dz and the pool's dz2.  Returns also
    {conv bias name: sum |dy|} of the stages with batch statistics, for the one allowance of compare()."""
    assert mutant is None or mutant in MUTANTS3D
    NB, (D0, H0, W0) = state["NB"], state["dims"][0]
    S = loss_scale(NB * D0, H0, W0) if S is None else S
    stages, ups = state["stages"], state["ups"]
    grads, bias_scale = {}, {}
    rnd = (lambda t: t) if store is None else (lambda t: (t * S).to(store).double() / S)
    col = lambda t: t.view(1, -1, 1, 1, 1)                                                # noqa: E731

    def stage_bwd(st, g, need_dinp=True):
        y = st["y"]
        scale, shift, mean, invstd = col(st["scale"]), col(st["shift"]), col(st["mean"]), col(st["invstd"])
        gh = act_bwd64(g, y * scale + shift, "relu")
        if force is not None and st["name"] in force[0]:
            gh = torch.where(force[0][st["name"]], g if force[1] else torch.zeros_like(g), gh)
        xh = (y - mean) * invstd
        s1, s2 = gh.sum((0, 2, 3, 4)), (gh * xh).sum((0, 2, 3, 4))
        for key, val in ((st["bnkey"] + ".weight", s2), (st["bnkey"] + ".bias", s1)):
            # the shared BatchNorm3d of a decoder block: the second contribution is ADDED to the first
            grads[key] = val if (key not in grads or mutant == "shared_bn_replace") else grads[key] + val
        M = y.numel() // y.shape[1]
        c1, c2 = (s1 / M, s2 / M) if st["train_stats"] else (torch.zeros_like(s1), torch.zeros_like(s2))
        dy = rnd(scale * (gh - col(c1) - xh * col(c2)))
        if st["bkey"] is not None:
            grads[st["bkey"]] = dy.sum((0, 2, 3, 4))
            if st["train_stats"]:
                bias_scale[st["bkey"]] = float(dy.abs().sum())
        grads[st["wkey"]] = G.conv3d_weight(st["inp"], st["w"].shape, dy, padding=1)
        if not need_dinp:
            return None
        return rnd(G.conv3d_input(st["inp"].shape, st["wd"], dy, padding=1))

    hd = state["head"]
    dl = dlogits.double()
    grads["s_block1.conv3.weight"] = G.conv3d_weight(hd["z_last"], hd["w"].shape, dl)
    grads["s_block1.conv3.bias"] = dl.sum((0, 2, 3, 4))
    dz = rnd(G.conv3d_input(hd["z_last"].shape, hd["w"], dl))
    dres = {}
    for k in (1, 2, 3):
        p = f"s_block{k}"
        dcat = stage_bwd(stages[p + ".conv1"], stage_bwd(stages[p + ".conv2"], dz))
        u = ups[k]
        dU, dres[k] = dcat[:, :u["cup"]], dcat[:, u["cup"]:]
        if mutant == "swap_halves" and k == 2:                      # the halves taken as if the buffer were [residual | up]
            dU, dres[k] = dcat[:, -u["cup"]:], dcat[:, :dcat.shape[1] - u["cup"]]
        grads[p + ".upconv1.bias"] = dU.sum((0, 2, 3, 4))
        # ConvTranspose3d(k2, s2) seen from its output side: a stride-2 conv dU -> x with the same [cin, cup, 2, 2, 2] weight
        grads[p + ".upconv1.weight"] = G.conv3d_weight(dU, u["w"].shape, u["zin"], stride=2)
        dz = rnd(F.conv3d(dU, u["wd"], None, stride=2))
    dpool = stage_bwd(stages["bottleNeck.conv1"], stage_bwd(stages["bottleNeck.conv2"], dz))
    for k in (3, 2, 1):
        p = A_BLOCKS[k - 1]
        # MaxPool3d(2) backward as torch routes it (first maximum of the stored 16-bit z in scan order), plus the residual half
        z = state["pool_z"][k].detach().clone().requires_grad_(True)
        routed = torch.autograd.grad(F.max_pool3d(z, 2), z, dpool)[0]
        if mutant == "drop_pool" and k == 2:
            routed = torch.zeros_like(routed)
        dz2 = rnd(dres[k] + routed)
        dpool = stage_bwd(stages[p + ".conv1"], stage_bwd(stages[p + ".conv2"], dz2), need_dinp=k > 1)
    return grads, bias_scale


def undecided3d(state):
    masks, n = {}, 0
    for name, st in state["stages"].items():
        sy = st["y"] * st["scale"].view(1, -1, 1, 1, 1)
        sh = st["shift"].view(1, -1, 1, 1, 1)
        m = (sy + sh).abs() < SIGN_MARGIN * (sy.abs() + sh.abs())
        if bool(m.any()):
            masks[name] = m
            n += int(m.sum())
    return masks, n


def replays3d(state, dlogits, store, S=None):
    """(R64, R16, d_U per tensor, undecided count, {conv bias name: sum |dy|})"""
    r64, bias_scale = replay3d(state, dlogits, None, S)
    r16, _ = replay3d(state, dlogits, store, S)
    masks, n_und = undecided3d(state)
    d_u = {k: 0.0 for k in r64}
    if n_und:
        on = replay3d(state, dlogits, None, S, force=(masks, True))[0]
        off = replay3d(state, dlogits, None, S, force=(masks, False))[0]
        d_u = {k: float((on[k] - off[k]).norm()) / max(float(r64[k].norm()), 1e-300) for k in r64}
    return r64, r16, d_u, n_und, bias_scale


def compare3d(got, r64, r16, d_u, bias_scale, dt):
    """compare() with the one allowance: the bias of a conv in front of a batch-statistics BatchNorm has gradient zero up to
    noise (the engine returns exact zeros), held in absolute terms to 2 * u(dt) * sum |dy| of its stage (u = 2^-11 / 2^-8)."""
    tol = 2.0 * (2.0 ** -11 if dt == torch.float16 else 2.0 ** -8)
    plain = [k for k in r64 if k not in bias_scale]
    rep, bad = compare({k: got[k] for k in plain}, {k: r64[k] for k in plain}, {k: r16[k] for k in plain}, d_u)
    for k, sc in bias_scale.items():
        worst = float((d64(got[k]) - r64[k]).abs().max())
        ok = worst <= tol * sc
        rep[k] = dict(err=worst, e16=0.0, ratio=worst / (tol * sc) if sc else 0.0, d_u=0.0, bound=tol * sc, row_worst=0.0, ok=ok,
                      absolute=True)
        if not ok:
            bad.append(k)
    return rep, bad
