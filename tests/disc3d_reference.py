"""Case lists and exact references for the kernels of the 3-D Pix2Pix discriminators (GenSeg-3D/models/networks.py:806-890 with a 3-D
norm layer): the image-side conv of csrc/ends_img.hip (gs_conv3d_img_fwd / _wgrad / _dgrad), the one-channel head of csrc/ends3d.hip
(gs_conv3d_head_fwd / _bwd) and the middle convs on the generic engine through ops.geom_conv3d / geom_conv3d_dgrad_s1 / geom_conv3d_s2_dgrad_class -- on
tests/exact_reference.py's construction: integer operands whose fp32 sums are exact in any order, so a kernel has to give the one
correctly rounded value.  Shared by tests/test_disc3d_kernels_gpu.py (kernel against reference, zero tolerance) and
tests/test_disc3d_reference_cpu.py (every case meets its conditions; the references equal autograd; the stated wrong implementations
do not pass)."""
import functools

import torch
import torch.nn.functional as F

from tests import exact_reference as er

GEOM = {4: (2, 1), 1: (1, 0)}                       # image side: k -> (stride, pad)
HEAD_PAD = {4: 1, 1: 0}                             # head: k -> pad (stride 1)
GSCALE = 0.25                                       # the loss-scale factor of the gradient cases (a power of two, != 1)


def slices(t: torch.Tensor) -> torch.Tensor:
    """[N, C, D, H, W] -> [N*D, H, W, C] contiguous: the engine's stack of depth slices"""
    cl = er.channels_last(t)
    return cl.reshape(cl.shape[0] * cl.shape[1], *cl.shape[2:])


def volumes(t: torch.Tensor, N: int) -> torch.Tensor:
    """[N*D, H, W, C] -> [N, C, D, H, W]: the adapter back from the engine's buffers"""
    ND, H, W, C = t.shape
    return t.reshape(N, ND // N, H, W, C).permute(0, 4, 1, 2, 3).contiguous()


# ================================================================================================ image side
# (Cin, Cout, k, N, (D, H, W)).  Cin: 1, 2 (the reference's real | fake pair), 3, 5, 16 (one data-gradient register form each: 2, 2, 4,
# 8, 16; an odd and an even count of 2-channel weight-gradient chunks).  Cout: every tile count 1..4 with and without a ragged last
# tile; 72 and 128 take a second 64-channel chunk in the data gradient.  Volumes: 2^3 (ONE output voxel: every tap but the centre
# 2 x 2 x 2 in the pad), 5 x 7 x 9 (odd: the far pad is reached on no axis, the last input slice / row / column is read by no tap),
# 6 x 10 x 70 (output 3 x 5 x 35: output width 35 crosses a 32-column patch, 5 rows cross a 4-row weight-gradient patch), and
# 40 x 18 x 70 (360 weight-gradient patches: more than the 256 blocks, so blocks walk several patches).  k1 at 3 x 4 x 5 and 2 x 3 x 70.
IMG_CASES = [
    (1, 8, 4, 1, (2, 2, 2)), (2, 64, 4, 3, (5, 7, 9)), (3, 72, 4, 3, (6, 10, 70)), (5, 128, 4, 3, (5, 7, 9)),
    (16, 128, 4, 1, (6, 10, 70)), (16, 64, 4, 3, (2, 2, 2)), (2, 64, 4, 1, (6, 10, 70)), (1, 72, 4, 3, (5, 7, 9)),
    (3, 8, 4, 3, (2, 2, 2)), (2, 8, 4, 3, (40, 18, 70)),
    (1, 64, 1, 3, (3, 4, 5)), (2, 8, 1, 1, (2, 3, 70)), (3, 72, 1, 3, (3, 4, 5)), (5, 128, 1, 3, (2, 3, 70)), (16, 64, 1, 1, (3, 4, 5)),
]


def img_id(c):
    Cin, Cout, k, N, (D, H, W) = c
    return f"cin{Cin}_cout{Cout}_k{k}_n{N}_{D}x{H}x{W}"


def img_out(c):
    Cin, Cout, k, N, vol = c
    s, p = GEOM[k]
    return tuple(er.out_size(v, k, s, p) for v in vol)


def conv3d_fn(k, s, p):
    return lambda x, w: F.conv3d(x, w, None, stride=s, padding=p)


@functools.lru_cache(maxsize=None)
def img_build(c, vset="S"):
    """operands x, w, b, dy and the fp64 references y, dx, dw of an image-side case (computed once; treat as read-only)"""
    Cin, Cout, k, N, vol = c
    OD, OH, OW = img_out(c)
    s, p = GEOM[k]
    # products per element: y k^3 Cin; dx at most k^3 Cout (bounded from above); dw one per output voxel
    return er.conv_case(("img3d",) + tuple(c), vset, (N, Cin) + tuple(vol), (Cout, Cin, k, k, k), conv3d_fn(k, s, p), k ** 3 * Cin,
                        k ** 3 * Cout, N * OD * OH * OW, bias=True)


# ================================================================================================ one-channel head
# (Cin, k, (D, H, W)), N = 2.  Cin 8 (one group), 64, 512 (the PatchGAN's), 1024 (the most).  Volumes 2^3 -> one logit (every tap but
# the centre 2^3... of the 4^3 in the pad or outside), 3^3 -> 2^3, 4 x 5 x 9 -> 3 x 4 x 8 (192 logits: three weight-gradient parts).
HEAD_N = 2
HEAD_CASES = [
    (8, 4, (2, 2, 2)), (64, 4, (3, 3, 3)), (512, 4, (4, 5, 9)), (1024, 4, (3, 3, 3)), (64, 4, (4, 5, 9)), (8, 4, (4, 5, 9)),
    (1024, 4, (2, 2, 2)),
    (8, 1, (3, 4, 5)), (64, 1, (3, 4, 5)), (512, 1, (3, 4, 5)), (1024, 1, (3, 4, 5)),
]


def head_id(c):
    Cin, k, (D, H, W) = c
    return f"cin{Cin}_k{k}_{D}x{H}x{W}"


def head_out(c):
    Cin, k, vol = c
    return tuple(er.out_size(v, k, 1, HEAD_PAD[k]) for v in vol)


@functools.lru_cache(maxsize=None)
def head_build(c, vset="S"):
    """x, w, b, dy (= the logit gradient) and the fp64 references y, dx, dw, db of a head case"""
    Cin, k, vol = c
    OD, OH, OW = head_out(c)
    r = er.conv_case(("head3d",) + tuple(c), vset, (HEAD_N, Cin) + tuple(vol), (1, Cin, k, k, k), conv3d_fn(k, 1, HEAD_PAD[k]),
                     k ** 3 * Cin, k ** 3, HEAD_N * OD * OH * OW, bias=True)
    er.require_channel_sums(r["dy"], "head3d db", squares=False)
    r["db"] = r["dy"].double().sum((0, 2, 3, 4))
    return r


# ================================================================================================ middle convs on the generic engine
# (Cin, Cout, stride, (D, H, W)), N = 2, k 4, pad 1.  4 x 6 x 10 (even: every stride-2 class has the same voxel count) and 7 x 5 x 9
# (odd: the classes differ in size, the far pad is not reached).
ENGINE_N = 2
ENGINE_CASES = [(cin, cout, s, vol) for (cin, cout) in ((8, 16), (64, 128)) for s in (2, 1) for vol in ((4, 6, 10), (7, 5, 9))]


def engine_id(c):
    Cin, Cout, s, (D, H, W) = c
    return f"cin{Cin}_cout{Cout}_s{s}_{D}x{H}x{W}"


def engine_out(c):
    Cin, Cout, s, vol = c
    return tuple(er.out_size(v, 4, s, 1) for v in vol)


@functools.lru_cache(maxsize=None)
def engine_build(c, vset="S"):
    Cin, Cout, s, vol = c
    OD, OH, OW = engine_out(c)
    return er.conv_case(("engine3d",) + tuple(c), vset, (ENGINE_N, Cin) + tuple(vol), (Cout, Cin, 4, 4, 4), conv3d_fn(4, s, 1), 64 * Cin,
                        64 * Cout, ENGINE_N * OD * OH * OW, bias=True)


def pack_slots(w: torch.Tensor, dgrad: bool) -> torch.Tensor:
    """[Cout][Cin][k][k][k] -> the engine's pack [k^3][Cout][Cin] (dgrad: [k^3][Cin][Cout]), slot = (kz*k + ky)*k + kx"""
    Cout, Cin = w.shape[0], w.shape[1]
    t = w.reshape(Cout, Cin, -1)
    return (t.permute(2, 1, 0) if dgrad else t.permute(2, 0, 1)).contiguous()


# ================================================================================================ the wrong implementations
# Each a function with the right one's signature; tests/test_disc3d_reference_cpu.py proves that the case lists tell them from it.
def fwd_right(x, w, b, k, s, p):
    return F.conv3d(x, w, b, stride=s, padding=p)


def fwd_kz_ky_exchanged(x, w, b, k, s, p):
    """kz and ky exchanged"""
    return fwd_right(x, w.transpose(2, 3), b, k, s, p)


def _past_the_end(x, od, k, s, first):
    """output slices whose taps, starting at input slice `first` + s * od, reach past the last input slice"""
    return [o for o in range(od) if first + s * o + k - 1 >= x.shape[2]]


def fwd_depth_pad_front_missing(x, w, b, k, s, p):
    """the depth pad missing in front, all of it on the far side: output slice od reads from input slice s * od instead of s * od - p,
    what then falls past the far end reads zeros"""
    if p == 0:
        return fwd_right(x, w, b, k, s, p)
    return fwd_right(F.pad(x, (0, 0, 0, 0, 0, p))[:, :, p:], w, b, k, s, p)


def fwd_depth_pad_far_missing(x, w, b, k, s, p):
    """the depth pad in front only: an output slice that needs the far pad is not produced (zeros).  The right function where the far pad
    is not reached (odd depths at stride 2)"""
    y = fwd_right(x, w, b, k, s, p).clone()
    if p:
        y[:, :, _past_the_end(x, y.shape[2], k, s, -p)] = 0
    return y


def fwd_depth_pad_missing(x, w, b, k, s, p):
    """no depth pad on either side: output slice od reads from input slice s * od, and a slice whose taps reach past the end is not
    produced (zeros)"""
    y = fwd_depth_pad_front_missing(x, w, b, k, s, p).clone()
    if p:
        y[:, :, _past_the_end(x, y.shape[2], k, s, 0)] = 0
    return y


def far_pad_reached(depth, k, s, p):
    return s * ((depth + 2 * p - k) // s) - p + k - 1 >= depth


def fwd_depth_stride_1(x, w, b, k, s, p):
    """stride 1 along depth: output slice d reads input slices d - p .. (shown on the slices both have)"""
    if s == 1:
        return fwd_right(x, w, b, k, s, p)
    y = F.conv3d(x, w, b, stride=(1, s, s), padding=p)
    return y[:, :, :(x.shape[2] + 2 * p - k) // s + 1]


def fwd_bias_dropped(x, w, b, k, s, p):
    return fwd_right(x, w, None, k, s, p)


FWD_MUTANTS = {"kz/ky exchanged": fwd_kz_ky_exchanged, "depth pad missing": fwd_depth_pad_missing,
               "depth pad on the far side only": fwd_depth_pad_front_missing, "depth pad in front only": fwd_depth_pad_far_missing,
               "depth stride 1": fwd_depth_stride_1, "bias dropped": fwd_bias_dropped}


def dgrad_right(dy, w, x_shape, k, s, p):
    return torch.nn.grad.conv3d_input(x_shape, w, dy, stride=s, padding=p)


def dgrad_depth_taps_unflipped(dy, w, x_shape, k, s, p):
    """the data gradient with its depth taps not flipped (kz read in the forward's order)"""
    return dgrad_right(dy, w.flip(2), x_shape, k, s, p)


def dgrad_depth_classes_exchanged(dy, w, x_shape, k, s, p):
    """the sub-voxel classes exchanged along depth: even slices use the odd slices' taps"""
    if s == 1:
        return dgrad_right(dy, w, x_shape, k, s, p)
    return dgrad_right(dy, w[:, :, [1, 0, 3, 2]], x_shape, k, s, p)


DGRAD_MUTANTS = {"depth taps un-flipped": dgrad_depth_taps_unflipped, "depth classes exchanged": dgrad_depth_classes_exchanged}


def db_right(dy):
    return dy.sum((0, 2, 3, 4))


def db_without_border(dy):
    """first-layer bias gradient summed without the border voxels"""
    if min(dy.shape[2:]) < 3:
        return dy.sum((0, 2, 3, 4)) * 0
    return dy[:, :, 1:-1, 1:-1, 1:-1].sum((0, 2, 3, 4))


# ================================================================================================ the networks: an fp64 statement
# Both 3-D discriminators under both norms on the CPU, from a state dict and a volume, as a PLAIN state (NCDHW fp64 tensors) -- the
# 3-D twin of pix2pix_backward_replay.discriminator_forward_state / instnorm_reference.discriminator_forward_state /
# pixel_reference.forward_state -- and the hand-derived backward replayed from that state or from the state the engine saved.
#   forward_state(sd, x, train, store=None)   (state, logits); store=dt rounds what the engine keeps in 16 bits (z, y, the packed weights)
#   state_from_ctx(engine, ctx)               Discriminator3DEngine's ctx ([N*D,H,W,C] buffers) -> the same plain state
#   replay(state, dl, need_dx, store=None)    ({state-dict name: gradient}, dx or None, {cancelled bias: sum |dy|})
#   replays / hold                            what backward_replay.compare3d needs, and the comparison
# BatchNorm3d backward: dy = scale * (gh - c1 - xh * c2), c1 = s1 / M, c2 = s2 / M with M = N*D*H*W (both zero for running
# statistics); InstanceNorm3d: per (sample, channel) over the WHOLE volume, dy = invstd * (g - mean(g) - xh * mean(g * xh)); the bias of a
# conv in front of it cancels (the engine returns exact zeros).  leaky'(0) = 0.2 (exact_reference.act_bwd64).
import math  # noqa: E402

from torch.nn import grad as G  # noqa: E402

from tests.backward_replay import BN_EPS, FLOOR32, SIGN_MARGIN, compare3d, d64, ncdhw  # noqa: E402,F401
from tests.exact_reference import act_bwd64  # noqa: E402
from tests.instnorm_reference import IN_EPS  # noqa: E402
from tests.pix2pix_backward_replay import _d_u, _forced, _rounders, flat  # noqa: E402

SP = (2, 3, 4)
FWD_NET_MUTANTS = ("kz_ky_exchanged", "depth_pad_missing", "depth_pad_far_side_only", "depth_pad_front_only", "depth_stride_1",
                   "in_stats_per_slice")
BWD_NET_MUTANTS = ("dgrad_depth_unflipped", "dgrad_depth_classes", "bn_count_without_d", "drop_c2", "first_bias_border")
_FIRST = {"kz_ky_exchanged": fwd_kz_ky_exchanged, "depth_pad_missing": fwd_depth_pad_missing,
          "depth_pad_far_side_only": fwd_depth_pad_front_missing, "depth_pad_front_only": fwd_depth_pad_far_missing,
          "depth_stride_1": fwd_depth_stride_1}


def _cv(t):
    """[C] -> [1, C, 1, 1, 1]"""
    return t.view(1, -1, 1, 1, 1)


def _pv(t):
    """[N, C] -> [N, C, 1, 1, 1]"""
    return t[:, :, None, None, None]


def net_layout(sd):
    """(Sequential name, conv indices, k) from the keys: `model` (PatchGAN, k 4) or `net` (PixelDiscriminator, k 1)"""
    seq = "model" if any(k.startswith("model.") for k in sd) else "net"
    convs = sorted(int(k.split(".")[1]) for k in sd if k.endswith(".weight") and sd[k].dim() == 5)
    return seq, convs, sd[f"{seq}.{convs[0]}.weight"].shape[2]


def _norm_stats(rec, sd, yfull, train, r32, mutant):
    if rec["norm"] == "instance":
        y = rec["y"]
        if mutant == "in_stats_per_slice":                             # statistics per depth slice instead of per volume
            mean = y.mean((3, 4), keepdim=True).expand_as(y)
            var = y.var((3, 4), unbiased=False, keepdim=True).expand_as(y)
            rec["mean_full"], rec["invstd_full"] = mean, torch.rsqrt(var + IN_EPS)
            mean, var = y.mean(SP), y.var(SP, unbiased=False)
        else:
            mean, var = y.mean(SP), y.var(SP, unbiased=False)
        rec["mean"], rec["invstd"] = r32(mean), r32(torch.rsqrt(var + IN_EPS))
        return
    bn = rec["bnname"]
    if train:                                                          # from the unrounded conv output, as the conv epilogue takes them
        mean, var = yfull.mean((0,) + SP), yfull.var((0,) + SP, unbiased=False)
    else:
        mean, var = sd[bn + ".running_mean"], sd[bn + ".running_var"]
    invstd = torch.rsqrt(var + BN_EPS)
    scale = sd[bn + ".weight"] * invstd
    rec.update(scale=r32(scale), shift=r32(sd[bn + ".bias"] - mean * scale), mean=r32(mean), invstd=r32(invstd))


def _normed(rec):
    y = rec["y"]
    if rec["norm"] == "instance":
        if "mean_full" in rec:
            return (y - rec["mean_full"]) * rec["invstd_full"]
        return (y - _pv(rec["mean"])) * _pv(rec["invstd"])
    return y * _cv(rec["scale"]) + _cv(rec["shift"])


def forward_state(sd, x, train, store=None, mutant=None):
    """the 3-D NLayerDiscriminator / PixelDiscriminator forward on the CPU -> (plain state, logits [N,1,OD,OH,OW]).  The forward mutants
    sit in the first layer (depth taps, pad, stride) and in the InstanceNorm statistics."""
    assert mutant is None or mutant in FWD_NET_MUTANTS
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    x = x.double()
    r16, r32 = _rounders(store)
    seq, convs, k = net_layout(sd)
    p, s0 = (1, 2) if k == 4 else (0, 1)
    nmid = len(convs) - 2
    inst = f"{seq}.{convs[1] + 1}.weight" not in sd
    n0 = f"{seq}.{convs[0]}"
    w, b = sd[n0 + ".weight"], sd[n0 + ".bias"]
    first = _FIRST.get(mutant, fwd_right)
    z = r16(F.leaky_relu(first(x, w, b, k, s0, p), 0.2))
    recs = [dict(kind="first", name=n0, k=k, s=s0, p=p, w=w, b=b, x=x, z=z)]
    cur = z
    for n, i in enumerate(convs[1:-1], 1):
        s = (2 if n < nmid else 1) if k == 4 else 1
        name = f"{seq}.{i}"
        w, b = sd[name + ".weight"], sd.get(name + ".bias")
        yfull = F.conv3d(cur, r16(w), b if store is None else None, stride=s, padding=p)      # the engine does not add a cancelled bias
        if inst and yfull[0, 0].numel() < 2:
            raise ValueError(f"Expected more than 1 spatial element when training, got input size {list(yfull.shape)}")
        rec = dict(kind="mid", name=name, k=k, s=s, p=p, w=w, b=b, inp=cur, y=r16(yfull), wd=r16(w), bnname=f"{seq}.{i + 1}",
                   norm="instance" if inst else "batch", train_stats=bool(train) or inst)
        _norm_stats(rec, sd, yfull, train, r32, mutant)
        recs.append(rec)
        cur = r16(F.leaky_relu(_normed(rec), 0.2))
    nl = f"{seq}.{convs[-1]}"
    w, b = sd[nl + ".weight"], sd.get(nl + ".bias")
    recs.append(dict(kind="last", name=nl, k=k, s=1, p=p, w=w, b=b, inp=cur))
    return dict(kind="pix2pix3d_d", N=x.shape[0], recs=recs), F.conv3d(cur, w, b, stride=1, padding=p)


def state_from_ctx(engine, ctx):
    """The saved forward of Discriminator3DEngine.forward as a plain state: [N*D,H,W,C] buffers become NCDHW fp64."""
    dt, N = engine.tdt, ctx["N"]
    recs = []
    for r in ctx["recs"]:
        conv = r["conv"]
        w = d64(conv.weight)
        rec = dict(kind=r["kind"], name=r["name"], k=r["k"], s=r["s"], p=r["p"], w=w, b=None if conv.bias is None else d64(conv.bias))
        if r["kind"] == "first":
            rec.update(x=d64(r["x"]), z=ncdhw(r["z"], N))          # z = leaky(conv + bias): its sign alone gives the activation gradient
        elif r["kind"] == "mid":
            rec.update(inp=ncdhw(r["inp"], N), y=ncdhw(r["y"], N), wd=w.to(dt).double(), bnname=r["bnname"], train_stats=bool(r["stats"]))
            if r.get("inorm") is not None:
                rec.update(norm="instance", mean=d64(r["inorm"][0]), invstd=d64(r["inorm"][1]))
            else:
                c = r["coef"]
                rec.update(norm="batch", scale=d64(c[0]), shift=d64(c[1]), mean=d64(c[2]), invstd=d64(c[3]))
        else:
            rec.update(inp=ncdhw(r["inp"], N))
        recs.append(rec)
    return dict(kind="pix2pix3d_d", N=N, recs=recs)


def _dgrad(shape, w, dy, s, p, mutant):
    if mutant == "dgrad_depth_unflipped":
        w = w.flip(2)
    elif mutant == "dgrad_depth_classes" and s == 2:
        w = w[:, :, [1, 0, 3, 2]]
    return G.conv3d_input(shape, w, dy, stride=s, padding=p)


def replay(state, dlogits, need_dx, store=None, S=None, mutant=None, force=None):
    """Discriminator3DEngine.backward in fp64 -> ({state-dict name: gradient}, dx or None, {cancelled bias name: sum |dy|})"""
    assert mutant is None or mutant in BWD_NET_MUTANTS
    dl = dlogits.double()
    S = float(2 ** round(math.log2(max(dl.numel(), 1)))) if S is None else S
    rnd = (lambda t: t) if store is None else (lambda t: (t * S).to(store).double() / S)
    recs = state["recs"]
    grads, bias_scale = {}, {}
    last = recs[-1]
    grads[last["name"] + ".weight"] = G.conv3d_weight(last["inp"], last["w"].shape, dl, stride=1, padding=last["p"])
    if last["b"] is not None:
        grads[last["name"] + ".bias"] = dl.sum((0,) + SP)
    dz = rnd(G.conv3d_input(last["inp"].shape, last["w"], dl, stride=1, padding=last["p"]))              # fp32 weights
    for i in range(len(recs) - 2, 0, -1):
        rec = recs[i]
        y = rec["y"]
        if rec["norm"] == "instance":
            xh = (y - _pv(rec["mean"])) * _pv(rec["invstd"])
            g = act_bwd64(dz, _forced(xh, force, ("mid", i)), "leaky")
            dy = _pv(rec["invstd"]) * (g - _pv(g.mean(SP)) - xh * _pv((g * xh).mean(SP)))
        else:
            xh = (y - _cv(rec["mean"])) * _cv(rec["invstd"])
            gh = act_bwd64(dz, _forced(y * _cv(rec["scale"]) + _cv(rec["shift"]), force, ("mid", i)), "leaky")
            s1, s2 = gh.sum((0,) + SP), (gh * xh).sum((0,) + SP)
            grads[rec["bnname"] + ".weight"], grads[rec["bnname"] + ".bias"] = s2, s1
            M = y.numel() // y.shape[1]
            if mutant == "bn_count_without_d":
                M //= y.shape[2]
            c1, c2 = (s1 / M, s2 / M) if rec["train_stats"] else (torch.zeros_like(s1), torch.zeros_like(s2))
            if mutant == "drop_c2":
                c2 = torch.zeros_like(c2)
            dy = _cv(rec["scale"]) * (gh - _cv(c1) - xh * _cv(c2))
        dy = rnd(dy)
        grads[rec["name"] + ".weight"] = G.conv3d_weight(rec["inp"], rec["w"].shape, dy, stride=rec["s"], padding=rec["p"])
        if rec["b"] is not None:
            grads[rec["name"] + ".bias"] = dy.sum((0,) + SP)
            bias_scale[rec["name"] + ".bias"] = float(dy.abs().sum())
        dz = rnd(_dgrad(rec["inp"].shape, rec["wd"], dy, rec["s"], rec["p"], mutant))
    first = recs[0]
    dy = rnd(act_bwd64(dz, first["z"], "leaky"))
    grads[first["name"] + ".weight"] = G.conv3d_weight(first["x"], first["w"].shape, dy, stride=first["s"], padding=first["p"])
    if first["b"] is not None:
        grads[first["name"] + ".bias"] = (dy[:, :, :-1, :-1, :-1] if mutant == "first_bias_border" else dy).sum((0,) + SP)
    dx = _dgrad(first["x"].shape, first["w"], dy, first["s"], first["p"], mutant) if need_dx else None
    return grads, dx, bias_scale


def undecided(state):
    """{("mid", i): mask} of the elements whose activation sign fp32 cannot decide (SIGN_MARGIN), and their count"""
    masks, n = {}, 0
    for i, rec in enumerate(state["recs"]):
        if rec["kind"] != "mid":
            continue
        y = rec["y"]
        if rec["norm"] == "instance":
            a, b = y, -_pv(rec["mean"])
        else:
            a, b = y * _cv(rec["scale"]), _cv(rec["shift"])
        m = (a + b).abs() < SIGN_MARGIN * (a.abs() + b.abs())
        if bool(m.any()):
            masks[("mid", i)] = m
            n += int(m.sum())
    return masks, n


def replays(state, dl, need_dx, store, S=None):
    """(R64, R16, d_U per tensor, count of undecided elements, bias_scale): what compare3d() needs"""
    def run(st, force=None):
        res = replay(state, dl, need_dx, st, S, force=force)
        return flat(res[:2]), res[2]
    r64, bias_scale = run(None)
    r16, _ = run(store)
    masks, n_und = undecided(state)
    d_u = {k: 0.0 for k in r64}
    if n_und:
        d_u = _d_u(r64, run(None, (masks, True))[0], run(None, (masks, False))[0])
    return r64, r16, d_u, n_und, bias_scale


def hold(got, rp, dt):
    """the project's bound on a result: every gradient and dx err <= 4 max(e16, FLOOR32 / 4) + d_U per tensor and per row
    (backward_replay.compare), a cancelled bias in absolute terms (compare3d) -> (report, failures)"""
    r64, r16, d_u, _, bias_scale = rp
    return compare3d(got, r64, r16, d_u, bias_scale, dt)


def summary_failures(s_got, s_ref, n, e16_full):
    """A gradient summary (golden_util.grad_summary: [sum, L2 norm, sampled elements ...] of a tensor of n elements) against the STORED
    summary of the reference, component by component, in units of the stored norm |g|.  If the full tensor holds the project's bound,
    |got - g|_2 <= B |g|_2 with B = 4 max(e16_full, FLOOR32) (e16_full: the 16-bit statement's own full-tensor error), then
        | |got| - |g| |                  <= B |g|            (triangle inequality)
        |samples(got) - samples(g)|_2    <= B |g|            (a subset of the elements)
        |sum(got) - sum(g)|              <= B |g| sqrt(n)    (Cauchy-Schwarz; attained when the error is the same in every element, which
                                                              an error in a norm's mean term comes close to within a channel)
    so these three are the summary's bound; no tighter one holds for the sum in general.  Returns the names of the components that
    miss it, with the three errors in units of their bounds."""
    import numpy as np
    B = 4 * max(e16_full, FLOOR32)
    nrm = float(s_ref[1])
    shares = {"sum": abs(s_got[0] - s_ref[0]) / (B * nrm * n ** 0.5), "norm": abs(s_got[1] - s_ref[1]) / (B * nrm),
              "samples": float(np.linalg.norm(s_got[2:] - s_ref[2:])) / (B * nrm)}
    return [c for c, v in shares.items() if not v <= 1.0], shares


# ---- the cases of tests/test_disc3d_networks_gpu.py, shared with the CPU test, which proves on these very seeds and shapes that the
# bounds tell the stated wrong implementations from a right one.  (kind, cin, ndf, n_layers, norm, N, (D, H, W), train, dtype, need_dx).
# Non-cubic volumes, so that an exchanged axis shows; 24 is the smallest side three stride-2 layers and two k4 / s1 layers leave a voxel from.
# The seed: the first from 21 on at which no activation sign of any case is undecided in fp32 (d_U = 0 in every bound; 21 has one such
# element, in d2_bn_train); tests/test_disc3d_reference_cpu.py asserts it.
NET_SEED = 22
NET_CASES = {
    "d2_bn_train": ("patch", 2, 64, 3, "batch", 2, (24, 32, 40), True, "f16", True),
    "d2_bn_eval": ("patch", 2, 64, 3, "batch", 2, (24, 32, 40), False, "f16", True),
    "d2_in_bf16": ("patch", 2, 16, 2, "instance", 1, (12, 16, 20), True, "bf16", True),
    "d6_in_nodx": ("patch", 6, 8, 3, "instance", 2, (24, 24, 32), True, "f16", False),
    "d1_bn_1layer": ("patch", 1, 64, 1, "batch", 2, (6, 8, 10), True, "f16", True),
    "p2_bn_train": ("pixel", 2, 64, None, "batch", 2, (3, 4, 5), True, "f16", True),
    "p2_bn_eval": ("pixel", 2, 64, None, "batch", 2, (3, 4, 5), False, "bf16", True),
    "p4_in": ("pixel", 4, 16, None, "instance", 2, (3, 4, 5), True, "f16", True),
}


def net_case(cid):
    """(state dict, input volume) of a network case"""
    from golden_util_disc3d import INPUT_STD, perturbed_running, state_dict_of
    kind, cin, ndf, nl, norm, N, vol, train, dtn, need_dx = NET_CASES[cid]
    sd = state_dict_of(kind, NET_SEED, cin, ndf, nl, norm)
    if not train:
        sd = perturbed_running(sd, NET_SEED + 2)
    x = INPUT_STD * torch.randn((N, cin) + tuple(vol), generator=torch.Generator().manual_seed(NET_SEED))
    return sd, x


def torch_module(kind, cin, ndf, n_layers, norm):
    """the module tree of the reference's 3-D discriminators in plain torch (for autograd in double and the key sets)"""
    import torch.nn as nn
    inst = norm == "instance"

    def nl(c):
        return nn.InstanceNorm3d(c, affine=False, track_running_stats=False) if inst else nn.BatchNorm3d(c)
    if kind == "pixel":
        net = nn.Module()
        net.net = nn.Sequential(nn.Conv3d(cin, ndf, 1), nn.LeakyReLU(0.2, True), nn.Conv3d(ndf, 2 * ndf, 1, bias=inst), nl(2 * ndf),
                                nn.LeakyReLU(0.2, True), nn.Conv3d(2 * ndf, 1, 1, bias=inst))
        net.forward = lambda x: net.net(x)
        return net
    seq = [nn.Conv3d(cin, ndf, 4, 2, 1), nn.LeakyReLU(0.2, True)]
    mult = [min(2 ** n, 8) for n in range(n_layers + 1)]
    for n in range(1, n_layers + 1):
        seq += [nn.Conv3d(ndf * mult[n - 1], ndf * mult[n], 4, 2 if n < n_layers else 1, 1, bias=inst), nl(ndf * mult[n]),
                nn.LeakyReLU(0.2, True)]
    seq += [nn.Conv3d(ndf * mult[n_layers], 1, 4, 1, 1)]
    net = nn.Module()
    net.model = nn.Sequential(*seq)
    net.forward = lambda x: net.model(x)
    return net
