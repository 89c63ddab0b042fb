"""Case lists and exact references for the image-side conv of 5..16 channels (csrc/ends_img.hip: gs_conv_imgwide_fwd / _wgrad /
_dgrad), on tests/exact_reference.py's construction: integer operands whose fp32 sums are exact in any order, so the kernels have
to give the one correctly rounded value.  Shared by tests/test_disc_wide_kernels_gpu.py (kernel against reference, zero tolerance)
and tests/test_disc_wide_reference_cpu.py (every case meets its conditions; the stated wrong implementations do not pass)."""
import functools

import torch
import torch.nn.functional as F

from tests import exact_reference as er

GEOM = {4: (2, 1), 1: (1, 0)}                       # k -> (stride, pad): the two geometries of the kernels
GSCALE = 0.25                                       # the loss-scale factor of the gradient cases (a power of two, != 1)

# (Cin, Cout, k, N, H, W).  Cin: one forward chunk of 4 + 1 (5), + 2, + 3, two full chunks = one weight-gradient chunk (8), + 1 (9),
# a ragged second weight-gradient chunk (11), the most (16).  Cout: every tile count 1..4, with and without a ragged last tile.
# Images: 2 x 2 (a 1 x 1 output: every tap but the centre 2 x 2 in the pad), 5 x 7 and 19 x 23 (odd: the bottom / right pad is
# reached, the last input row / column is read by no tap), 38 x 134 (output 19 x 67: more than one 8 x 32 forward patch and more
# than one 4 x 32 weight-gradient patch both ways, a multiple of neither), 9 x 5762 (273 weight-gradient patches: more than the
# 256 blocks, so blocks walk several patches).  N = 3 everywhere but the one-block case.
CASES = [
    (5, 8, 4, 3, 2, 2), (6, 64, 4, 3, 5, 7), (7, 24, 4, 3, 19, 23), (8, 32, 4, 3, 19, 23), (9, 96, 4, 3, 5, 7),
    (11, 128, 4, 3, 38, 134), (16, 128, 4, 3, 19, 23), (6, 64, 4, 3, 38, 134), (5, 8, 4, 3, 9, 5762), (16, 64, 4, 1, 2, 2),
    (5, 64, 1, 3, 1, 1), (6, 32, 1, 3, 5, 7), (7, 128, 1, 3, 19, 67), (9, 24, 1, 3, 5, 7), (11, 96, 1, 3, 19, 67),
    (16, 8, 1, 3, 5, 7), (8, 64, 1, 3, 40, 700),
]


def case_id(c):
    return "cin%d_cout%d_k%d_n%d_%dx%d" % c


def out_hw(c):
    Cin, Cout, k, N, H, W = c
    s, p = GEOM[k]
    return er.out_size(H, k, s, p), er.out_size(W, k, s, p)


def conv_fn(k):
    s, p = GEOM[k]
    return lambda x, w: F.conv2d(x, w, None, stride=s, padding=p)


@functools.lru_cache(maxsize=None)
def build(c, vset="S"):
    """operands x, w, b, dy and the fp64 references y, dx, dw of a case (computed once, shared by the tests; treat as read-only)"""
    Cin, Cout, k, N, H, W = c
    OH, OW = out_hw(c)
    # products per element: y k*k*Cin; dx at most k*k*Cout (bounded from above); dw one per output pixel
    return er.conv_case(("imgwide",) + tuple(c), vset, (N, Cin, H, W), (Cout, Cin, k, k), conv_fn(k), k * k * Cin, k * k * Cout,
                        N * OH * OW, bias=True)


# ---- the wrong implementations the tests must tell from the right one (each a function (x, w, b) -> y or (dy, ...) -> gradient)
def fwd_right(x, w, b, k):
    s, p = GEOM[k]
    return F.conv2d(x, w, b, stride=s, padding=p)


def fwd_taps_exchanged(x, w, b, k):
    """ky / kx exchanged in the first layer"""
    return fwd_right(x, w.transpose(2, 3), b, k)


def fwd_pad_bottom_right(x, w, b, k):
    """pad taken at the bottom / right instead of the top / left (k4 / s2 / p1: two zero rows after the image, none before)"""
    s, p = GEOM[k]
    if p == 0:
        return fwd_right(x, w, b, k)
    xp = F.pad(x, (0, 2 * p, 0, 2 * p))
    return F.conv2d(xp, w, b, stride=s, padding=0)


def fwd_channels_reversed(x, w, b, k):
    """image channels in reverse order"""
    return fwd_right(x.flip(1), w, b, k)


def fwd_halves_exchanged(x, w, b, k):
    """the concat halves exchanged"""
    h = x.shape[1] // 2
    return fwd_right(torch.cat((x[:, h:], x[:, :h]), 1), w, b, k)


def fwd_bias_dropped(x, w, b, k):
    return fwd_right(x, w, None, k)


FWD_MUTANTS = {"ky/kx exchanged": fwd_taps_exchanged, "pad at the bottom/right": fwd_pad_bottom_right,
               "channels reversed": fwd_channels_reversed, "concat halves exchanged": fwd_halves_exchanged,
               "bias dropped": fwd_bias_dropped}


def db_right(dy):
    return dy.sum((0, 2, 3))


def db_without_border(dy):
    """bias gradient summed without the border pixels"""
    if dy.shape[2] < 3 or dy.shape[3] < 3:
        return dy.sum((0, 2, 3)) * 0
    return dy[:, :, 1:-1, 1:-1].sum((0, 2, 3))


def dgrad_right(dy, w, x_shape, k):
    s, p = GEOM[k]
    return torch.nn.grad.conv2d_input(x_shape, w, dy, stride=s, padding=p)


def dgrad_classes_exchanged(dy, w, x_shape, k):
    """data gradient with the sub-pixel classes exchanged: the row-parity classes use each other's taps"""
    s, p = GEOM[k]
    if s == 1:
        return dgrad_right(dy, w, x_shape, k)
    w2 = w[:, :, [1, 0, 3, 2], :]
    return torch.nn.grad.conv2d_input(x_shape, w2, dy, stride=s, padding=p)


# ================================================================================================ network cases
# Shared by tests/test_disc_wide_networks_gpu.py and tests/test_disc_wide_reference_cpu.py (which proves on these very seeds and
# shapes that the bounds tell the stated wrong implementations from a right one).
# PatchGAN cases: (input_nc, ndf, n_layers, norm, N, H, W, train, dtype, need_dx)
D_CASES = {
    "d6_bn_train": (6, 64, 3, "batch", 2, 32, 32, True, "f16", True),
    "d6_bn_eval": (6, 64, 3, "batch", 2, 32, 32, False, "f16", True),
    "d6_bn_bf16_nodx": (6, 64, 3, "batch", 2, 32, 32, True, "bf16", False),
    "d5_in_34x70": (5, 32, 2, "instance", 3, 34, 70, True, "f16", True),
    "d8_1layer_19x23": (8, 64, 1, "batch", 1, 19, 23, True, "f16", True),
    "d16_ndf128": (16, 128, 2, "batch", 2, 16, 48, True, "f16", True),
    "d11_ndf96": (11, 96, 2, "batch", 2, 18, 18, True, "f16", False),
}
# PixelDiscriminator cases: (input_nc, ndf, norm, N, H, W, train, dtype, need_dx)
P_CASES = {
    "p2_bn_train": (2, 64, "batch", 2, 8, 8, True, "f16", True),
    "p2_bn_eval": (2, 64, "batch", 2, 8, 8, False, "f16", True),
    "p6_in_5x7": (6, 32, "instance", 3, 5, 7, True, "f16", True),
    "p6_in_bf16_nodx": (6, 32, "instance", 3, 5, 7, True, "bf16", False),
}
SEED = 11


def patchgan_case(cid):
    """(state dict, input) of a PatchGAN case"""
    from golden_util import seeded_discriminator_state_dict
    from golden_util_instance import seeded_discriminator_state_dict_instance
    from tests import pix2pix_backward_replay as pr
    cin, ndf, nl, norm, N, H, W, train, dtn, need_dx = D_CASES[cid]
    if norm == "instance":
        sd = seeded_discriminator_state_dict_instance(SEED, cin, ndf, nl)
    else:
        sd = seeded_discriminator_state_dict(SEED, cin, ndf, nl, bias_std=0.05)
        if not train:
            pr.perturb_running(sd, SEED + 2)
    x = 0.5 * torch.randn((N, cin, H, W), generator=torch.Generator().manual_seed(SEED))
    return sd, x


def patchgan_forwards(cid, sd, x, store=None):
    """(plain state, logits) of the fp64 statement; store=dt rounds what the engine keeps in 16 bits"""
    from tests import instnorm_reference as ir
    from tests import pix2pix_backward_replay as pr
    cin, ndf, nl, norm, N, H, W, train, dtn, need_dx = D_CASES[cid]
    if norm == "instance":
        return ir.discriminator_forward_state(sd, x, store=store)
    return pr.discriminator_forward_state(sd, x, train, store=store)
