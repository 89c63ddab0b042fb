"""Whole-network execution plan of the U-Net on the HIP kernels (forward + backward).

Reference call sites: unet/unet_model.py:26-37 (forward), unet/unet_parts.py (blocks).  One
torch.autograd.Function spans the network so that the plan is free to keep activations in 16-bit NHWC,
to write the encoder outputs straight into the skip half of the decoder's concat buffers (torch.cat
becomes free), to fuse the 2x2 max-pool into the BatchNorm+ReLU pass, and to run gradients through the
same buffers in reverse.  Parameters stay ordinary fp32 nn.Parameters in the reference layouts.

Data layout in HBM (per level i = 0..4, C_i = 64*2^i, h_i = H >> i):
  y   raw conv output            [N, h, w, C]   16-bit   (kept for BatchNorm/ReLU backward)
  z   relu(bn(y))                [N, h, w, C]   16-bit   (conv input of the next layer; kept for wgrad)
  cat concat buffer of level i   [N, h_i, w_i, 2*C_i]:  channels [0,C_i) = skip (encoder z),
                                                        channels [C_i,2C_i) = ConvTranspose2d output
Gradients use the same layouts; they are carried multiplied by a power-of-two loss scale S ~ N*H*W so
that fp16 storage never underflows (gradients are O(1) after scaling thanks to BatchNorm); every
parameter gradient is multiplied by 1/S on its way out (exact).
"""
from __future__ import annotations

import functools
import math
import os
import warnings
from typing import Callable, Dict, List, Optional

import torch

from .. import ops
from .._lib import ACT_NONE, ACT_RELU
from ..engine_common import ParamIndex, _flush_nbt, bn_coeffs, compute_dtype, pack_key, pack_reuse_allowed

# eval-mode forward without a graph: fold BatchNorm into the conv weights (GSSEG_FOLD_BN=0 keeps the two-pass form)
FOLD_BN_INFERENCE = os.environ.get("GSSEG_FOLD_BN", "1") != "0"
# Weight gradients of levels 1-4 and of the transposed convolutions on a second HIP stream, launched BEHIND their stage's
# data gradient so that they run beside the BatchNorm backward of the next stage.  Concurrent kernels
# stretch each other's event-bracketed durations, so per-kernel roofline figures are taken with GSSEG_WGRAD_STREAM=0, which
# keeps everything on one stream.  A stream that is being captured always gets the one-stream form.
WGRAD_SIDE_STREAM = os.environ.get("GSSEG_WGRAD_STREAM", "1") != "0"
# ConvTranspose2d bias gradients out of the epilogue sums of the data-gradient convolution that writes d(concat), instead of
# a column-sum pass over that tensor (un-padded case; GSSEG_UP_BIAS_FUSED=0 restores the pass).
# Stem backward (one input channel, image without gradient): BatchNorm backward apply + weight gradient in one pass
# (GSSEG_STEM_BWD_FUSED=0 restores bn_act_bwd_apply + conv_smallcin_wgrad).
FUSED_STEM_BWD = os.environ.get("GSSEG_STEM_BWD_FUSED", "1") != "0"
# Head backward: the data gradient of the 1x1 head is formed inside the BatchNorm backward of the last stage.
# Stem forward without its convolution output in memory (statistics from the image, conv + BatchNorm + ReLU in one pass).
FUSED_STEM_FWD = os.environ.get("GSSEG_STEM_FWD_FUSED", "1") != "0"
FUSED_HEAD_FWD = os.environ.get("GSSEG_HEAD_FWD_FUSED", "1") != "0"
FUSED_HEAD_BWD = os.environ.get("GSSEG_HEAD_BWD_FUSED", "1") != "0"
FUSED_UP_BIAS_GRAD = os.environ.get("GSSEG_UP_BIAS_FUSED", "1") != "0"


class _ConvRec:
    """Saved state of one conv -> BN -> ReLU stage."""
    __slots__ = ("name", "wkey", "bnkey", "inp", "inp_is_image", "y", "coef", "geom", "cin", "cout", "h", "w",
                 "wd", "train_stats", "inp_stride", "z", "tap_sums", "wide")


class _UpRec:
    __slots__ = ("name", "zin", "cat", "geom_bwd", "geom_wg", "wd", "cin", "cout", "h", "w", "H2", "W2", "pt", "pl")


STREAM_SMALL_CONV = os.environ.get("GSSEG_STREAM_CONV", "1") != "0"


@functools.lru_cache(maxsize=4096)
def stream_conv(N, h, w, cin, cout):
    """A 3x3 conv with so few output pixels that the halo kernels would start <= 128 workgroups on 256 CUs (the deep levels at small
    batch: 2 x 32 x 32 pixels x 512 channels = 64 items with 32-stage K loops, 39-69 us each) runs on the weight-streaming igemm form
    instead (csrc/skinny.hip: K split over one block per CU).  cin / cout: the GEMM's K channels and columns (swapped for a data
    gradient).  The C side has the last word (GSSEG_SKINNY, shape limits): gs_conv_igemm_mtiles tells which form takes it."""
    M = N * h * w
    if not STREAM_SMALL_CONV or M > 8192 or cin % 64 or cout % 32:
        return False
    tiles = (-(-w // 32)) * (-(-h // 8)) if w >= 24 else (-(-w // 16)) * (-(-h // 16))
    if N * tiles * (-(-cout // 64)) > 128:
        return False
    return ops.conv_igemm_mtiles(ops.geom_conv(N, h, w, cin, cout, 3, 1, 1)) == -(-M // 16)


STEM_WKEY = "inc.double_conv.0.weight"                      # the image-end conv: told apart by name, its Cin may be a multiple of 8
STAGES = (["inc.0", "inc.3"] + [f"down{i}.{k}" for i in range(1, 5) for k in (0, 3)] +
          [s_ for j in range(1, 5) for s_ in (f"up{j}.up", f"up{j}.conv.0", f"up{j}.conv.3")])
# MFMA segments of one stage of the pair forward: "1" = x_hi.w_hi, "x" = + x_lo.w_hi, "w" = + x_hi.w_lo, "xw" = all three
# "q" = x_hi.w_hi on the 16-bit MFMA + the two correction terms as ONE FP8 block-scaled segment (csrc/common.hpp): 2x the MFMA work of
# "1" instead of the 3x of "xw"; the lo plane of its input travels as a q plane.  Shapes outside the LDS-DMA kernel run it as "xw".
_SEG_MODES = ("1", "x", "w", "xw", "xw-", "q")
# The correction form of the "mixed" plan's MIXED_XW stages: "xw" (default: 16-bit correction segments) or "q" (GSSEG_MIXED_SEG=q).
# Round-4 experiment with a stated kill criterion (VERDICT r3 item 2 ii: keep "q" only if every fixture stays < 8.5e-4 AND the bs=32
# step gains >= 1 ms): fixtures 5.7e-4 .. 7.7e-4 (xw: 5.4e-4 .. 6.7e-4) -- met; step 14.98 -> 14.69 ms = -0.3 ms -- NOT met, so "q" is
# not the default.  The FP8 stage itself runs at 0.85x the time of a 16-bit stage (in-kernel stamps, profiles/r04_q8_phase.txt) and
# the 4-wave form reaches the ideal q/xw = 0.67, but the 8-wave kernel that the large layers need has no registers left for it:
# 66 VGPRs + 59 SGPRs spilled, its epilogue takes 1.8x as long.
MIXED_SEG = os.environ.get("GSSEG_MIXED_SEG", "xw")
# Where the 16-bit error of the logits is made (tools/parity_attribution.py, profiles/r03_parity_attribution_wyz.json): the
# 256^2 / 128^2 / 64^2 stages of the encoder and the last two decoder levels; everything at 32^2 and below contributes
# < 5e-5 each.  "mixed" keeps all three MFMA segments there and one segment elsewhere -- every tensor still travels as a
# hi/lo pair (the deep levels hold few bytes), so only the MFMA work is saved: 48 of the 92 GFLOP per image run three
# segments.  fp16 only: bf16 pairs carry 16 significand bits, which every stage needs.
MIXED_XW = ("inc.3", "down1.0", "down1.3", "down2.0", "down2.3", "up3.conv.0", "up3.conv.3", "up4.conv.0", "up4.conv.3")


def resolve_plan(precise, dtype: str, bilinear: bool = False):
    """precise: False / None -> None (default engine); True -> every stage "xw"; "mixed" / "auto" -> MIXED_XW (bf16 and the
    bilinear=True net: every stage); a dict {stage: mode} -> that plan (missing stages "1").
    bilinear=True (unet_parts.py:49-50: half the decoder channels, four interpolations): every conv stage contributes 5e-4 ..
    5e-3 on its own when run on 16-bit inputs (tools/parity_fp8_sim.py --bilinear; the nine MIXED_XW stages alone leave 1.9e-3
    measured / 2.5e-3 simulated), so "mixed" keeps the correction segments on all of them: 2e-5 measured."""
    if precise is None or precise is False or precise == 0 or precise == "0" or precise == "":
        return None
    if precise is True or precise == 1 or precise == "1" or precise == "full":
        return {s_: "xw" for s_ in STAGES}
    if precise == "mixed" or precise == "auto":
        if dtype != "f16" or bilinear:
            return {s_: "xw" for s_ in STAGES}
        plan = {s_: (MIXED_SEG if s_ in MIXED_XW else "1") for s_ in STAGES}
        if MIXED_SEG == "xw" and os.environ.get("GSSEG_MIXED_UPW", "all") == "skip":
            # experiment: the decoder-entry convs run the w_lo segment on the skip half only ("xw-")
            plan["up3.conv.0"] = plan["up4.conv.0"] = "xw-"
        return plan
    if isinstance(precise, dict):
        bad = [k for k, v in precise.items() if k not in STAGES or v not in _SEG_MODES]
        if bad:
            raise ValueError(f"precise plan: unknown stages / modes {bad}")
        return {s_: precise.get(s_, "1") for s_ in STAGES}
    raise ValueError("precise must be False, True, 'mixed', 'auto' or a {stage: mode} dict")


def _segs(mode: str, cin: int, lo_len=None):
    """(segment list for pack_weight_segs, K extent, input wrap) of a stage reading a [hi | lo] pair of cin channels.  lo_len:
    only the first lo_len channels of the lo plane are valid (a concat buffer whose up half was written hi-only): the x_lo
    segment then covers those alone -- the input is read as [hi (cin) | lo (lo_len)] and wraps to the hi plane for w_lo."""
    ll = cin if lo_len is None else lo_len
    if mode == "1":
        return [(0, 0, cin)], cin, cin
    if mode == "x":
        return [(0, 0, cin), (0, 0, ll)], cin + ll, cin + ll
    if mode == "w":
        return [(0, 0, cin), (1, 0, cin)], 2 * cin, cin
    if mode == "xw-":                                      # w_lo only on the channels whose x_lo is valid: [hi (cin) | lo (ll)] then hi[0:ll)
        return [(0, 0, cin), (0, 0, ll), (1, 0, ll)], cin + 2 * ll, cin + ll
    return [(0, 0, cin), (0, 0, ll), (1, 0, cin)], 2 * cin + ll, cin + ll


def _stage_keys(st: str):
    """state-dict keys of plan stage `st`: (weight key, BatchNorm module key or None, transposed) -- "down2.3" ->
    ("down2.maxpool_conv.1.double_conv.3.weight", "down2.maxpool_conv.1.double_conv.4", False), "up1.up" -> ("up1.up.weight", None, True)"""
    if st.endswith(".up"):
        return st + ".weight", None, True
    blk, idx = st.rsplit(".", 1)
    prefix = blk if (blk == "inc" or blk.endswith(".conv")) else blk + ".maxpool_conv.1"
    return f"{prefix}.double_conv.{idx}.weight", f"{prefix}.double_conv.{int(idx) + 1}", False


class UNetEngine(ParamIndex):
    """Executes UNet.forward / backward for a `UNet` module tree on the HIP kernels."""

    def __init__(self, net, dtype: str = "f16", precise: bool = False):
        self.net = net
        self.dtype, self.tdt = compute_dtype(dtype)
        # precise forward (module docstring of forward_precise): activations / weights as hi+lo pairs of 16-bit values,
        # logits within ~1e-5 of the fp32 reference instead of ~4e-3; the backward pass is unchanged (it reads the hi halves)
        self.plan = resolve_plan(precise, self.dtype, bool(getattr(net, "bilinear", False)))      # None: the default single 16-bit engine
        self.precise = self.plan is not None
        # "auto" (what UNet() builds): the mixed pair forward wherever it is implemented, the 16-bit engine elsewhere (an
        # explicit "mixed" / True raises there instead)
        self.auto = precise == "auto"
        self._warned_fallback = False    # "auto" names its fallback to the 16-bit engine once per engine
        self.dynamic_loss_scale = os.environ.get("GSSEG_DYNAMIC_LOSS_SCALE", "0") == "1"
        self._packs: Dict[str, tuple] = {}
        self.trust_versions = False      # True: training forwards reuse version-keyed packs (GSSEG_PACK_CACHE, engine_common.py)
        self._side_streams: Dict[torch.device, torch.cuda.Stream] = {}     # weight-gradient stream per device
        # data-parallel hooks (parallel.GradReducer): grads are allocated inside the reducer's flat buckets,
        # announced as soon as they are final (so the RCCL all-reduce overlaps the rest of backward), and
        # `after_backward` makes the compute stream wait for the collectives.
        self.grad_ready_hook: Optional[Callable[[str, torch.Tensor], None]] = None
        self.last_backward_streams = 0     # streams the last backward() used: 2 = weight gradients on the side stream
        self.grad_alloc: Optional[Callable[[str, torch.Tensor], torch.Tensor]] = None
        self.after_backward: Optional[Callable[[], None]] = None
        self.grad_fetch: Optional[Callable[[str], torch.Tensor]] = None      # reduced gradient handed to autograd
        # True: a backward pass whose parameters already hold a gradient (the second backward of the Unet problem of
        # train_end2end_jsrt.py:176-226, which sums two passes of the net) adds its gradients to `.grad` with ONE foreach launch
        # and hands autograd nothing, instead of one 5-us AccumulateGrad add per parameter (~90); same sums, same order
        self.accumulate_grads = False

    # ------------------------------------------------------------------ parameters (ParamIndex: param_items, buffer_dict, submodule)
    def _side_stream(self, dev):
        st = self._side_streams.get(dev)
        if st is None:
            st = self._side_streams[dev] = torch.cuda.Stream(device=dev)
        return st

    def invalidate_packs(self):
        """Drop the cached 16-bit weight packs (they are otherwise reused until a Parameter changes)."""
        self._packs.clear()

    def _prepack(self, params: Dict[str, torch.Tensor], need_dgrad: bool, conv_fwd: bool = True):
        """Re-pack every stale 3x3 / k2-s2 conv weight of the network in ONE launch (after an optimiser step all of them are
        stale: 21 pack launches of 5-8 us each were launch-bound); _packed() below then finds them cached.  conv_fwd=False (the
        pair forward, whose 3x3 convs read SEGMENT packs): the 3x3 convs get their data-gradient pack only -- half the launch's
        bytes (a pack entry then holds None in the forward slot)."""
        items, fresh = [], []
        for name, w in params.items():
            if not name.endswith(".weight") or w.dim() != 4:
                continue
            transposed = name.endswith(".up.weight")
            if transposed:
                if tuple(w.shape[2:]) != (2, 2):
                    continue
                cin, cout = w.shape[0], w.shape[1]
            else:
                if tuple(w.shape[2:]) != (3, 3) or name == STEM_WKEY:         # the image-end layer is not packed (any channel count)
                    continue
                cout, cin = w.shape[0], w.shape[1]
            key = pack_key(w)
            ent = self._packs.get(name)
            want_f = conv_fwd or transposed
            if ent is not None and ent[0] == key and (ent[2] is not None or not need_dgrad) and (ent[1] is not None or not want_f):
                continue
            if not want_f and not need_dgrad:
                continue
            taps = w.shape[2] * w.shape[3]
            wf = torch.empty((taps, cout, cin), dtype=self.tdt, device=w.device) if want_f else None
            wd = torch.empty((taps, cin, cout), dtype=self.tdt, device=w.device) if need_dgrad else None
            items.append((w.detach(), wf, wd, transposed))
            fresh.append((name, key, wf, wd))
        if len(items) > 1:
            ops.pack_weight_multi(items)
            for name, key, wf, wd in fresh:
                self._packs[name] = (key, wf, wd)

    def _packed(self, name: str, w: torch.Tensor, transposed: bool, need_dgrad: bool, need_fwd: bool = True):
        """16-bit K-major packs of a conv weight, cached until the Parameter is modified (need_fwd=False: a cached entry without
        its forward pack -- _prepack(conv_fwd=False) -- will do)."""
        key = pack_key(w)
        ent = self._packs.get(name)
        if ent is not None and ent[0] == key and (ent[2] is not None or not need_dgrad) and (ent[1] is not None or not need_fwd):
            return ent[1], ent[2]
        if transposed:
            cin, cout = w.shape[0], w.shape[1]
        else:
            cout, cin = w.shape[0], w.shape[1]
        taps = w.shape[2] * w.shape[3]
        wf = torch.empty((taps, cout, cin), dtype=self.tdt, device=w.device)
        wd = torch.empty((taps, cin, cout), dtype=self.tdt, device=w.device) if need_dgrad else None
        ops.pack_weight(w.detach(), wf, wd, transposed)
        self._packs[name] = (key, wf, wd)
        return wf, wd

    def _packed_padded(self, name: str, w: torch.Tensor, cpad: int, need_dgrad: bool):
        """packs of a 3x3 conv weight whose input channels are zero-padded to cpad (an image of more than 4 channels enters
        the MFMA path as a 16-bit NHWC tensor with a multiple of 8 channels)"""
        key = (pack_key(w), cpad)
        ent = self._packs.get(name + "|padded")
        if ent is not None and ent[0] == key and (ent[2] is not None or not need_dgrad):
            return ent[1], ent[2]
        cout, cin = w.shape[0], w.shape[1]
        wp = torch.zeros((cout, cpad, 3, 3), dtype=torch.float32, device=w.device)
        wp[:, :cin] = w.detach()
        wf = torch.empty((9, cout, cpad), dtype=self.tdt, device=w.device)
        wd = torch.empty((9, cpad, cout), dtype=self.tdt, device=w.device) if need_dgrad else None
        ops.pack_weight(wp, wf, wd, False)
        self._packs[name + "|padded"] = (key, wf, wd)
        return wf, wd

    def _folded(self, wkey: str, bnkey: str, w, gamma, beta, rm, rv, eps: float, image: bool):
        """Inference: BatchNorm(eval) folded into the conv -- w' = w * gamma/sqrt(var+eps) per output channel and a bias
        beta - mean*gamma/sqrt(var+eps).  Cached until a Parameter or running statistic changes."""
        key = tuple(pack_key(t) for t in (w, gamma, beta, rm, rv)) + (eps,)
        ent = self._packs.get(wkey + "|folded")
        if ent is not None and ent[0] == key:
            return ent[1], ent[2]
        with torch.no_grad():
            s = gamma.detach().float() * torch.rsqrt(rv.float() + eps)
            w_eff = (w.detach().float() * s.view(-1, 1, 1, 1)).contiguous()
            bias = (beta.detach().float() - rm.float() * s).contiguous()
            if image:
                wf = w_eff                                   # the direct first-layer kernel reads fp32 [Cout,Cin,3,3]
            else:
                wf = torch.empty((9, w.shape[0], w.shape[1]), dtype=self.tdt, device=w.device)
                ops.pack_weight(w_eff, wf, None, False)
        self._packs[wkey + "|folded"] = (key, wf, bias)
        return wf, bias

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor, params: Dict[str, torch.Tensor], training: bool, need_grad: bool, labels: bool = False):
        """-> (fp32 NCHW logits, backward context).  labels (UNet.predict; no graph): -> (uint8 label map [N,H,W], None) -- from the
        pair head's label epilogue where the pair forward runs (no logits tensor), from this engine's logits elsewhere."""
        net = self.net
        if not x.is_cuda:
            raise RuntimeError("UNet (semantic_segmentation_amd) runs on the MI355X only: move the input and the "
                               "module to cuda; there is no CPU / ATen fallback")
        if x.dim() != 4 or x.shape[1] != net.n_channels:
            raise ValueError(f"expected input [N,{net.n_channels},H,W], got {tuple(x.shape)}")
        N, _, H, W = x.shape
        if H < 16 or W < 16:
            raise ValueError("input must be at least 16x16 (four 2x2 poolings)")
        if self.precise:
            # what the pair forward does not cover: the end kernels stop at 64 image channels / classes (gs_conv_widecin_fwd_split,
            # gs_head1x1_fwd_split); "auto" then runs the 16-bit engine, which takes any count, and says so once
            why = None
            if not ops.USE_HALO_CONV:
                why = "GSSEG_CONV3X3 is not 'halo' (the pair forward needs the halo-reuse conv kernel)"
            elif net.n_channels > 64 or net.n_classes > 64:
                why = f"the pair forward's end kernels take up to 64 image channels and classes (got {net.n_channels}, {net.n_classes})"
            if why is None:
                return self.forward_precise(x, params, training, need_grad, labels)
            if not self.auto:
                if ops.USE_HALO_CONV:
                    raise NotImplementedError("UNet pair forward: " + why)
                return self.forward_precise(x, params, training, need_grad, labels)      # (raises: no halo-reuse conv kernel)
            if not self._warned_fallback:
                self._warned_fallback = True
                warnings.warn(f"UNet(precise='auto'): {why} -- running the single 16-bit engine, whose logits are about 5e-3 from "
                              "the fp32 reference instead of 1e-3", RuntimeWarning, stacklevel=2)
        dev, tdt = x.device, self.tdt
        x = x.contiguous().float()
        bufs = self.buffer_dict()
        nbt_pending = []                 # num_batches_tracked counters of this pass: ONE foreach increment at the end
        hs = [H >> i for i in range(5)]
        ws_ = [W >> i for i in range(5)]
        bilinear = bool(net.bilinear)
        C = [64, 128, 256, 512, 1024 // (2 if bilinear else 1)]      # unet_model.py:18-19
        if not pack_reuse_allowed(need_grad, self.trust_versions):
            self._packs.clear()                                       # `.data` writes are invisible to the version keys
        if training or need_grad:
            self._prepack(params, need_grad)                          # every stale weight pack in one launch

        def empty(*shape, dtype=tdt):
            return torch.empty(shape, dtype=dtype, device=dev)

        partials = None      # BatchNorm partial-sum workspace, (re)allocated per conv from torch's cache

        recs: List[_ConvRec] = []
        ups: List[_UpRec] = []

        def conv_bn_relu(prefix, idx, inp, cin, cout, h, w, z, z_stride, z_coff, zp, image=False, wide=0):
            """prefix.double_conv.{idx} conv + .{idx+1} BN + ReLU.  wide = C0 > 4: `inp` is the image already converted to a
            16-bit NHWC tensor of cin = ceil8(C0) channels (zero padded); the weight's input channels are padded alike."""
            wkey, bnkey = f"{prefix}.double_conv.{idx}.weight", f"{prefix}.double_conv.{idx + 1}"
            wparam = params[wkey]
            rm = bufs.get(bnkey + ".running_mean")
            batch_stats = training or rm is None
            if FOLD_BN_INFERENCE and not batch_stats and not need_grad and ops.USE_HALO_CONV and not wide:
                # inference: one kernel per conv block (folded BN as bias, ReLU in the epilogue, written where the
                # consumer reads it); the 2x2 pool of the Down blocks is a read-only pass over the skip tensor
                wf, bias = self._folded(wkey, bnkey, wparam, params[bnkey + ".weight"], params[bnkey + ".bias"], rm,
                                        bufs[bnkey + ".running_var"], self.submodule(bnkey).eps, image)
                if image:
                    if z_stride != cout or z_coff != 0:
                        raise RuntimeError("first-layer output must be dense")
                    ops.conv_smallcin_fwd(inp, wf, bias, z, None, 3, 1, 1, act=ACT_RELU)
                else:
                    ops.conv3x3(inp, wf, z, N, h, w, cin, cout, ops.TAPS3_FWD, bias, None, act=ACT_RELU,
                                out_stride=z_stride, out_coff=z_coff)
                if zp is not None:
                    ops.maxpool2x2_fwd(z, zp, N, h, w, cout, z_stride=z_stride, z_coff=z_coff)
                return None
            rec = _ConvRec()
            rec.name, rec.wkey, rec.bnkey = f"{prefix}.{idx}", wkey, bnkey
            rec.cin, rec.cout, rec.h, rec.w, rec.inp_is_image = cin, cout, h, w, image
            rec.inp_stride = None
            rec.wide = wide
            nonlocal partials
            g = None if image else ops.geom_conv(N, h, w, cin, cout, 3, 1, 1)
            # (training-mode statistics only: in eval mode a sample's logits must not depend on which other samples share its
            # batch, bit for bit -- the K split of the streaming form follows the pixel count)
            streaming = (not image) and batch_stats and ops.USE_HALO_CONV and stream_conv(N, h, w, cin, cout)
            if image:
                ntiles = ops.conv_smallcin_mtiles(N, h, w)
            elif ops.USE_HALO_CONV and not streaming:
                ntiles = ops.conv3x3_stat_rows(N, h, w, cin, cout)
            else:
                ntiles = ops.conv_igemm_mtiles(g)
            partials = empty(ops.bn_partials_numel(ntiles, cout), dtype=torch.float32) if batch_stats else None
            if (image and FUSED_STEM_FWD and cin == 1 and cout == 64 and z is not None and zp is None and z_stride == cout
                    and z_coff == 0 and inp.is_contiguous()):
                # one-channel stem: the BatchNorm statistics come from the image and the weights alone, the convolution
                # output is normalised in registers and never stored (the backward re-forms it from the image)
                wst = wparam.detach().contiguous()
                # per-tile tap sums / Gram entries of the image: the backward's closed-form weight gradient needs their totals
                rec.tap_sums = None
                if need_grad:        # (eval-mode statistics: c1 = c2 = 0 multiply them, so they only have to be finite)
                    rec.tap_sums = empty(ntiles * 54, dtype=torch.float32) if batch_stats else torch.zeros(ntiles * 54, dtype=torch.float32, device=dev)
                if batch_stats:
                    ops.stem_stats(inp, wst, partials, rec.tap_sums)
                coef, rec.train_stats = bn_coeffs(self.submodule(bnkey), partials, ntiles, cout, N * h * w, training, dev, nbt_pending)
                ops.stem_fwd_bn(inp, wst, coef[0], coef[1], ACT_RELU, z)
                rec.geom, rec.wd = None, None
                rec.y, rec.coef, rec.z = None, coef, z
                if need_grad:
                    rec.inp = inp
                    recs.append(rec)
                return rec
            y = empty(N, h, w, cout)
            if image:
                ops.conv_smallcin_fwd(inp, wparam.detach().contiguous(), None, y, partials, 3, 1, 1)
                rec.geom, rec.wd = None, None
            else:
                wf, wd = (self._packed_padded(wkey, wparam, cin, need_grad) if wide
                          else self._packed(wkey, wparam, False, need_grad))
                if ops.USE_HALO_CONV and not streaming:
                    ops.conv3x3(inp, wf, y, N, h, w, cin, cout, ops.TAPS3_FWD, None, partials)
                else:
                    ops.conv_igemm(g, inp, wf, y, None, partials)
                rec.geom, rec.wd = g, wd
            coef, rec.train_stats = bn_coeffs(self.submodule(bnkey), partials, ntiles, cout, N * h * w, training, dev, nbt_pending)
            if z is not None:
                ops.bn_act_apply(y, coef[0], coef[1], ACT_RELU, z, z_stride, z_coff, zp)
            rec.y, rec.coef = y, coef               # (z is None: the caller applies BatchNorm + ReLU on its own load path)
            if need_grad:
                rec.inp = inp
                recs.append(rec)
            return rec

        # ---- encoder ----
        cats = [None] * 4
        for i in range(4):
            zero_needed = (hs[i] - 2 * hs[i + 1]) or (ws_[i] - 2 * ws_[i + 1])
            alloc = torch.zeros if zero_needed else torch.empty
            cats[i] = alloc((N, hs[i], ws_[i], 2 * C[i]), dtype=tdt, device=dev)
        inp = x
        cin = net.n_channels
        wide = 0
        if cin > 4:
            # more than four input channels (the reference takes any, unet_model.py:8-12): the image enters the MFMA path as a
            # 16-bit NHWC tensor zero-padded to a multiple of 8 channels (the direct first-layer kernels read 1..4 fp32 channels)
            if not ops.USE_HALO_CONV:
                raise NotImplementedError("n_channels above 4 needs the halo-reuse conv kernel")
            wide, cpad = cin, (cin + 7) // 8 * 8
            xin = (torch.zeros if cpad != cin else torch.empty)((N, H, W, cpad), dtype=tdt, device=dev)
            ops.nchw_to_nhwc(x, xin, dst_stride=cpad)
            inp, cin = xin, cpad
        pooled = None
        for i in range(5):
            prefix = "inc" if i == 0 else f"down{i}.maxpool_conv.1"
            h, w = hs[i], ws_[i]
            zmid = empty(N, h, w, C[i])
            conv_bn_relu(prefix, 0, inp, cin, C[i], h, w, zmid, C[i], 0, None, image=(i == 0 and not wide),
                         wide=wide if i == 0 else 0)
            if i < 4:
                pooled = empty(N, hs[i + 1], ws_[i + 1], C[i])
                conv_bn_relu(prefix, 3, zmid, C[i], C[i], h, w, cats[i], 2 * C[i], 0, pooled)
                inp, cin = pooled, C[i]
            else:
                x5 = empty(N, h, w, C[i])
                conv_bn_relu(prefix, 3, zmid, C[i], C[i], h, w, x5, C[i], 0, None)
                inp = x5

        # ---- decoder ----
        for j in range(1, 5):
            lvl = 4 - j                      # output level of up_j
            prefix = f"up{j}"
            cout_t = C[lvl]                                           # skip channels == up-sampled channels
            cin_t = inp.shape[3]                                      # decoder input: 2*cout_t (convT) / cout_t (bilinear)
            h, w = hs[lvl + 1], ws_[lvl + 1]
            H2, W2 = hs[lvl], ws_[lvl]
            pt, pl = (H2 - 2 * h) // 2, (W2 - 2 * w) // 2
            cat = cats[lvl]
            wd = None
            if bilinear:
                # nn.Upsample(scale_factor=2, bilinear, align_corners=True) straight into the concat buffer
                ops.upsample2x_bilinear_fwd(inp, cat, N, h, w, cin_t, H2, W2, out_stride=2 * cout_t, out_coff=cout_t,
                                            ooy=pt, oox=pl)
            else:
                wkey = prefix + ".up.weight"
                wf, wd = self._packed(wkey, params[wkey], True, need_grad)
                bias = params[prefix + ".up.bias"].detach()
                # all four sub-pixel classes in one pointwise GEMM: the input is read once
                ops.upconv2x2_fwd(inp, wf, bias, cat, N, 1, h, w, cin_t, cout_t, 1, H2, W2, out_stride=2 * cout_t,
                                  out_coff=cout_t, ooy=pt, oox=pl)
            if need_grad:
                u = _UpRec()
                u.name, u.zin, u.cat, u.wd = prefix, inp, cat, wd
                u.cin, u.cout, u.h, u.w, u.H2, u.W2, u.pt, u.pl = cin_t, cout_t, h, w, H2, W2, pt, pl
                u.geom_bwd = u.geom_wg = None
                if not bilinear:
                    taps = [(py + pt, px + pl) for py in range(2) for px in range(2)]
                    # the ConvTranspose2d seen from its output side: a stride-2, 4-tap conv dU -> x
                    u.geom_bwd = ops.make_geom(N, H2, W2, cout_t, h, w, cin_t, h, w, taps, isy=2, isx=2,
                                               in_stride=2 * cout_t, in_coff=cout_t)
                ups.append(u)
            cmid = params[prefix + ".conv.double_conv.0.weight"].shape[0]     # in_channels // 2 when bilinear
            cout3 = params[prefix + ".conv.double_conv.3.weight"].shape[0]
            zmid = empty(N, H2, W2, cmid)
            conv_bn_relu(prefix + ".conv", 0, cat, 2 * cout_t, cmid, H2, W2, zmid, cmid, 0, None)
            # last stage in front of the 1x1 head: its activation has one reader, the head, which applies BatchNorm + ReLU on
            # its own load path -- the tensor is not stored (GSSEG_HEAD_FWD_FUSED=0 restores it)
            fuse_head = (j == 4 and FUSED_HEAD_FWD and cout3 == 64 and net.n_classes <= 4
                         and not (FOLD_BN_INFERENCE and not need_grad and not training))
            zout = None if fuse_head else empty(N, H2, W2, cout3)
            last_rec = conv_bn_relu(prefix + ".conv", 3, zmid, cmid, cout3, H2, W2, zout, cout3, 0, None)
            inp = zout

        logits = empty(N, net.n_classes, H, W, dtype=torch.float32)
        if inp is None:
            ops.head1x1_bn_fwd(last_rec.y, last_rec.coef[0], last_rec.coef[1], ACT_RELU,
                               params["outc.conv.weight"].detach().contiguous(), params["outc.conv.bias"].detach(), logits)
        elif net.n_classes <= 4:
            ops.conv_smallcout_fwd(inp, params["outc.conv.weight"].detach().contiguous(),
                                   params["outc.conv.bias"].detach(), logits)
        elif net.n_classes <= 64:
            # 5..64 classes: every class in one launch of the thread-per-pixel head kernel on the single 16-bit plane
            ops.head1x1_wide_fwd(inp, params["outc.conv.weight"].detach().reshape(net.n_classes, 64).contiguous(),
                                 params["outc.conv.bias"].detach(), logits)
        else:
            # more than 64 classes (the reference takes any): the pointwise head kernel in groups of four output channels
            wo, bo = params["outc.conv.weight"].detach(), params["outc.conv.bias"].detach()
            for g0 in range(0, net.n_classes, 4):
                g1 = min(g0 + 4, net.n_classes)
                tmp = empty(N, g1 - g0, H, W, dtype=torch.float32)
                ops.conv_smallcout_fwd(inp, wo[g0:g1].contiguous(), bo[g0:g1].contiguous(), tmp)
                logits[:, g0:g1] = tmp
        _flush_nbt(nbt_pending)
        if labels:                                 # this engine's head is not the pair head: the predicate on its logits
            lab = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
            ops.labels_from_logits(logits, lab)
            return lab, None
        ctx = None
        if need_grad:
            ctx = dict(recs=recs, ups=ups, x=x, z_last=inp, N=N, H=H, W=W, hs=hs, ws=ws_, C=C, training=training)
        return logits, ctx

    # ------------------------------------------------------------------ precise forward
    def _prepack_segs(self, params: Dict[str, torch.Tensor], eff: Dict[str, str]):
        """Segment packs of the pair forward ([taps][Cout][K], K = the stage's concatenation of hi / lo segments; "q" stages: the
        q pack [taps][Cout][2*Cin] + per-cout exponents), every stale one re-packed in ONE launch per kind; cached until the
        Parameter is modified.  eff: the plan with "q" replaced by "xw" where this input size has no "q" kernel."""
        items, fresh, qitems, qfresh = [], [], [], []
        full = all(v == "xw" for v in self.plan.values())
        for st in STAGES:
            mode = eff[st]
            wkey, _, transposed = _stage_keys(st)
            w = params.get(wkey)
            if w is None or w.dim() != 4:
                continue
            cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
            if st == "inc.0":                              # the image-end layer is not packed (any channel count)
                continue
            if transposed and mode == "1" and not full:
                continue                                   # runs on the default LDS-DMA GEMM with the ordinary pack
            lo_len = self._lo_len(st, eff, cin)
            key = (pack_key(w), mode, lo_len)
            ent = self._packs.get(wkey + "|segs")
            if ent is not None and ent[0] == key:
                continue
            if mode == "q":
                pack = torch.empty((w.shape[2] * w.shape[3], cout, 2 * cin), dtype=self.tdt, device=w.device)
                wexp = torch.empty(cout, dtype=torch.int32, device=w.device)
                qitems.append((w.detach().contiguous(), pack, wexp))
                qfresh.append((wkey, key, (pack, wexp)))
                continue
            segs, K, _ = _segs(mode, cin, lo_len)
            pack = torch.empty((w.shape[2] * w.shape[3], cout, K), dtype=self.tdt, device=w.device)
            items.append((w.detach().contiguous(), pack, transposed, segs))
            fresh.append((wkey, key, pack))
        if items:
            ops.pack_weight_segs(items)
        if qitems:
            ops.pack_weight_q8(qitems)
        for wkey, key, pack in fresh + qfresh:
            self._packs[wkey + "|segs"] = (key, pack)

    def _prepack_segs_folded(self, params: Dict[str, torch.Tensor], bufs: Dict[str, torch.Tensor], eff: Dict[str, str]):
        """Inference of the pair forward: BatchNorm(eval) folded into the segment packs -- w' = w * gamma / sqrt(var + eps) per output
        channel (fp32, then split into the stage's hi / lo segments, so the folded weight keeps its ~22 bits) and the bias
        beta - mean * gamma / sqrt(var + eps) that the conv epilogue adds before the ReLU.  Cached until a Parameter or a running
        statistic changes; every stale pack in ONE launch.  Returns False when a BatchNorm has no running statistics."""
        items, fresh = [], []
        for st in STAGES:
            wkey, bnkey, transposed = _stage_keys(st)
            if transposed:
                continue
            w = params.get(wkey)
            if w is None or w.dim() != 4 or st == "inc.0":
                continue                                   # (the image-end stem folds nothing: it is one pass already)
            rm, rv = bufs.get(bnkey + ".running_mean"), bufs.get(bnkey + ".running_var")
            if rm is None or rv is None:
                return False
            gamma, beta = params[bnkey + ".weight"], params[bnkey + ".bias"]
            cin, cout = w.shape[1], w.shape[0]
            lo_len = self._lo_len(st, eff, cin)
            eps = self.submodule(bnkey).eps
            key = tuple(pack_key(t) for t in (w, gamma, beta, rm, rv)) + (eps, eff[st], lo_len)
            ent = self._packs.get(wkey + "|fsegs")
            if ent is not None and ent[0] == key:
                continue
            with torch.no_grad():
                sc = gamma.detach().float() * torch.rsqrt(rv.float() + eps)
                w_eff = (w.detach().float() * sc.view(-1, 1, 1, 1)).contiguous()
                bias = (beta.detach().float() - rm.float() * sc).contiguous()
            segs, K, _ = _segs(eff[st], cin, lo_len)
            pack = torch.empty((9, cout, K), dtype=self.tdt, device=w.device)
            items.append((w_eff, pack, False, segs))
            fresh.append((wkey, key, pack, bias))
        if items:
            ops.pack_weight_segs(items)
        for wkey, key, pack, bias in fresh:
            self._packs[wkey + "|fsegs"] = (key, pack, bias)
        return True

    def _seg_pack(self, wkey: str):
        return self._packs[wkey + "|segs"][1]

    def _lo_len(self, st: str, eff: Dict[str, str], cin: int):
        """leading channels of the lo plane of stage `st`'s input that are valid (None: all cin; the lo_len of _segs).  The decoder
        entry conv behind a "1" transposed conv of a plan that is not all-"xw": that conv runs on the LDS-DMA GEMM and writes the
        hi plane only, so the up half of the concat buffer carries no lo plane.  (Behind the bilinear up-sampling the lo plane is
        written whenever the stage has an x_lo segment, and without one _segs does not look at lo_len.)  The segment packs and the
        K / wrap the kernels are launched with both come from here."""
        if (st.endswith(".conv.0") and eff[st[:-len(".conv.0")] + ".up"] == "1" and not self.net.bilinear
                and not all(v == "xw" for v in self.plan.values())):
            return cin // 2
        return None

    def forward_precise(self, x: torch.Tensor, params: Dict[str, torch.Tensor], training: bool, need_grad: bool, labels: bool = False):
        """The pair forward: every activation and conv output travels as a PAIR of 16-bit values v = hi + lo (hi = 16-bit(v),
        lo = 16-bit(v - hi): ~22 significand bits in fp16); BatchNorm / ReLU / max-pool / the head read and write pairs.  The
        MFMA contraction of a stage runs over a K concatenation of SEGMENTS chosen by `self.plan` (exact products, one fp32
        accumulator): "xw" = [x_hi | x_lo | x_hi] . [w_hi | w_hi | w_lo] (3x the MFMA work), "x" / "w" two of them, "1" = x_hi . w_hi.
          precise=True    every stage "xw": max |dlogit| ~1e-5 against the fp32 reference (unet/unet_model.py:26-37).
          precise="mixed" "xw" on the nine stages that make the 16-bit error (MIXED_XW; tools/parity_attribution.py), "1"
                          elsewhere: max |dlogit| 5e-4 .. 7e-4 -- the north star's 1e-3 -- for half the extra MFMA work.
        In a plan that is not all-"xw": the one-channel stem runs as in the default engine (statistics from the image, conv +
        BatchNorm + ReLU in one pass -> z pair, conv output never stored); a "1" transposed conv runs on the LDS-DMA GEMM
        and writes the hi plane only (the consumer's x_lo segment then covers the skip half alone); the head reads the last
        stage's conv-output pair with BatchNorm + ReLU on its load path; lo planes nobody reads are not written.

        HBM layout: a pair buffer is [N,h,w,2*Ct] = [hi plane (Ct) | lo plane (Ct)]; for the concat levels Ct = 2C with
        skip in channels [0,C) and the up-sampled tensor in [C,2C) of EACH plane.  Raw conv outputs are two dense tensors.
        The backward pass is the default one: it reads the hi halves (exactly what the default mode stores) through
        strides, so gradients have the default mode's accuracy."""
        net = self.net
        bilinear = bool(net.bilinear)
        if not ops.USE_HALO_CONV:
            raise RuntimeError("precise mode needs the halo-reuse conv kernel (GSSEG_CONV3X3=halo)")
        N, _, H, W = x.shape
        dev, tdt = x.device, self.tdt
        x = x.contiguous().float()
        bufs = self.buffer_dict()
        nbt_pending = []
        hs = [H >> i for i in range(5)]
        ws_ = [W >> i for i in range(5)]
        C = [64, 128, 256, 512, 1024 // (2 if bilinear else 1)]      # unet_model.py:18-19
        plan = self.plan
        full = all(v == "xw" for v in plan.values())
        if not pack_reuse_allowed(need_grad, self.trust_versions):
            self._packs.clear()                            # `.data` writes are invisible to the version keys
        # "q" stages exist on the LDS-DMA kernel only (W >= 24, channels % 64 == 0, fp16): elsewhere they run as "xw"
        lvl_of = {"inc": 0, "down1": 1, "down2": 2, "down3": 3, "down4": 4, "up1": 3, "up2": 2, "up3": 1, "up4": 0}
        eff = dict(plan)
        for st_, m_ in plan.items():
            if m_ == "q":
                w_ = params.get(_stage_keys(st_)[0])
                lv = lvl_of[st_.split(".")[0]]
                ok = (not st_.endswith(".up") and st_ != "inc.0" and w_ is not None and self.dtype == "f16"
                      and ops.conv3x3_q8_ok(ws_[lv], w_.shape[1], w_.shape[0]))
                if not ok:
                    eff[st_] = "xw"
        plan = eff
        if need_grad or not full:
            self._prepack(params, need_grad, conv_fwd=False)      # the backward's data-gradient packs / the "1" up-convs' packs, one launch
        self._prepack_segs(params, eff)                    # the forward's segment packs, one launch per kind
        # inference (eval mode, no graph): BatchNorm folded into the segment packs, conv + bias + ReLU write the z pair directly and
        # the 2x2 pool of a Down block is a read-only pass over the skip pair (as the 16-bit engine does it, unet_engine.forward)
        fold = (FOLD_BN_INFERENCE and not training and not need_grad and "q" not in eff.values()
                and self._prepack_segs_folded(params, bufs, eff))

        def empty(*shape, dtype=tdt):
            return torch.empty(shape, dtype=dtype, device=dev)

        recs: List[_ConvRec] = []
        ups: List[_UpRec] = []

        def stage(prefix, idx, inp, cin, cout, h, w, zbuf, z_stride, want_lo, zp=None, zp_want_lo=False, image=False,
                  to_head=False):
            """prefix.double_conv.{idx} conv + BN + ReLU on pairs.  inp: fp32 image or a pair buffer [N,h,w,2*cin]; the z pair
            goes to channels [0,cout) / [z_stride/2, z_stride/2 + cout) of zbuf (pixel stride z_stride), the lo plane only when
            a consumer reads it; zp: pooled pair buffer [.., 2*cout].  to_head: BatchNorm + ReLU are left to the head's load
            path (returns the record; nothing stored).  The valid part of the input's lo plane: self._lo_len, as the packs."""
            short = prefix.replace(".maxpool_conv.1", "") + f".{idx}"
            wkey, bnkey = f"{prefix}.double_conv.{idx}.weight", f"{prefix}.double_conv.{idx + 1}"
            wparam = params[wkey]
            rm = bufs.get(bnkey + ".running_mean")
            batch_stats = training or rm is None
            rec = _ConvRec()
            rec.name, rec.wkey, rec.bnkey = f"{prefix}.{idx}", wkey, bnkey
            wide_img = image and cin > 4                    # more than four image channels: the fp32 MFMA stem (csrc/stem_wide.hip)
            rec.cin, rec.cout, rec.h, rec.w, rec.inp_is_image = cin, cout, h, w, image and not wide_img
            rec.inp, rec.train_stats, rec.geom, rec.z, rec.tap_sums = inp, batch_stats, None, None, None
            rec.inp_stride = None if image else 2 * cin
            ntiles = ops.conv_widecin_mtiles(N, h, w) if wide_img else ops.conv_smallcin_mtiles(N, h, w) if image else (
                ops.conv3x3_stat_rows(N, h, w, 2 * cin, cout, pair="q") if plan[short] == "q" else ops.conv3x3_stat_rows(N, h, w, cin, cout, pair=True))
            partials = empty(ops.bn_partials_numel(ntiles, cout), dtype=torch.float32) if batch_stats else None
            want_lo, zp_want_lo = int(want_lo), int(zp_want_lo)     # 0 none / 1 16-bit lo plane / 2 q plane (lo_fmt below)
            z_lo = zbuf[..., z_stride // 2:] if (zbuf is not None and want_lo) else None
            if (image and not full and FUSED_STEM_FWD and cin == 1 and cout == 64 and zp is None and z_stride == 2 * cout
                    and inp.is_contiguous()):
                # one-channel stem as in the default engine: statistics from the image, one pass writes the z pair
                wst = wparam.detach().contiguous()
                if need_grad:
                    rec.tap_sums = (empty(ntiles * 54, dtype=torch.float32) if batch_stats
                                    else torch.zeros(ntiles * 54, dtype=torch.float32, device=dev))
                if batch_stats:
                    ops.stem_stats(inp, wst, partials, rec.tap_sums)
                coef = bn_coeffs(self.submodule(bnkey), partials, ntiles, cout, N * h * w, training, dev, nbt_pending)[0]
                if want_lo == 2:
                    ops.stem_fwd_bn_pair_q8(inp, wst, coef[0], coef[1], ACT_RELU, zbuf)
                else:
                    ops.stem_fwd_bn_pair(inp, wst, coef[0], coef[1], ACT_RELU, zbuf, write_lo=bool(want_lo))
                rec.y, rec.coef, rec.z, rec.wd = None, coef, zbuf, None
                if need_grad:
                    recs.append(rec)
                return rec
            if fold and not image and not batch_stats:
                _, fpack, fbias = self._packs[wkey + "|fsegs"]
                _, K, wrap = _segs(plan[short], cin, self._lo_len(short, plan, cin))
                if to_head:                                # the head reads a dense pair
                    zd = empty(2, N, h, w, cout)
                    ops.conv3x3_segs(inp, fpack, zd[0], zd[1], N, h, w, K, wrap, cin, cout, in_stride=2 * cin, bias=fbias, act=ACT_RELU)
                    return zd
                ops.conv3x3_segs(inp, fpack, zbuf, zbuf[..., z_stride // 2:], N, h, w, K, wrap, cin, cout, in_stride=2 * cin,
                                 out_stride=z_stride, out_coff=0, bias=fbias, act=ACT_RELU)
                if zp is not None:
                    ops.maxpool2x2_fwd_pair(zbuf, zbuf[..., z_stride // 2:], z_stride, zp, zp[..., zp.shape[3] // 2:], zp.shape[3],
                                            N, h, w, cout)
                return None
            y_hi, y_lo = empty(N, h, w, cout), empty(N, h, w, cout)
            lo_layout = ops.LO_DENSE                        # of y_lo: asked once, handed to the conv and to the plane's one reader
            if wide_img:
                # the conv-output pair and the statistics from the fp32 image and weights: no 16-bit image in the forward
                ops.conv_widecin_fwd_split(inp, wparam.detach().contiguous(), y_hi, y_lo, partials)
                if need_grad:
                    # what the backward's wide image stage reads (as the 16-bit engine's forward builds it): the image as a 16-bit
                    # NHWC tensor zero-padded to a multiple of 8 channels, the weight's data-gradient pack padded alike
                    cpad = (cin + 7) // 8 * 8
                    xin = (torch.zeros if cpad != cin else torch.empty)((N, h, w, cpad), dtype=tdt, device=dev)
                    ops.nchw_to_nhwc(inp, xin, dst_stride=cpad)
                    rec.inp, rec.cin, rec.wide = xin, cpad, cin
            elif image:
                ops.conv_smallcin_fwd_split(inp, wparam.detach().contiguous(), y_hi, y_lo, partials, 3, 1)
            elif plan[short] == "q":
                qpack, wexp = self._seg_pack(wkey)
                ops.conv3x3_q8(inp, qpack, wexp, y_hi, y_lo, N, h, w, cin, cout, in_stride=2 * cin, bn_partials=partials)
            else:
                _, K, wrap = _segs(plan[short], cin, self._lo_len(short, plan, cin))
                if partials is not None and want_lo != 2 and zp_want_lo != 2:      # (the q-plane apply pass reads a dense lo plane)
                    lo_layout = ops.conv3x3_pair_lo_layout(N, h, w, K, cout)
                ops.conv3x3_segs(inp, self._seg_pack(wkey), y_hi, y_lo, N, h, w, K, wrap, cin, cout, in_stride=2 * cin,
                                 bn_partials=partials, lo_layout=lo_layout)
            coef = bn_coeffs(self.submodule(bnkey), partials, ntiles, cout, N * h * w, training, dev, nbt_pending)[0]
            rec.y, rec.coef = y_hi, coef
            if wide_img:
                rec.wd = self._packed_padded(wkey, wparam, rec.cin, True)[1] if need_grad else None
            else:
                rec.wd = None if image else (self._packed(wkey, wparam, False, True, need_fwd=False)[1] if need_grad else None)
            if need_grad:
                recs.append(rec)
            if to_head:
                return rec, y_lo, lo_layout
            zp_hi = zp if zp is not None else None
            zp_lo = zp[..., zp.shape[3] // 2:] if (zp is not None and zp_want_lo) else None
            if want_lo == 2 or zp_want_lo == 2:
                ops.bn_act_apply_split_q8(y_hi, y_lo, coef[0], coef[1], ACT_RELU, zbuf, z_lo, want_lo == 2, z_stride, 0, zp_hi, zp_lo,
                                          zp_want_lo == 2, 0 if zp is None else zp.shape[3])
            else:
                ops.bn_act_apply_split(y_hi, y_lo, coef[0], coef[1], ACT_RELU, zbuf, z_lo, z_stride, 0, zp_hi, zp_lo,
                                       0 if zp is None else zp.shape[3], lo_layout=lo_layout)
            return rec

        def reads_lo(st):
            """the form in which consumer stage `st` reads the lo plane of its input: 0 not at all, 1 a 16-bit lo plane (an x_lo
            segment), 2 a q plane (FP8 correction chunks)"""
            return 2 if plan[st] == "q" else (1 if "x" in plan[st] else 0)

        # ---- encoder ----
        cats = [None] * 4
        for i in range(4):
            zero_needed = (hs[i] - 2 * hs[i + 1]) or (ws_[i] - 2 * ws_[i + 1])
            alloc = torch.zeros if zero_needed else torch.empty
            cats[i] = alloc((N, hs[i], ws_[i], 4 * C[i]), dtype=tdt, device=dev)      # [skip_h up_h | skip_l up_l]
        inp, cin = x, net.n_channels
        for i in range(5):
            prefix = "inc" if i == 0 else f"down{i}.maxpool_conv.1"
            blk = "inc" if i == 0 else f"down{i}"
            h, w = hs[i], ws_[i]
            zmid = empty(N, h, w, 2 * C[i])
            stage(prefix, 0, inp, cin, C[i], h, w, zmid, 2 * C[i], reads_lo(blk + ".3"), image=(i == 0))
            if i < 4:
                pooled = empty(N, hs[i + 1], ws_[i + 1], 2 * C[i])
                stage(prefix, 3, zmid, C[i], C[i], h, w, cats[i], 4 * C[i], reads_lo(f"up{4 - i}.conv.0"),
                      zp=pooled, zp_want_lo=reads_lo(f"down{i + 1}.0"))
                inp, cin = pooled, C[i]
            else:
                x5 = empty(N, h, w, 2 * C[i])
                stage(prefix, 3, zmid, C[i], C[i], h, w, x5, 2 * C[i], reads_lo("up1.up") or bilinear)   # (the pair up-sampling reads both planes)
                inp = x5

        # ---- decoder ----
        z_last = None
        for j in range(1, 5):
            lvl = 4 - j
            prefix = f"up{j}"
            cout_t = C[lvl]                                           # skip channels == up-sampled channels
            cin_t = inp.shape[3] // 2                                 # decoder input: 2*cout_t (convT) / cout_t (bilinear)
            h, w = hs[lvl + 1], ws_[lvl + 1]
            H2, W2 = hs[lvl], ws_[lvl]
            pt, pl = (H2 - 2 * h) // 2, (W2 - 2 * w) // 2
            cat = cats[lvl]
            wkey = prefix + ".up.weight"
            up_mode = plan[prefix + ".up"]
            if bilinear:
                # nn.Upsample(scale_factor=2, bilinear, align_corners=True) of the PAIR (unet_parts.py:49-50), straight into the up
                # half of both planes of the concat buffer; the lo plane only when the consumer runs an x_lo segment
                want = reads_lo(prefix + ".conv.0")
                if want == 2:
                    raise NotImplementedError("a 'q' stage behind the bilinear up-sampling (its pair kernel writes 16-bit lo planes)")
                ops.upsample2x_bilinear_fwd_pair(inp, inp[..., cin_t:], cat, cat[..., 2 * cout_t:] if want else None, N, h, w,
                                                 cin_t, H2, W2, in_stride=2 * cin_t, out_stride=4 * cout_t, out_coff=cout_t,
                                                 ooy=pt, oox=pl)
            elif up_mode == "1" and not full:
                # x_hi . w_hi on the LDS-DMA pointwise GEMM, hi plane only: the consumer's x_lo segment skips the up half
                wf, _ = self._packed(wkey, params[wkey], True, need_grad)
                ops.upconv2x2_fwd(inp, wf, params[prefix + ".up.bias"].detach(), cat, N, 1, h, w, cin_t, cout_t, 1, H2, W2,
                                  in_stride=2 * cin_t, out_stride=4 * cout_t, out_coff=cout_t, ooy=pt, oox=pl)
                if reads_lo(prefix + ".conv.0") == 2:
                    # the consumer is a "q" stage: the q chunks of the up half -- hi8 from the hi plane just written, lo8 = 0 (its
                    # x_lo . w_hi term then covers the skip channels only, exactly like the 16-bit "lo_len" segment)
                    ops.q8_from_hi(cat, cat[..., 2 * cout_t:], N * H2 * W2, cout_t, 4 * cout_t, cout_t)
            else:
                if reads_lo(prefix + ".conv.0") == 2:
                    raise NotImplementedError("a 'q' stage behind a pair transposed conv (it writes 16-bit lo planes)")
                _, K, wrap = _segs(up_mode, cin_t)
                ops.upconv2x2_fwd_segs(inp, self._seg_pack(wkey), params[prefix + ".up.bias"].detach(),
                                       cat[..., cout_t:], cat[..., 3 * cout_t:], N, h, w, K, wrap, cin_t, cout_t, H2, W2,
                                       in_stride=2 * cin_t, out_stride=4 * cout_t, ooy=pt, oox=pl)
            if need_grad:
                u = _UpRec()
                u.name, u.zin, u.cat = prefix, inp, cat
                u.cin, u.cout, u.h, u.w, u.H2, u.W2, u.pt, u.pl = cin_t, cout_t, h, w, H2, W2, pt, pl
                u.wd = u.geom_bwd = u.geom_wg = None
                if not bilinear:
                    u.wd = self._packed(wkey, params[wkey], True, True)[1]
                    taps = [(py + pt, px + pl) for py in range(2) for px in range(2)]
                    # the transposed conv seen from its output side (dU -> dx); dU is the up half of the DENSE gradient of the
                    # concat input, x the hi plane of the pair buffer (pixel stride 2*cin_t) for the weight gradient
                    u.geom_bwd = ops.make_geom(N, H2, W2, cout_t, h, w, cin_t, h, w, taps, isy=2, isx=2,
                                               in_stride=2 * cout_t, in_coff=cout_t)
                    u.geom_wg = ops.make_geom(N, H2, W2, cout_t, h, w, cin_t, h, w, taps, isy=2, isx=2,
                                              in_stride=2 * cout_t, in_coff=cout_t, out_stride=2 * cin_t)
                ups.append(u)
            cmid = params[prefix + ".conv.double_conv.0.weight"].shape[0]     # in_channels // 2 when bilinear
            cout3 = params[prefix + ".conv.double_conv.3.weight"].shape[0]
            zmid = empty(N, H2, W2, 2 * cmid)
            stage(prefix + ".conv", 0, cat, 2 * cout_t, cmid, H2, W2, zmid, 2 * cmid, reads_lo(prefix + ".conv.3"))
            if j < 4:
                zout = empty(N, H2, W2, 2 * cout3)
                nxt_lo = True if bilinear else reads_lo(f"up{j + 1}.up")      # (the pair up-sampling interpolates both planes)
                stage(prefix + ".conv", 3, zmid, cmid, cout3, H2, W2, zout, 2 * cout3, nxt_lo)
                inp = zout
            elif fold:                             # folded inference: the last stage leaves a dense z pair for the plain pair head
                zl = stage(prefix + ".conv", 3, zmid, cmid, cout3, H2, W2, None, 0, False, to_head=True)
                zl_hi, zl_lo = zl[0], zl[1]
                last_rec = None
                z_last = zl_hi
            elif not full and FUSED_HEAD_FWD and cout3 == 64 and net.n_classes <= 4:
                # last stage: its activation has one reader, the head, which applies BatchNorm + ReLU on its own load path
                last_rec, y_lo_last, lo_last = stage(prefix + ".conv", 3, zmid, cmid, cout3, H2, W2, None, 0, False, to_head=True)
            else:                                  # last stage: two dense planes (the head and its backward read dense tensors)
                zl = empty(2, N, H2, W2, cout3)
                zl_hi, zl_lo = zl[0], zl[1]
                last_rec = None
                st_rec = stage(prefix + ".conv", 3, zmid, cmid, cout3, H2, W2, None, 0, False, to_head=True)
                ops.bn_act_apply_split(st_rec[0].y, st_rec[1], st_rec[0].coef[0], st_rec[0].coef[1], ACT_RELU, zl_hi, zl_lo,
                                       cout3, 0, lo_layout=st_rec[2])
                z_last = zl_hi

        if labels:
            # UNet.predict: the same head launch with the label epilogue (gs_head1x1_labels) -- no logits tensor is allocated
            lab = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
            wout = params["outc.conv.weight"].detach().reshape(net.n_classes, 64).contiguous()
            if z_last is None:
                ops.head1x1_labels(last_rec.y, y_lo_last, wout, params["outc.conv.bias"].detach(), lab, last_rec.coef[0],
                                   last_rec.coef[1], ACT_RELU, lo_layout=lo_last)
            else:
                ops.head1x1_labels(zl_hi, zl_lo, wout, params["outc.conv.bias"].detach(), lab)
            _flush_nbt(nbt_pending)
            return lab, None
        logits = empty(N, net.n_classes, H, W, dtype=torch.float32)
        if z_last is None:
            ops.head1x1_bn_fwd_split(last_rec.y, y_lo_last, last_rec.coef[0], last_rec.coef[1], ACT_RELU,
                                     params["outc.conv.weight"].detach().contiguous(), params["outc.conv.bias"].detach(), logits,
                                     lo_layout=lo_last)
        else:
            ops.head1x1_fwd_split(zl_hi, zl_lo, params["outc.conv.weight"].detach().contiguous(),
                                  params["outc.conv.bias"].detach(), logits)
        _flush_nbt(nbt_pending)
        ctx = None
        if need_grad:
            ctx = dict(recs=recs, ups=ups, x=x, z_last=z_last, N=N, H=H, W=W, hs=hs, ws=ws_, C=C, training=training)
        return logits, ctx

    # ------------------------------------------------------------------ backward
    def backward(self, ctx, params: Dict[str, torch.Tensor], dlogits: torch.Tensor, need_dx: bool):
        net, tdt = self.net, self.tdt
        N, H, W, hs, ws_, C = ctx["N"], ctx["H"], ctx["W"], ctx["hs"], ctx["ws"], ctx["C"]
        dev = dlogits.device
        if self.dynamic_loss_scale and self.grad_ready_hook is not None:
            # (before any kernel or collective: the bucket all-reduces would be issued on gradients renormalised by THIS rank's
            # factor, and raising later would leave the reducer's asynchronous work un-waited)
            raise RuntimeError("dynamic_loss_scale is not supported together with the bucketed GradReducer")
        recs: Dict[str, _ConvRec] = {r.name: r for r in ctx["recs"]}
        ups: Dict[str, _UpRec] = {u.name: u for u in ctx["ups"]}
        # Gradients travel in 16 bits multiplied by a power-of-two scale S so that fp16 neither underflows nor overflows.
        # The static choice S = 2^round(log2(N*H*W)) assumes |dlogits| ~ 1/(N*H*W): a MEAN-reduced loss with O(1)..O(100)
        # weights (every loss of the reference's scripts).  A sum-reduced loss, a 1e4 loss weight or torch's GradScaler
        # (x65536) breaks that assumption: set `dynamic_loss_scale` (UNet(..., dynamic_loss_scale=True) /
        # GSSEG_DYNAMIC_LOSS_SCALE=1) and the incoming gradient is renormalised ON THE DEVICE (no host sync) by a power of
        # two derived from its own amax; the parameter gradients are multiplied back at the end (exact).  bf16 does not need it.
        S = float(2 ** round(math.log2(N * H * W)))
        inv_s = 1.0 / S
        renorm = None
        if self.dynamic_loss_scale:
            amax = dlogits.detach().abs().amax().float()
            # r = 2^k with amax * S * r in [1, 2): the head's fp16 data gradient then has the magnitude the static scale
            # is designed for (mean-reduced CE / BCE: amax * N*H*W ~ 1)
            k = torch.floor(-torch.log2(torch.clamp(amax * S, min=1e-30)))
            renorm = torch.exp2(torch.clamp(k, -60.0, 60.0))
            dlogits = dlogits * renorm
        grads: Dict[str, torch.Tensor] = {}

        def empty(*shape, dtype=tdt):
            return torch.empty(shape, dtype=dtype, device=dev)

        def emit(name, g):
            grads[name] = g
            if self.grad_ready_hook is not None:
                self.grad_ready_hook(name, g)

        # The MFMA weight gradients of levels 1-4 and of the transposed convolutions (with their ordered slab reductions) run
        # on a SECOND stream: nothing downstream in the backward pass needs them.  A stage launches its data gradient on the
        # main stream FIRST and hands the weight gradient over behind it, so the weight gradient of stage L runs while the
        # main stream does reduce / coeffs / apply of stage L-1 (launched in front of the data gradient, both persistent
        # MFMA grids, it would be finished before any BatchNorm kernel starts).  A 128-cout weight-gradient block keeps two
        # 208-register waves on every SIMD, which leaves 96 of the 512 registers: the BatchNorm kernels only become
        # co-resident in their slim form (ops.bn_bwd_set_form, <= 96 VGPRs), taken for the plain launches of levels 1-4 from
        # the hand-over of such a weight gradient until the next join: it may still be running behind whatever was handed over
        # after it (in an Up block the 2C -> C weight gradient behind the transposed convolution's); the normal forms
        # (109-172 VGPRs) wait for a CU to drain.  Level 0 (the 64-cout LDS-DMA kernel leaves 80 registers and streams
        # ~5 TB/s itself) stays on the main stream, and its BatchNorm launches on the normal form.  dY is handed
        # over with an event; tensors the side stream reads are recorded on it (caching allocator); wg_ws is touched on the
        # main stream only after a join; the main stream joins at the end.  With a gradient-ready hook (bucketed
        # all-reduce) a weight gradient is announced one stage later, after the main stream has waited for its event.
        # GSSEG_WGRAD_STREAM=0 keeps everything on one stream, and so does a stream under capture (graphs keep their shape).
        main_stream = torch.cuda.current_stream(dev)
        two_streams = WGRAD_SIDE_STREAM and not torch.cuda.is_current_stream_capturing()
        self.last_backward_streams = 2 if two_streams else 1
        side = self._side_stream(dev) if two_streams else None
        deferred = []                # (name, grad, event) of side-stream gradients not yet announced
        side_busy = [False]          # something was handed to the side stream since the last join
        slim_bn = [False]            # ... and some of it is a weight gradient that leaves 96 registers per SIMD lane

        def flush_deferred(upto_all: bool):
            while deferred and (upto_all or len(deferred) > 1):
                name, g, ev = deferred.pop(0)
                main_stream.wait_event(ev)
                emit(name, g)

        def join_side():
            """the main stream waits for everything handed to the side stream (before it touches wg_ws itself)"""
            if side is not None and side_busy[0]:
                flush_deferred(True)
                main_stream.wait_stream(side)
                side_busy[0] = slim_bn[0] = False

        def on_side(inputs, fn, name, g, beside=True, leaves_96=False):
            """run fn() (launches that read `inputs`, already complete on the main stream, and write g) on the side stream;
            beside=False: on the main stream, after a join.  leaves_96: see slim_bn"""
            if side is None or not beside:
                join_side()
                fn()
                emit(name, g)
                return
            side_busy[0], slim_bn[0] = True, slim_bn[0] or leaves_96
            ev = torch.cuda.Event()
            ev.record(main_stream)
            for t_ in inputs:
                t_.record_stream(side)
            with torch.cuda.stream(side):
                side.wait_event(ev)
                fn()
                if self.grad_ready_hook is not None:
                    done = torch.cuda.Event()
                    done.record(side)
                    deferred.append((name, g, done))
            if self.grad_ready_hook is None:
                grads[name] = g
            else:
                flush_deferred(False)

        def galloc(name, like, zero=False):
            if self.grad_alloc is not None:
                g = self.grad_alloc(name, like)
                if zero:
                    g.zero_()
                return g
            return (torch.zeros_like if zero else torch.empty_like)(like, memory_format=torch.contiguous_format)

        # workspaces
        # one zeroed arena for every MFMA weight-gradient accumulator of this backward (fp32 atomics need zeros):
        # ONE fill of 124 MB instead of a small fill in front of each of the 22 wgrad launches
        # 3x3 weight gradients: split-K parts in slabs + ordered reduction fused with scale / unpack -- deterministic,
        # no atomics, no zero fill.  (GSSEG_WGRAD_DET=0: layers with fewer than 8 parts fall back to fp32 atomics;
        # measured equal within noise on the headline config.)
        det_min = 8 if os.environ.get("GSSEG_WGRAD_DET", "1") == "0" else 1
        det_recs = set()
        wg_need, tot_w = 1, 0
        for r in ctx["recs"]:
            wnum = params[r.wkey].numel()
            if (not r.inp_is_image and ops.USE_HALO_CONV and r.cin % 8 == 0 and r.cout % 8 == 0 and
                    ops.conv3x3_wgrad_parts(N, r.h, r.w, r.cin, r.cout) >= det_min):
                det_recs.add(r.name)
                wg_need = max(wg_need, ops.conv3x3_wgrad_ws_floats(N, r.h, r.w, r.cin, r.cout))
            elif not r.inp_is_image:
                tot_w += wnum
        for u in ctx["ups"]:
            if u.geom_bwd is not None:                   # ConvTranspose2d weight gradient: slabs too (deterministic)
                wg_need = max(wg_need, ops.conv_wgrad_ws_floats(u.geom_wg if u.geom_wg is not None else u.geom_bwd),
                              ops.upconv2x2_wgrad_ws_floats(N, u.h, u.w, u.cin, u.cout))
        dw_arena = torch.zeros(max(tot_w, 1), dtype=torch.float32, device=dev)
        wg_ws = empty(wg_need, dtype=torch.float32)
        arena_off = [0]

        def dw_take(numel):
            a = arena_off[0]
            arena_off[0] = a + numel
            return dw_arena[a:a + numel]
        npart = 0
        for i in range(5):
            npart = max(npart, ops.bn_partials_numel(ops.bn_bwd_tiles(N, hs[i], ws_[i]), C[i]))
            if i == 0:
                npart = max(npart, ops.bn_partials_numel(ops.stem_bwd_tiles(N, hs[i], ws_[i]), 64))
            if i < 4 and ops.USE_HALO_CONV:          # the data-gradient convolution's partials over d(concat) (fused bias gradient)
                npart = max(npart, ops.bn_partials_numel(ops.conv3x3_mtiles(N, hs[i], ws_[i], 2 * C[i]), 2 * C[i]))
                if N * hs[i] * ws_[i] <= 8192:      # ... one row per 16 pixels when the weight-streaming form runs it
                    npart = max(npart, ops.bn_partials_numel(-(-(N * hs[i] * ws_[i]) // 16), 2 * C[i]))
        partials = empty(npart, dtype=torch.float32)
        col_ws = empty(1024 * 1024, dtype=torch.float32)

        # ---- head ----
        z_last = ctx["z_last"]
        dl = (dlogits.contiguous().float() * S)
        wout = params["outc.conv.weight"]
        dwo = galloc("outc.conv.weight", wout, zero=True)
        dbo = galloc("outc.conv.bias", params["outc.conv.bias"], zero=True)
        # the data gradient of the head (dl . W, 268 MB at batch 32) is not written: the BatchNorm backward of the last stage
        # forms it from dl (GSSEG_HEAD_BWD_FUSED=0 restores the tensor)
        head_src = None
        wout_c = wout.detach().contiguous()
        rlast = recs["up4.conv.3"]
        if z_last is None:                       # the last activation was never stored: the head's weight gradient re-forms it
            ops.head1x1_bn_wgrad(rlast.y, rlast.coef[0], rlast.coef[1], ACT_RELU, wout_c, dl, dwo, dbo, gscale=inv_s)
        if FUSED_HEAD_BWD and wout.shape[0] <= 4 and dl.is_contiguous():
            head_src = (dl, wout_c)
            dz = None
            if z_last is not None:
                ops.conv_smallcout_bwd(z_last, wout_c, dl, None, dwo, dbo, gscale=inv_s)
        elif 4 < wout.shape[0] <= 64:
            # 5..64 classes: ONE data-gradient launch (the class sum in fp32, rounded once) and one weight-gradient launch
            dz = empty(N, H, W, 64)
            ops.head1x1_wide_bwd(z_last, wout_c.reshape(wout.shape[0], 64), dl, dz, dwo, dbo, gscale=inv_s)
        elif wout.shape[0] > 64:
            # more than 64 classes (16-bit engine only): groups of four output channels, data gradients summed in fp32
            dzs = torch.zeros((N, H, W, 64), dtype=torch.float32, device=dev)
            for g0 in range(0, wout.shape[0], 4):
                g1 = min(g0 + 4, wout.shape[0])
                dzg = empty(N, H, W, 64)
                ops.conv_smallcout_bwd(z_last, wout_c[g0:g1].contiguous(), dl[:, g0:g1].contiguous(), dzg, dwo[g0:g1], dbo[g0:g1],
                                       gscale=inv_s)
                dzs += dzg
            dz = dzs.to(tdt)
        else:
            dz = empty(N, H, W, 64)
            if z_last is not None:
                ops.conv_smallcout_bwd(z_last, wout_c, dl, dz, dwo, dbo, gscale=inv_s)
            else:
                ops.conv_smallcout_bwd(None, wout_c, dl, dz, None, None)
        emit("outc.conv.weight", dwo)
        emit("outc.conv.bias", dbo)

        def conv_stage_bwd(rec: _ConvRec, dz_a, sa, ca, dzp, need_dinp: bool, colsum=None, head=None):
            """Backward of conv -> BN -> ReLU.  Returns d(input) (dense NHWC) or None.
            colsum = (coff, C, out): also out[c] = inv_s * sum over pixels of d(input)[..., coff + c], from the data-gradient
            convolution's epilogue sums (the bias gradient of the transposed convolution that feeds this stage).
            head = (dl, w_head): the gradient source is the pointwise head's logit gradient and weight instead of dz_a."""
            h, w, cin, cout = rec.h, rec.w, rec.cin, rec.cout
            coef = rec.coef
            pooled = dzp is not None
            if rec.y is None:
                # the stem's convolution output was never stored: both backward passes re-form it from the image
                wst = params[rec.wkey].detach().contiguous()
                done = False
                if not need_dinp and not pooled and head is None:
                    # one pass over z (its sign) and dz; BatchNorm and weight gradients in closed form from A = sum g x_tap,
                    # s1 = sum g and the image's tap sums / Gram matrix
                    nts = ops.stem_bwd_tiles(N, h, w)
                    sws = empty(nts * 576, dtype=torch.float32)
                    s1p = empty(nts * 64, dtype=torch.float32)
                    if ops.stem_bwd_onepass(rec.inp, rec.z, dz_a, sa, ca, ACT_RELU, s1p, sws, z_stride=rec.z.shape[3]):
                        dgamma = galloc(rec.bnkey + ".weight", params[rec.bnkey + ".weight"])
                        dbeta = galloc(rec.bnkey + ".bias", params[rec.bnkey + ".bias"])
                        dw = galloc(rec.wkey, params[rec.wkey], zero=True)
                        ops.stem_bwd_finalize(sws, s1p, rec.tap_sums, wst, coef[0], coef[2], coef[3], rec.train_stats, inv_s,
                                              dw, dgamma, dbeta, N, h, w)
                        emit(rec.wkey, dw)
                        emit(rec.bnkey + ".weight", dgamma)
                        emit(rec.bnkey + ".bias", dbeta)
                        done = True
                if done:
                    return None
                y_re = empty(N, h, w, cout)                  # image gradient wanted / very wide image: the tensor path
                ops.conv_smallcin_fwd(rec.inp, wst, None, y_re, None, 3, 1, 1)
                rec.y = y_re
            ntiles = ops.bn_bwd_tiles_used(N, h, w, pooled)
            # plain launches of levels 1-4 beside a weight gradient that may still be running
            slim = slim_bn[0] and not pooled and head is None and (h, w) != (hs[0], ws_[0])
            if head is not None:
                ops.bn_act_bwd_reduce_head(rec.y, head[0], head[1], coef[0], coef[1], coef[2], coef[3], ACT_RELU, partials)
            else:
                with ops.bn_bwd_form(ops.BN_BWD_SLIM if slim else ops.BN_BWD_NORMAL):
                    ops.bn_act_bwd_reduce(rec.y, dz_a, sa, ca, dzp, coef[0], coef[1], coef[2], coef[3], ACT_RELU, partials)
            dgamma = galloc(rec.bnkey + ".weight", params[rec.bnkey + ".weight"])
            dbeta = galloc(rec.bnkey + ".bias", params[rec.bnkey + ".bias"])
            c12 = empty(2, cout, dtype=torch.float32)
            ops.bn_bwd_coeffs(partials, ntiles, cout, N * h * w, inv_s, dgamma, dbeta, c12[0], c12[1])
            if not rec.train_stats:
                c12.zero_()          # eval-mode BN: statistics are constants
            wparam = params[rec.wkey]
            dw_stem = None
            if (rec.inp_is_image and not need_dinp and not pooled and FUSED_STEM_BWD and cin == 1 and cout == 64
                    and rec.inp.is_contiguous()):
                # one-channel stem, image without gradient: d(conv output) has one consumer, the weight gradient -- both
                # in one pass, the tensor is never written
                dw_stem = galloc(rec.wkey, wparam, zero=True)
                if ops.stem_bn_bwd_wgrad(rec.y, dz_a, sa, ca, rec.inp, coef[0], coef[1], coef[2], coef[3], c12[0], c12[1],
                                         ACT_RELU, dw_stem, inv_s):
                    emit(rec.wkey, dw_stem)
                    emit(rec.bnkey + ".weight", dgamma)
                    emit(rec.bnkey + ".bias", dbeta)
                    return None
            dy = empty(N, h, w, cout)
            if head is not None:
                ops.bn_act_bwd_apply_head(rec.y, head[0], head[1], coef[0], coef[1], coef[2], coef[3], c12[0], c12[1], ACT_RELU, dy)
            else:
                with ops.bn_bwd_form(ops.BN_BWD_SLIM if slim else ops.BN_BWD_NORMAL):
                    ops.bn_act_bwd_apply(rec.y, dz_a, sa, ca, dzp, coef[0], coef[1], coef[2], coef[3], c12[0], c12[1],
                                         ACT_RELU, True, dy)
            dinp = None
            if rec.inp_is_image:
                dw = dw_stem if dw_stem is not None else galloc(rec.wkey, wparam, zero=True)
                ops.conv_smallcin_wgrad(rec.inp, dy, dw, 3, 1, 1, inv_s)
                if need_dinp:
                    dinp = torch.empty_like(rec.inp)
                    ops.conv_smallcin_dgrad(dy, wparam.detach().contiguous(), dinp, 3, 1, 1, inv_s)
            elif getattr(rec, "wide", 0):
                # the image stage of a wide input: the weight gradient over the zero-padded channels, then the real ones
                dwp = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=dev)
                join_side()                                   # wg_ws on the main stream
                ops.conv3x3_wgrad_det(rec.inp, dy, wg_ws, dwp, N, h, w, cin, cout, inv_s)
                dw = galloc(rec.wkey, wparam)
                dw.copy_(dwp[:, :rec.wide])
                wgrad_on_side = False
                if need_dinp:
                    dxp = empty(N, h, w, cin)
                    ops.conv3x3(dy, rec.wd, dxp, N, h, w, cout, cin, ops.TAPS3_DGRAD)
                    dfull = torch.empty((N, cin, h, w), dtype=torch.float32, device=dev)
                    ops.nhwc_to_nchw(dxp, dfull, gscale=inv_s)
                    dinp = dfull[:, :rec.wide].contiguous()
            else:
                dw = galloc(rec.wkey, wparam)
                wgrad_on_side = rec.name in det_recs
                if not wgrad_on_side:
                    dwp = dw_take(wparam.numel())
                    if ops.USE_HALO_CONV and cin % 8 == 0 and cout % 8 == 0:
                        ops.conv3x3_wgrad(rec.inp, dy, dwp, N, h, w, cin, cout, in_stride=rec.inp_stride)
                    else:
                        ops.conv_wgrad(rec.geom, rec.inp, dy, dwp)
                    ops.unpack_wgrad(dwp, dw, cout, cin, 9, False, inv_s)
                if need_dinp:
                    dinp = empty(N, h, w, cin)
                    if ops.USE_HALO_CONV and rec.inp_stride is None and rec.train_stats and stream_conv(N, h, w, cout, cin):
                        # few pixels: the data gradient on the weight-streaming form too (its partial rows feed the fused bias gradient)
                        gd = ops.geom_conv_dgrad_s1(N, h, w, cin, cout, 3, 1)
                        if colsum is not None:
                            ops.conv_igemm(gd, dy, rec.wd, dinp, None, partials)
                            ops.bn_partials_colsum(partials, ops.conv_igemm_mtiles(gd), cin, colsum[0], colsum[1], inv_s, colsum[2])
                        else:
                            ops.conv_igemm(gd, dy, rec.wd, dinp)
                    elif ops.USE_HALO_CONV and colsum is not None:
                        ops.conv3x3(dy, rec.wd, dinp, N, h, w, cout, cin, ops.TAPS3_DGRAD, bn_partials=partials)
                        ops.bn_partials_colsum(partials, ops.conv3x3_stat_rows(N, h, w, cout, cin), cin, colsum[0], colsum[1], inv_s, colsum[2])
                    elif ops.USE_HALO_CONV:
                        ops.conv3x3(dy, rec.wd, dinp, N, h, w, cout, cin, ops.TAPS3_DGRAD)
                    else:
                        ops.conv_igemm(ops.geom_conv_dgrad_s1(N, h, w, cin, cout, 3, 1), dy, rec.wd, dinp)
                if wgrad_on_side:
                    # split-K parts in slabs + ordered reduction fused with scale / unpack: deterministic, no atomics.
                    # Behind the data gradient (see `side` above); the 64-cout LDS-DMA kernel (level 0) on the main stream
                    fam = ops.conv3x3_wgrad_family(w, cout)
                    on_side((rec.inp, dy, wg_ws, dw),
                            lambda: ops.conv3x3_wgrad_det(rec.inp, dy, wg_ws, dw, N, h, w, cin, cout, inv_s, in_stride=rec.inp_stride),
                            rec.wkey, dw, beside=fam != 1, leaves_96=True)
            if rec.inp_is_image or not wgrad_on_side:
                emit(rec.wkey, dw)
            emit(rec.bnkey + ".weight", dgamma)
            emit(rec.bnkey + ".bias", dbeta)
            return dinp

        # ---- decoder, reversed ----
        dcats = [None] * 4
        for j in range(4, 0, -1):
            lvl = 4 - j
            prefix = f"up{j}"
            cout_t = C[lvl]
            r3, r0 = recs[prefix + ".conv.3"], recs[prefix + ".conv.0"]
            dmid = conv_stage_bwd(r3, dz, r3.cout, 0, None, True, head=head_src if j == 4 else None)
            u = ups[prefix]
            # un-padded transposed convolution: its bias gradient is a column sum of d(concat) over every pixel, which the
            # data-gradient convolution writing d(concat) sums in its epilogue (no separate pass over the tensor)
            db_fused = None
            if (u.geom_bwd is not None and ops.USE_HALO_CONV and FUSED_UP_BIAS_GRAD and u.pt == 0 and u.pl == 0
                    and 2 * u.h == u.H2 and 2 * u.w == u.W2):
                db_fused = galloc(prefix + ".up.bias", params[prefix + ".up.bias"])
            dcat = conv_stage_bwd(r0, dmid, r0.cout, 0, None, True,
                                  colsum=None if db_fused is None else (cout_t, cout_t, db_fused))
            dcats[lvl] = dcat
            if u.geom_bwd is None:                                    # bilinear up-sampling: transposed interpolation
                dz = empty(N, u.h, u.w, u.cin)
                ops.upsample2x_bilinear_bwd(dcat, dz, N, u.h, u.w, u.cin, u.H2, u.W2, dy_stride=2 * cout_t,
                                            dy_coff=cout_t, ooy=u.pt, oox=u.pl)
                continue
            wkey = prefix + ".up.weight"
            wparam = params[wkey]
            if db_fused is not None:
                db = db_fused
            else:
                db = galloc(prefix + ".up.bias", params[prefix + ".up.bias"])
                ops.colsum(dcat, 2 * cout_t, cout_t, N, u.H2, u.W2, u.pt, u.pl, 2 * u.h, 2 * u.w, cout_t, inv_s, col_ws, db)
            dw = galloc(wkey, wparam)
            dz = empty(N, u.h, u.w, u.cin)
            ops.upconv2x2_dgrad(u.geom_bwd, dcat, u.wd, dz, N, u.h, u.w, u.cin, u.cout, u.H2, u.W2, 2 * cout_t, cout_t, u.pt, u.pl)
            # K = pixels pointwise GEMM on LDS-DMA operands (csrc/upwgrad.hip); the generic engine for shapes outside it.
            # u.zin: the layer's input -- dense, or the hi plane of a pair buffer (pixel stride = its last dimension).
            # Behind the data gradient like the 3x3 ones; its 112-register waves leave room for the normal BatchNorm forms
            on_side((dcat, u.zin, wg_ws, dw),
                    lambda u=u, dcat=dcat, dw=dw: ops.upconv2x2_wgrad_det(
                        u.geom_wg if u.geom_wg is not None else u.geom_bwd, u.zin, dcat, wg_ws, dw, N, u.h, u.w, u.cin, u.cout,
                        u.H2, u.W2, u.zin.shape[3], 2 * u.cout, u.cout, u.pt, u.pl, inv_s),
                    wkey, dw)
            emit(prefix + ".up.bias", db)

        # ---- encoder, reversed ----
        dx = None
        dpool = None
        for i in range(4, -1, -1):
            prefix = "inc" if i == 0 else f"down{i}.maxpool_conv.1"
            if i == 4:
                dmid = conv_stage_bwd(recs[prefix + ".3"], dz, C[i], 0, None, True)
            else:
                dmid = conv_stage_bwd(recs[prefix + ".3"], dcats[i], 2 * C[i], 0, dpool, True)
            r0 = recs[prefix + ".0"]
            dinp = conv_stage_bwd(r0, dmid, C[i], 0, None, (i > 0) or need_dx)
            if i > 0:
                dpool = dinp
            else:
                dx = dinp
        if side is not None:
            flush_deferred(True)
            main_stream.wait_stream(side)          # every weight gradient is complete before anything downstream reads it
        if renorm is not None:
            inv_r = torch.reciprocal(renorm)
            torch._foreach_mul_(list(grads.values()), inv_r)
            if dx is not None:
                dx = dx * inv_r
        if self.after_backward is not None:
            self.after_backward()
        return grads, dx


class _UNetFunction(torch.autograd.Function):
    """autograd bridge: (x, *params) -> logits."""

    @staticmethod
    def forward(ctx, engine: UNetEngine, names, training: bool, need_grad: bool, x, *plist):
        params = dict(zip(names, plist))
        logits, ectx = engine.forward(x, params, training, need_grad)
        ctx.engine, ctx.names, ctx.ectx, ctx.plist = engine, names, ectx, plist
        ctx.x_needs_grad = x.requires_grad
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        if ctx.ectx is None:
            raise RuntimeError("UNet forward ran without gradient tracking")
        params = dict(zip(ctx.names, ctx.plist))
        grads, dx = ctx.engine.backward(ctx.ectx, params, dlogits, ctx.x_needs_grad)
        # with a GradReducer attached autograd receives the REDUCED gradients, as copies (fetch): a stolen bucket view would
        # be overwritten (not accumulated) by the next backward
        fetch, alias = ctx.engine.grad_fetch, ctx.engine.grad_alloc is not None
        out = [(fetch(n) if fetch is not None else (grads[n].clone() if alias else grads[n])) if (p.requires_grad and n in grads)
               else None for n, p in zip(ctx.names, ctx.plist)]
        if ctx.engine.accumulate_grads and fetch is None and not alias:
            have, new = [], []
            for i, p in enumerate(ctx.plist):
                if out[i] is not None and p.grad is not None and p.grad.shape == out[i].shape and p.grad.dtype == out[i].dtype:
                    have.append(p.grad)
                    new.append(out[i])
                    out[i] = None
            if have:
                torch._foreach_add_(have, new)
        return (None, None, None, None, dx if ctx.x_needs_grad else None, *out)


def run_unet_labels(engine: UNetEngine, x: torch.Tensor) -> torch.Tensor:
    """UNet.predict: the forward without a graph, ending in the label map (uint8 [N,H,W])"""
    with torch.no_grad():
        return engine.forward(x, dict(engine.param_items()), engine.net.training, False, labels=True)[0]


def run_unet(engine: UNetEngine, x: torch.Tensor) -> torch.Tensor:
    items = engine.param_items()
    names = tuple(n for n, _ in items)
    plist = tuple(p for _, p in items)
    # grad mode is always off inside Function.forward: decide here whether to keep activations
    need_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in plist))
    return _UNetFunction.apply(engine, names, engine.net.training, need_grad, x, *plist)
