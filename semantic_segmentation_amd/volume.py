"""Volumes of any size in front of and behind UNet3D, on the device.

The reference never hands its 3-D network a raw scan: every item goes through GenSeg-3D/transforms.py on the host -- three
RandomFlip(0.5) (:33-44), NormalizeIntensity over the non-zero voxels (:22-30), PadToDivisible(k=16) (:47-60), composed in that
order (:69-76; validation without the flips, :90-94) -- and its scripts score torch.argmax(logits, 1) against the padded mask
(GenSeg-3D/train_unet.py:37-51, 56-78).  `VolumePrep` is that transform as two launches (statistics, then flip + normalise + pad of
image and mask in one kernel), `restore` its inverse geometry on a label map, `label_dice` the Dice of train_unet.py:37-51 with the
arg-max already taken by `UNet3D.predict`, `evaluate_volumes` the loop of :56-78.

Reference quirks kept: the statistics run over `image != 0` (IEEE compare) of ALL channels of an item together, the std is the
unbiased one, 1e-5 is added to the std (not to the variance), padding goes to the far end only and is applied AFTER normalising
(pad voxels are 0, not (0 - mean) / std), an item with fewer than two non-zero voxels normalises to NaN, and the Dice multiplies
and sums the class indices as numbers.  Nothing here synchronises with the host; there is no CPU path."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .ops import _stream


@dataclass
class VolumeMeta:
    """What `restore` needs: the item's own shape, its padded shape, and the device tensors the kernels read."""
    shape: Tuple[int, int, int, int, int]            # (N, C, D, H, W) of the image as given (batch / channel axes added)
    padded: Tuple[int, int, int]                     # (Dp, Hp, Wp)
    flips: Optional[torch.Tensor]                    # int32 [N] on the device (bit 0: D, 1: H, 2: W) or None
    stats: Optional[torch.Tensor]                    # fp64 [N, 4] = count, mean, std, 1 / (std + 1e-5), or None
    ndim: int                                        # rank of the image as given (3, 4 or 5)


def _need_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what} runs on the MI355X only (no CPU path)")


def _as_u8(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype == torch.uint8:
        return t.contiguous()
    if t.dtype.is_floating_point or t.dtype == torch.bool or t.is_complex():
        raise TypeError(f"{what} must be uint8 or integer class indices, got {t.dtype}")
    return t.to(torch.uint8).contiguous()


def pad_up(n: int, k: int) -> int:
    return (n + k - 1) // k * k


def volume_stats(image: torch.Tensor) -> torch.Tensor:
    """fp64 [N, 4] = {count, mean, std, 1 / (std + 1e-5)} over the non-zero voxels of each item of an fp32 [N, ...] tensor."""
    _need_gpu(image, "volume_stats")
    if image.dtype != torch.float32 or image.dim() < 2:
        raise TypeError(f"volume_stats: expected fp32 [N, ...], got {image.dtype} {tuple(image.shape)}")
    image = image.contiguous()
    n = image.shape[0]
    lib = _lib.load()
    ws = torch.empty(lib.gs_volume_stats_ws_doubles(n), dtype=torch.float64, device=image.device)
    stats = torch.empty(n, 4, dtype=torch.float64, device=image.device)
    _lib.call("gs_volume_nonzero_stats", image.data_ptr(), n, image.numel() // n, ws.data_ptr(), stats.data_ptr(), _stream())
    return stats


class VolumePrep:
    """transforms.py's item transform on the device.  k: pad every spatial dim up to a multiple of it (a positive multiple of 8;
    16 is the reference's, 8 what UNet3D needs); normalize=False skips NormalizeIntensity; flip_prob: probability of each of the
    three flips when `prepare` is not given any (0.5 = train_transform, 0.0 = val_transform), drawn on the host from
    np.random.default_rng(seed)."""

    def __init__(self, k: int = 16, normalize: bool = True, flip_prob: float = 0.0, seed: int = 0):
        if int(k) != k or k <= 0 or k % 8:
            raise ValueError(f"VolumePrep: k={k} must be a positive multiple of 8")
        if not 0.0 <= flip_prob <= 1.0:
            raise ValueError(f"VolumePrep: flip_prob={flip_prob} must be in [0, 1]")
        self.k, self.normalize, self.flip_prob = int(k), bool(normalize), float(flip_prob)
        self.rng = np.random.default_rng(seed)

    def draw_flips(self, n: int) -> np.ndarray:
        """int32 [n] bitmasks: three independent draws per item, in the order of transforms.py:71-73 (D, H, W)"""
        hit = self.rng.random((n, 3)) < self.flip_prob
        return (hit * np.array([1, 2, 4])).sum(1).astype(np.int32)

    def _flips(self, flips, n: int, device) -> Optional[torch.Tensor]:
        if flips is False:
            return None
        if flips is None:
            if self.flip_prob == 0.0:
                return None
            flips = self.draw_flips(n)
        if isinstance(flips, torch.Tensor):
            if flips.device != device or flips.dtype != torch.int32:
                flips = flips.to(device=device, dtype=torch.int32)
            flips = flips.contiguous()
        else:
            host = np.ascontiguousarray(np.asarray(flips, dtype=np.int32).reshape(-1))
            if host.size and (host.min() < 0 or host.max() > 7):
                raise ValueError("VolumePrep: a flip mask has bits 0..2 only")
            flips = torch.from_numpy(host).to(device)
        if tuple(flips.shape) != (n,):
            raise ValueError(f"VolumePrep: flips must hold one bitmask per item ({n}), got {tuple(flips.shape)}")
        return flips

    def prepare(self, image: torch.Tensor, mask: Optional[torch.Tensor] = None, flips=None):
        """-> (fp32 [N, C, Dp, Hp, Wp], uint8 [N, Dp, Hp, Wp] or None, VolumeMeta).  image: fp32 [D,H,W], [C,D,H,W] or
        [N,C,D,H,W] on the GPU; mask: uint8 / integer class indices [N,D,H,W] or [N,1,D,H,W] (or one item without the batch axis);
        flips: one bitmask per item (bit 0: D, 1: H, 2: W) as a sequence or a device int32 tensor; None draws them with flip_prob,
        False means none whatever flip_prob is (validation)."""
        _need_gpu(image, "VolumePrep")
        if image.dtype != torch.float32:
            raise TypeError(f"VolumePrep: the image must be fp32, got {image.dtype}")
        ndim = image.dim()
        if ndim not in (3, 4, 5):
            raise ValueError(f"VolumePrep: expected [D,H,W], [C,D,H,W] or [N,C,D,H,W], got {tuple(image.shape)}")
        x = image.reshape((1,) * (5 - ndim) + tuple(image.shape)).contiguous()
        n, c, d, h, w = x.shape
        dp, hp, wp = pad_up(d, self.k), pad_up(h, self.k), pad_up(w, self.k)
        m = None
        if mask is not None:
            _need_gpu(mask, "VolumePrep")
            m = _as_u8(mask, "VolumePrep: the mask")
            if m.numel() != n * d * h * w or tuple(m.shape[-3:]) != (d, h, w):
                raise ValueError(f"VolumePrep: mask {tuple(mask.shape)} does not match the image {tuple(image.shape)}")
            m = m.reshape(n, d, h, w)
        fl = self._flips(flips, n, x.device)
        stats = volume_stats(x) if self.normalize else None
        out = torch.empty(n, c, dp, hp, wp, dtype=torch.float32, device=x.device)
        mout = torch.empty(n, dp, hp, wp, dtype=torch.uint8, device=x.device) if m is not None else None
        _lib.call("gs_volume_prepare", x.data_ptr(), m.data_ptr() if m is not None else None,
                  stats.data_ptr() if stats is not None else None, fl.data_ptr() if fl is not None else None, out.data_ptr(),
                  mout.data_ptr() if mout is not None else None, n, c, d, h, w, dp, hp, wp, _stream())
        return out, mout, VolumeMeta((n, c, d, h, w), (dp, hp, wp), fl, stats, ndim)

    def restore(self, labels: torch.Tensor, meta: VolumeMeta) -> torch.Tensor:
        """uint8 label map [N, Dp, Hp, Wp] of a prepared batch -> uint8 [N, D, H, W] in the item's own extent and orientation"""
        _need_gpu(labels, "VolumePrep")
        n, _, d, h, w = meta.shape
        dp, hp, wp = meta.padded
        if labels.dtype != torch.uint8 or tuple(labels.shape) != (n, dp, hp, wp):
            raise ValueError(f"VolumePrep.restore: expected uint8 {(n, dp, hp, wp)}, got {labels.dtype} {tuple(labels.shape)}")
        labels = labels.contiguous()
        if labels.data_ptr() % 16:
            labels = labels.clone()
        out = torch.empty(n, d, h, w, dtype=torch.uint8, device=labels.device)
        _lib.call("gs_volume_restore_labels", labels.data_ptr(), meta.flips.data_ptr() if meta.flips is not None else None,
                  out.data_ptr(), n, d, h, w, dp, hp, wp, _stream())
        return out


def label_sums(pred: torch.Tensor, target: torch.Tensor, eps: float = 1e-6):
    """-> (int64 [N, 3] = sum p t, sum p, sum t per item; 0-dim fp32 Dice over the batch).  pred / target: label maps [N, ...]."""
    _need_gpu(pred, "label_sums")
    _need_gpu(target, "label_sums")
    p, t = _as_u8(pred, "label_sums: pred"), _as_u8(target, "label_sums: target")
    if p.dim() < 2 or p.numel() != t.numel() or p.shape[0] != t.shape[0]:
        raise ValueError(f"label_sums: pred {tuple(pred.shape)} and target {tuple(target.shape)} do not match")
    if (p.data_ptr() - t.data_ptr()) % 16:
        p, t = p.clone(), t.clone()                    # fresh allocations share their alignment
    n = p.shape[0]
    lib = _lib.load()
    ws = torch.empty(lib.gs_label_sums_ws_int64(n), dtype=torch.int64, device=p.device)
    sums = torch.empty(n, 3, dtype=torch.int64, device=p.device)
    dice = torch.empty((), dtype=torch.float32, device=p.device)
    _lib.call("gs_label_sums", p.data_ptr(), t.data_ptr(), n, p.numel() // n, ws.data_ptr(), sums.data_ptr(), dice.data_ptr(),
              float(eps), _stream())
    return sums, dice


def label_dice(pred_u8: torch.Tensor, target: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """dice_score of GenSeg-3D/train_unet.py:37-51 on a label map (the arg-max of :39 already taken by UNet3D.predict):
    (2 sum(p t) + eps) / (sum p + sum t + eps), integer sums over the whole batch, the quotient in fp64 -> 0-dim fp32 on the device."""
    return label_sums(pred_u8, target, eps)[1]


def evaluate_volumes(net, batches, prep: Optional[VolumePrep] = None, crop: bool = False) -> float:
    """evaluate() of GenSeg-3D/train_unet.py:56-78 over raw (image, mask) pairs: eval mode (and back to the mode found), prepare,
    predict, label_dice, mean over the batches; ONE host sync, at the end.  crop=False scores the padded extent as the reference
    does (its masks are padded by the same transform); crop=True scores the scan's own voxels only."""
    prep = prep if prep is not None else VolumePrep()
    was_training = net.training
    net.eval()
    scores = []
    try:
        for image, mask in batches:
            x, m, meta = prep.prepare(image, mask, flips=False)
            labels = net.predict(x)
            if crop:
                n, _, d, h, w = meta.shape
                scores.append(label_dice(prep.restore(labels, meta), _as_u8(mask, "evaluate_volumes: the mask").reshape(n, d, h, w)))
            else:
                scores.append(label_dice(labels, m))
    finally:
        net.train(was_training)
    if not scores:
        return 0.0
    return float(torch.stack(scores).double().mean().item())
