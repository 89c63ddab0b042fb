"""Tensor-level wrappers over the C ABI (include/gsseg.h).  Shapes/dtypes are validated HERE, before
any launch, so failures are synchronous Python exceptions.  torch supplies device memory and the
current HIP stream only; all arithmetic happens in libgsseg_hip.so."""
from __future__ import annotations

import collections
import contextlib
import ctypes
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import ACT_NONE, GS_BF16, GS_F16, GsConvGeom

DTYPES = {"f16": (GS_F16, torch.float16), "bf16": (GS_BF16, torch.bfloat16)}


def dt_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float16:
        return GS_F16
    if t.dtype == torch.bfloat16:
        return GS_BF16
    raise TypeError(f"expected a float16/bfloat16 tensor, got {t.dtype}")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_RAW_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """Handle of torch's current HIP stream on the current device.  torch.cuda.current_stream() builds a Stream object
    (~9 us per call, a third of the host time of a small-batch step); the raw accessors return the same handle."""
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return _RAW_STREAM(_RAW_DEVICE())
    return torch.cuda.current_stream().cuda_stream


_TAP_ARRAYS = {}


def _tap_arrays(taps):
    """(dy, dx) int32[9] ctypes arrays of a 3x3 tap list, built once per list (2.2 us per call otherwise: ~50 conv launches per
    U-Net pass at the script's batch 2, where the host bounds the step)."""
    key = tuple(taps)
    r = _TAP_ARRAYS.get(key)
    if r is None:
        r = _TAP_ARRAYS[key] = ((ctypes.c_int32 * 9)(*[t[0] for t in key]), (ctypes.c_int32 * 9)(*[t[1] for t in key]))
    return r


_TAPS3D = {sgn: ((ctypes.c_int32 * 3)(*[sgn * (k - 1) for k in range(3)]), (ctypes.c_int32 * 9)(*[sgn * (k // 3 - 1) for k in range(9)]),
                 (ctypes.c_int32 * 9)(*[sgn * (k % 3 - 1) for k in range(9)])) for sgn in (1, -1)}


def _dev(t: torch.Tensor):
    if not t.is_cuda:
        raise RuntimeError("semantic_segmentation_amd ops need tensors on the MI355X (cuda) device; "
                           "there is no CPU path")
    # launches go to the CURRENT device's current stream: a tensor of another device would be dereferenced there
    cur = _RAW_DEVICE() if _RAW_DEVICE is not None else torch.cuda.current_device()
    if t.device.index != cur:
        raise RuntimeError(f"tensor on cuda:{t.device.index} but the current device is cuda:{cur}: one process per GPU "
                           "-- call torch.cuda.set_device (or run under torch.cuda.device(t.device))")


def _f32(t: Optional[torch.Tensor], name: str):
    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
        raise TypeError(f"{name} must be a contiguous float32 tensor")


# ---------------------------------------------------------------------------- geometry builders
def make_geom(N, IH, IW, Cin, OHg, OWg, Cout, OH, OW, taps: Sequence[Tuple[int, int]], isy=1, isx=1,
              osy=1, osx=1, ooy=0, oox=0, in_stride=None, in_coff=0, out_stride=None, out_coff=0,
              tap_w: Optional[Sequence[int]] = None, Dg=1, Din=1, Dout=1, isz=1, osz=1, ooz=0,
              tap_dz: Optional[Sequence[int]] = None) -> GsConvGeom:
    g = GsConvGeom()
    g.N, g.IH, g.IW, g.Cin = N, IH, IW, Cin
    g.in_pix_stride = Cin if in_stride is None else in_stride
    g.in_coff = in_coff
    g.OHg, g.OWg, g.Cout, g.OH, g.OW = OHg, OWg, Cout, OH, OW
    g.out_pix_stride = Cout if out_stride is None else out_stride
    g.out_coff = out_coff
    g.isy, g.isx, g.osy, g.osx, g.ooy, g.oox = isy, isx, osy, osx, ooy, oox
    if not 0 < len(taps) <= _lib.GS_MAX_TAPS:
        raise ValueError(f"{len(taps)} taps out of range")
    g.ntaps = len(taps)
    for i, (dy, dx) in enumerate(taps):
        g.tap_dy[i], g.tap_dx[i] = dy, dx
        g.tap_w[i] = i if tap_w is None else tap_w[i]
        g.tap_dz[i] = 0 if tap_dz is None else tap_dz[i]
    g.Dg, g.Din, g.Dout, g.isz, g.osz, g.ooz = Dg, Din, Dout, isz, osz, ooz
    return g


def conv_out_size(i: int, k: int, s: int, p: int) -> int:
    return (i + 2 * p - k) // s + 1


def geom_conv(N, IH, IW, Cin, Cout, k, stride, pad, **kw) -> GsConvGeom:
    """nn.Conv2d(k, stride, pad): taps in (ky,kx) row-major order, weights [k*k][Cout][Cin]."""
    OH, OW = conv_out_size(IH, k, stride, pad), conv_out_size(IW, k, stride, pad)
    taps = [(ky - pad, kx - pad) for ky in range(k) for kx in range(k)]
    return make_geom(N, IH, IW, Cin, OH, OW, Cout, OH, OW, taps, isy=stride, isx=stride, **kw)


def geom_conv_dgrad_s1(N, IH, IW, Cin, Cout, k, pad, **kw) -> GsConvGeom:
    """Data gradient of a stride-1 Conv2d as a convolution over dy: dx[i] = sum_t dy[i + pad - k_t] Wd[t].
    'Input' of this launch is dy [N,OH,OW,Cout]; 'output' is dx [N,IH,IW,Cin]; weights [k*k][Cin][Cout]."""
    OH, OW = conv_out_size(IH, k, 1, pad), conv_out_size(IW, k, 1, pad)
    taps = [(pad - ky, pad - kx) for ky in range(k) for kx in range(k)]
    return make_geom(N, OH, OW, Cout, IH, IW, Cin, IH, IW, taps, **kw)


# ---------------------------------------------------------------------------- per-launch timing
class KernelTimer:
    """Brackets selected launches with HIP events on the launch stream (torch's current stream, which is
    the stream handed to the C ABI) and accumulates algorithmic work per kernel class.  Used by bench.py
    for the roofline figures; off by default (TIMER is None)."""

    def __init__(self, pool: int = 0):
        self.records = []          # (kind, flops, bytes, ev0, ev1)
        # events created (and recorded once, which is what really creates the HIP event) up front, so that the timed
        # region of a benchmark does not contain thousands of hipEventCreate calls
        self._pool = [torch.cuda.Event(enable_timing=True) for _ in range(pool)]
        for ev in self._pool:
            ev.record()
        if pool:
            torch.cuda.synchronize()

    def _event(self):
        return self._pool.pop() if self._pool else torch.cuda.Event(enable_timing=True)

    def start(self):
        ev = self._event()
        ev.record()
        return ev

    def stop(self, kind, ev0, flops=0.0, nbytes=0.0):
        ev1 = self._event()
        ev1.record()
        self.records.append((kind, float(flops), float(nbytes), ev0, ev1))

    def reset(self):
        """forget the launches bracketed so far (warm-up steps run with the timer attached); the pool keeps its unused events"""
        self.records = []

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kind, fl, nb, e0, e1 in self.records:
            d = out.setdefault(kind, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += nb
        return out


TIMER: Optional[KernelTimer] = None


def _geom_flops(g: GsConvGeom) -> float:
    return 2.0 * g.N * g.Dg * g.OHg * g.OWg * g.Cout * g.ntaps * g.Cin


def _geom_bytes(g: GsConvGeom, wgrad: bool = False) -> float:
    """algorithmic HBM bytes of one implicit-GEMM launch: the input tensor once, the output once, the weights once (fp32 for a
    weight gradient)"""
    inp = 2.0 * g.N * g.Din * g.IH * g.IW * g.Cin
    out = 2.0 * g.N * g.Dg * g.OHg * g.OWg * g.Cout
    return inp + out + (4.0 if wgrad else 2.0) * g.ntaps * g.Cin * g.Cout


def geom_convT_class(N, IH, IW, Cin, Cout, k, pad, py, px, OH=None, OW=None, **kw) -> GsConvGeom:
    """Sub-pixel class (py,px) of ConvTranspose2d(k, stride 2, pad): output pixels (2i+py, 2j+px) <- input
    (i+dy, j+dx) for the taps with ky == py+pad (mod 2); weight slots index a [k*k][Cout][Cin] pack."""
    kys = [ky for ky in range(k) if (py + pad - ky) % 2 == 0]
    kxs = [kx for kx in range(k) if (px + pad - kx) % 2 == 0]
    taps = [((py + pad - ky) // 2, (px + pad - kx) // 2) for ky in kys for kx in kxs]
    slots = [ky * k + kx for ky in kys for kx in kxs]
    OHf = (IH - 1) * 2 - 2 * pad + k if OH is None else OH
    OWf = (IW - 1) * 2 - 2 * pad + k if OW is None else OW
    ohg, owg = (OHf - py + 1) // 2, (OWf - px + 1) // 2
    return make_geom(N, IH, IW, Cin, ohg, owg, Cout, OHf, OWf, taps, osy=2, osx=2, ooy=py, oox=px, tap_w=slots, **kw)


def geom_conv_s2_dgrad_class(N, IH, IW, Cin, Cout, k, pad, py, px, **kw) -> GsConvGeom:
    """Data gradient of Conv2d(k, stride 2, pad) for input pixels (2i+py, 2j+px): reads dy [N,OH,OW,Cout] at
    (i + (py+pad-ky)/2, ...) for ky == py+pad (mod 2); weight slots index the [k*k][Cin][Cout] dgrad pack."""
    OH, OW = conv_out_size(IH, k, 2, pad), conv_out_size(IW, k, 2, pad)
    kys = [ky for ky in range(k) if (py + pad - ky) % 2 == 0]
    kxs = [kx for kx in range(k) if (px + pad - kx) % 2 == 0]
    taps = [((py + pad - ky) // 2, (px + pad - kx) // 2) for ky in kys for kx in kxs]
    slots = [ky * k + kx for ky in kys for kx in kxs]
    ihg, iwg = (IH - py + 1) // 2, (IW - px + 1) // 2
    return make_geom(N, OH, OW, Cout, ihg, iwg, Cin, IH, IW, taps, osy=2, osx=2, ooy=py, oox=px, tap_w=slots, **kw)


# Conv3d on depth-slice stacks [N*D,H,W,C]: the 2-D builders with a depth axis (GsConvGeom.Dg / Din / Dout / isz / osz / ooz / tap_dz).
# Weight slot of tap (kz,ky,kx) = (kz*k + ky)*k + kx: a [Cout][Cin][k][k][k] tensor VIEWED as [Cout][Cin][k*k][k] goes through
# pack_weight / conv_wgrad_det unchanged (they see k*k*k taps in the tensor's own order) -- conv3d_weight_view().
def conv3d_weight_view(w: torch.Tensor) -> torch.Tensor:
    """[A][B][k][k][k] -> the 4-D view [A][B][k*k][k] pack_weight takes (same memory, slot (kz*k + ky)*k + kx)"""
    if w.dim() != 5 or not w.is_contiguous():
        raise ValueError("conv3d_weight_view: a contiguous 5-D weight")
    A, B, k = w.shape[0], w.shape[1], w.shape[2]
    return w.view(A, B, k * k, k)


def _taps3d(k):
    return [(kz, ky, kx) for kz in range(k) for ky in range(k) for kx in range(k)]


def geom_conv3d(N, D, IH, IW, Cin, Cout, k, stride, pad, **kw) -> GsConvGeom:
    """nn.Conv3d(k, stride, pad) on x [N*D,IH,IW,Cin] -> y [N*OD,OH,OW,Cout]: taps in (kz,ky,kx) row-major order, weights
    [k*k*k][Cout][Cin]; k*k*k <= 64 taps (k <= 4)."""
    OD, OH, OW = conv_out_size(D, k, stride, pad), conv_out_size(IH, k, stride, pad), conv_out_size(IW, k, stride, pad)
    t3 = _taps3d(k)
    return make_geom(N, IH, IW, Cin, OH, OW, Cout, OH, OW, [(ky - pad, kx - pad) for (_, ky, kx) in t3], isy=stride, isx=stride,
                     tap_dz=[kz - pad for (kz, _, _) in t3], Dg=OD, Din=D, Dout=OD, isz=stride, **kw)


def geom_conv3d_dgrad_s1(N, D, IH, IW, Cin, Cout, k, pad, **kw) -> GsConvGeom:
    """Data gradient of a stride-1 Conv3d as a convolution over dy: dx[i] = sum_t dy[i + pad - k_t] Wd[t], every axis alike.
    'Input' of this launch is dy [N*OD,OH,OW,Cout]; 'output' is dx [N*D,IH,IW,Cin]; weights [k*k*k][Cin][Cout]."""
    OD, OH, OW = conv_out_size(D, k, 1, pad), conv_out_size(IH, k, 1, pad), conv_out_size(IW, k, 1, pad)
    t3 = _taps3d(k)
    return make_geom(N, OH, OW, Cout, IH, IW, Cin, IH, IW, [(pad - ky, pad - kx) for (_, ky, kx) in t3],
                     tap_dz=[pad - kz for (kz, _, _) in t3], Dg=D, Din=OD, Dout=D, **kw)


def geom_conv3d_s2_dgrad_class(N, D, IH, IW, Cin, Cout, k, pad, pz, py, px, **kw) -> GsConvGeom:
    """Data gradient of Conv3d(k, stride 2, pad) for input voxels (2a+pz, 2i+py, 2j+px): reads dy [N*OD,OH,OW,Cout] at
    (a + (pz+pad-kz)/2, ...) for kz == pz+pad (mod 2), rows and columns alike: (k/2)^3 taps of the [k*k*k][Cin][Cout] dgrad pack."""
    OD, OH, OW = conv_out_size(D, k, 2, pad), conv_out_size(IH, k, 2, pad), conv_out_size(IW, k, 2, pad)
    sel = [(kz, ky, kx) for (kz, ky, kx) in _taps3d(k)
           if (pz + pad - kz) % 2 == 0 and (py + pad - ky) % 2 == 0 and (px + pad - kx) % 2 == 0]
    taps = [((py + pad - ky) // 2, (px + pad - kx) // 2) for (_, ky, kx) in sel]
    dz = [(pz + pad - kz) // 2 for (kz, _, _) in sel]
    slots = [(kz * k + ky) * k + kx for (kz, ky, kx) in sel]
    dg, ihg, iwg = (D - pz + 1) // 2, (IH - py + 1) // 2, (IW - px + 1) // 2
    return make_geom(N, OH, OW, Cout, ihg, iwg, Cin, IH, IW, taps, osy=2, osx=2, ooy=py, oox=px, tap_w=slots, tap_dz=dz,
                     Dg=dg, Din=OD, Dout=D, osz=2, ooz=pz, **kw)


# ---------------------------------------------------------------------------- MFMA engine
_SPLITK_WS = collections.OrderedDict()      # (device index, stream handle) -> zeroed fp32 workspace, least recently used first
_SPLITK_WS_MAX = int(os.environ.get("GSSEG_SPLITK_WS_MAX", "3"))
_SPLITK_PINNED = set()                      # keys baked into a captured graph: never evicted


def _splitk_workspace(device: torch.device, stream) -> Optional[torch.Tensor]:
    """gs_conv_igemm's split-K workspace (134 MB), passed with every call: one per (device, stream), because launches that
    share one must be ordered on one stream (ticket counters and slabs are reused); allocated zeroed once, the kernels
    leave the counters zeroed.  At most GSSEG_SPLITK_WS_MAX (3) un-pinned ones are kept: a process that runs the engine on many
    streams (or whose stream handles torch recycles) evicts the least recently used one -- it was allocated and used on its own
    stream only, so handing it back to torch's stream-ordered allocator is safe -- instead of pinning 134 MB per handle.
    Stream capture: a workspace handed to a capturing stream is baked into the graph, so it is PINNED (never evicted) from
    then on, and it must exist BEFORE the capture starts (allocating it here would put the buffer into the graph's pool and its
    zero fill into the graph, while this cache would go on handing the pointer to eager code): graphs.capture_step and
    harness.EndToEndTrainer create it first; anything else that captures engine code calls ops.splitk_workspace_for_capture()."""
    if os.environ.get("GSSEG_SPLITK", "1") == "0":
        return None
    key = (device.index, int(stream or 0))
    capturing = torch.cuda.is_current_stream_capturing()
    ws = _SPLITK_WS.get(key)
    if ws is None:
        if capturing:
            raise RuntimeError("the split-K workspace of this stream does not exist yet and cannot be created during a stream capture: "
                               "call semantic_segmentation_amd.ops.splitk_workspace_for_capture() on the capture stream before capturing")
        n = int(_lib.load().gs_conv_igemm_workspace_floats())
        ws = torch.zeros(n, dtype=torch.float32, device=device)     # zero fill runs on this same (current) stream
        _SPLITK_WS[key] = ws
        evictable = [k for k in _SPLITK_WS if k not in _SPLITK_PINNED and k != key]
        while len(evictable) + 1 > max(1, _SPLITK_WS_MAX) and evictable:
            _SPLITK_WS.pop(evictable.pop(0))
    else:
        _SPLITK_WS.move_to_end(key)
    if capturing:
        _SPLITK_PINNED.add(key)
    return ws


def splitk_workspace_for_capture(device: Optional[torch.device] = None) -> Optional[torch.Tensor]:
    """Create (eagerly) and pin the split-K workspace of the CURRENT stream: call on the capture stream before a stream capture of
    engine code (a hipGraph bakes the pointer in; see _splitk_workspace)."""
    device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    stream = _stream()
    ws = _splitk_workspace(device, stream)
    if ws is not None:
        _SPLITK_PINNED.add((device.index, int(stream or 0)))
    return ws


def conv_igemm(g: GsConvGeom, x, w, y, bias=None, bn_partials=None, act=ACT_NONE):
    _dev(x)
    _f32(bias, "bias"); _f32(bn_partials, "bn_partials")
    if not (x.dtype == w.dtype == y.dtype):
        raise TypeError("conv_igemm: x, w, y must share one 16-bit dtype")
    if bn_partials is not None:
        need = _lib.load().gs_bn_partials_floats(conv_igemm_mtiles(g), g.Cout)
        if bn_partials.numel() < need:
            raise ValueError(f"bn_partials too small: {bn_partials.numel()} < {need}")
    stream = _stream()
    ws = _splitk_workspace(x.device, stream)
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv_igemm", g, _p(x), _p(w), _p(y), _p(bias), _p(bn_partials), act, dt_code(x), _p(ws),
              ws.numel() if ws is not None else 0, stream)
    if ev is not None:
        TIMER.stop("igemm_fwd", ev, _geom_flops(g), _geom_bytes(g))


# taps of a 3x3/pad-1 conv in weight order, and the flipped list that turns the same kernel into its dgrad
def conv_igemm_batch(geoms, x, ws_list, y, bias=None, bn_partials=None, act=ACT_NONE):
    """Up to four GEMMs (the sub-pixel classes of one layer) over the same x / y / bias in ONE launch: geoms[i] with weights
    ws_list[i] and optional BatchNorm partials bn_partials[i].  At the script's batch size (2) a class launch fills a
    fraction of the chip; together the classes fill it and pay one launch gap."""
    _dev(x)
    _f32(bias, "bias")
    n = len(geoms)
    if not 1 <= n <= 4 or len(ws_list) != n or (bn_partials is not None and len(bn_partials) != n):
        raise ValueError("conv_igemm_batch: 1..4 GEMMs with one weight tensor (and optionally one partials tensor) each")
    if any(w.dtype != x.dtype for w in ws_list) or y.dtype != x.dtype:
        raise TypeError("conv_igemm_batch: x, w, y must share one 16-bit dtype")
    if bn_partials is not None:
        for g, p in zip(geoms, bn_partials):
            _f32(p, "bn_partials")
            if p.numel() < _lib.load().gs_bn_partials_floats(conv_igemm_mtiles(g), g.Cout):
                raise ValueError("conv_igemm_batch: bn_partials too small")
    garr = (ctypes.POINTER(GsConvGeom) * n)(*[ctypes.pointer(g) for g in geoms])
    warr = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws_list])
    parr = (ctypes.c_void_p * n)(*[p.data_ptr() for p in bn_partials]) if bn_partials is not None else None
    stream = _stream()
    ws = _splitk_workspace(x.device, stream)
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv_igemm_batch", n, garr, _p(x), warr, _p(y), _p(bias), parr, act, dt_code(x), _p(ws),
              ws.numel() if ws is not None else 0, stream)
    if ev is not None:
        TIMER.stop("igemm_fwd", ev, sum(_geom_flops(g) for g in geoms), sum(_geom_bytes(g) for g in geoms))


TAPS3_FWD = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]
TAPS3_DGRAD = [(1 - ky, 1 - kx) for ky in range(3) for kx in range(3)]
USE_HALO_CONV = os.environ.get("GSSEG_CONV3X3", "halo") != "generic"


def conv3x3_mtiles(N, H, W, Cout) -> int:
    return _lib.load().gs_conv3x3_mtiles(N, H, W, Cout)


def conv3x3_stat_rows(N, H, W, Cin, Cout, pair=False) -> int:
    """Rows of BatchNorm partial sums a conv3x3 launch of these dimensions WRITES (what bn_finalize / bn_partials_colsum must
    be told): one per block and cout-tile group on the LDS-DMA kernel, one per patch otherwise and in the pair forward.  A
    buffer of conv3x3_mtiles() rows always suffices."""
    # pair: False / True (the pair forward: Cin = its K extent) / "q" (a "q" stage: Cin = K = 2 * channels; its form is chosen per shape)
    return int(_lib.load().gs_conv3x3_stat_rows(N, H, W, Cin, Cout, 2 if pair == "q" else (1 if pair else 0)))


def conv3d3_stat_rows(NB, D, H, W, Cin, Cout) -> int:
    return conv3x3_stat_rows(NB * D, H, W, Cin, Cout)


def set_persistent_grid(blocks: int = 0) -> None:
    """At most `blocks` workgroups for the persistent conv kernels (0: the default, one per CU); parallel.py leaves CUs to RCCL."""
    _lib.call("gs_set_persistent_grid", int(blocks))


def get_persistent_grid() -> int:
    return int(_lib.load().gs_get_persistent_grid())


def conv3x3_set_kernel_form(form: int = -1) -> None:
    """Diagnostics: pin the form of the conv3x3 kernel (-1 auto, 0 register-staged, 4 / 8 LDS-DMA waves per block).
    Process-wide; tests compare the forms on the same operands and restore -1."""
    _lib.call("gs_conv3x3_set_kernel_form", int(form))


def conv3x3(x, w, y, N, H, W, Cin, Cout, taps=TAPS3_FWD, bias=None, bn_partials=None, act=ACT_NONE,
            in_stride=None, in_coff=0, out_stride=None, out_coff=0):
    """3x3/s1/p1 convolution (or its data gradient with TAPS3_DGRAD + the dgrad weight pack) on the
    halo-reuse MFMA kernel.  x/y NHWC 16-bit (strided), w [9][Cout][Cin]."""
    _dev(x)
    _f32(bias, "bias"); _f32(bn_partials, "bn_partials")
    if not (x.dtype == w.dtype == y.dtype):
        raise TypeError("conv3x3: x, w, y must share one 16-bit dtype")
    if bn_partials is not None and bn_partials.numel() < bn_partials_numel(conv3x3_stat_rows(N, H, W, Cin, Cout), Cout):
        raise ValueError("conv3x3: bn_partials too small (conv3x3_stat_rows rows of [2][Cout])")
    dy, dx = _tap_arrays(taps)
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv3x3", _p(x), _p(w), _p(y), _p(bias), _p(bn_partials), N, H, W, Cin,
              Cin if in_stride is None else in_stride, in_coff, Cout, Cout if out_stride is None else out_stride,
              out_coff, dy, dx, act, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("conv3x3_halo", ev, 2.0 * N * H * W * Cout * 9 * Cin,
                   2.0 * (N * H * W * (Cin + Cout) + 9 * Cin * Cout))


def conv3x3_wgrad(x, dy, dw, N, H, W, Cin, Cout, in_stride=None, in_coff=0, out_stride=None, out_coff=0):
    """dw[9][Cout][Cin] (fp32, caller zeroes) += weight gradient of the 3x3/s1/p1 conv, halo-reuse MFMA kernel."""
    _dev(x)
    _f32(dw, "dw")
    if x.dtype != dy.dtype:
        raise TypeError("conv3x3_wgrad: x and dy must share one 16-bit dtype")
    if dw.numel() < 9 * Cout * Cin:
        raise ValueError("conv3x3_wgrad: dw too small")
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv3x3_wgrad", _p(x), _p(dy), _p(dw), N, H, W, Cin, Cin if in_stride is None else in_stride,
              in_coff, Cout, Cout if out_stride is None else out_stride, out_coff, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("wgrad3x3_halo", ev, 2.0 * N * H * W * Cout * 9 * Cin,
                   2.0 * N * H * W * (Cin + Cout) + 4.0 * 9 * Cin * Cout)


def upconv2x2_fwd(x, w, bias, y, N, D, IH, IW, Cin, Cout, Dout, OH, OW, in_stride=None, in_coff=0, out_stride=None,
                  out_coff=0, ooz=0, ooy=0, oox=0, act=ACT_NONE):
    """ConvTranspose2d/3d(kernel 2, stride 2) forward as one pointwise MFMA GEMM with a sub-pixel scatter.
    w: packed [4|8][Cout][Cin] (pack_weight(..., transposed=True)); y may be a concat buffer (out_coff)."""
    _dev(x)
    _f32(bias, "bias")
    if not (x.dtype == w.dtype == y.dtype):
        raise TypeError("upconv2x2_fwd: x, w, y must share one 16-bit dtype")
    ncls = 8 if (D > 1 or Dout > 1) else 4
    if w.numel() != ncls * Cout * Cin:
        raise ValueError("upconv2x2_fwd: packed weight has the wrong size")
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_upconv2x2_fwd", _p(x), _p(w), _p(bias), _p(y), N, D, IH, IW, Cin,
              Cin if in_stride is None else in_stride, in_coff, Cout, Dout, OH, OW,
              Cout if out_stride is None else out_stride, out_coff, ooz, ooy, oox, act, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("igemm_fwd", ev, 2.0 * N * D * IH * IW * Cin * ncls * Cout,
                   2.0 * (N * D * IH * IW * (Cin + ncls * Cout) + ncls * Cin * Cout))


def upconv2x2_dgrad(geom, dy, wd, dx, N, IH, IW, Cin, Cout, OH, OW, dy_stride, dy_coff, ooy, oox):
    """Data gradient of ConvTranspose2d(k 2, s 2): the LDS-DMA GEMM over (sub-pixel class, co) where it covers the shape
    (gs_upconv2x2_dgrad), else the generic engine on `geom` (the 4-tap stride-2 geometry of the same layer).  Both are HIP
    kernels; dx dense [N, IH, IW, Cin]."""
    _dev(dy)
    if not (dy.dtype == wd.dtype == dx.dtype):
        raise TypeError("upconv2x2_dgrad: dy, wd, dx must share one 16-bit dtype")
    ev = TIMER.start() if TIMER is not None else None
    rc = _lib.load().gs_upconv2x2_dgrad(_p(dy), _p(wd), _p(dx), N, IH, IW, Cin, Cout, OH, OW, dy_stride, dy_coff, ooy, oox,
                                        Cin, 0, dt_code(dy), _stream())
    if rc == _lib.GS_EUNSUPPORTED:            # shape outside the DMA GEMM: the generic engine (it times itself)
        return conv_igemm(geom, dy, wd, dx)
    if rc != 0:
        _lib.check(rc, "gs_upconv2x2_dgrad")
    if ev is not None:
        TIMER.stop("igemm_fwd", ev, 2.0 * N * IH * IW * Cin * 4 * Cout,
                   2.0 * (N * IH * IW * (Cin + 4 * Cout) + 4 * Cin * Cout))


def conv3d3_eligible(Cin, Cout, out_stride=None, out_coff=0) -> bool:
    """shapes the 3-D halo kernels take (others go through conv_igemm with depth taps)"""
    os_ = Cout if out_stride is None else out_stride
    return USE_HALO_CONV and Cin % 8 == 0 and Cout % 8 == 0 and os_ % 8 == 0 and out_coff % 8 == 0


def conv3d3_mtiles(NB, D, H, W, Cout) -> int:
    return int(_lib.load().gs_conv3d_3x3x3_mtiles(NB, D, H, W, Cout))


def conv3d3(x, w, y, NB, D, H, W, Cin, Cout, dgrad=False, bias=None, bn_partials=None, act=ACT_NONE, in_stride=None,
            in_coff=0, out_stride=None, out_coff=0):
    """Conv3d(k3, p1) forward (w = [27][Cout][Cin] pack) or data gradient (dgrad=True: x = dY, w = [27][Cin][Cout]
    pack, Cin/Cout given from the kernel's point of view: Cin = channels of x) on depth-slice NHWC tensors."""
    _dev(x)
    _f32(bias, "bias"); _f32(bn_partials, "bn_partials")
    if not (x.dtype == w.dtype == y.dtype):
        raise TypeError("conv3d3: x, w, y must share one 16-bit dtype")
    if w.numel() != 27 * Cout * Cin:
        raise ValueError("conv3d3: packed weight has the wrong size")
    if bn_partials is not None and bn_partials.numel() < bn_partials_numel(conv3d3_stat_rows(NB, D, H, W, Cin, Cout), Cout):
        raise ValueError("conv3d3: bn_partials too small")
    sgn = -1 if dgrad else 1
    dz, dy, dx = _TAPS3D[sgn]
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv3d_3x3x3", _p(x), _p(w), _p(y), _p(bias), _p(bn_partials), NB, D, H, W, Cin,
              Cin if in_stride is None else in_stride, in_coff, Cout, Cout if out_stride is None else out_stride, out_coff,
              dz, dy, dx, act, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("conv3x3_halo", ev, 2.0 * NB * D * H * W * Cout * 27 * Cin)


def conv3d3_wgrad(x, dy, dw, NB, D, H, W, Cin, Cout, in_stride=None, in_coff=0, out_stride=None, out_coff=0):
    """dw[27][Cout][Cin] (fp32, caller zeroes) += weight gradient of Conv3d(k3, p1)."""
    _dev(x)
    _f32(dw, "dw")
    if x.dtype != dy.dtype:
        raise TypeError("conv3d3_wgrad: x and dy must share one 16-bit dtype")
    if dw.numel() < 27 * Cout * Cin:
        raise ValueError("conv3d3_wgrad: dw too small")
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv3d_3x3x3_wgrad", _p(x), _p(dy), _p(dw), NB, D, H, W, Cin, Cin if in_stride is None else in_stride,
              in_coff, Cout, Cout if out_stride is None else out_stride, out_coff, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("wgrad3x3_halo", ev, 2.0 * NB * D * H * W * Cout * 27 * Cin)


def conv3d3_wgrad_ws_floats(NB, D, H, W, Cin, Cout) -> int:
    return int(_lib.load().gs_conv3d_3x3x3_wgrad_ws_floats(NB, D, H, W, Cin, Cout))


def conv3d3_wgrad_det(x, dy, ws, grad, NB, D, H, W, Cin, Cout, gscale, in_stride=None, in_coff=0, out_stride=None,
                      out_coff=0):
    """Deterministic Conv3d(k3,p1) weight gradient into the reference layout [Cout][Cin][3][3][3] (27 taps fastest):
    split-K parts in fp32 slabs (no zero fill), ordered reduction fused with scale + unpack.  No atomics."""
    _dev(x)
    _f32(ws, "ws"); _f32(grad, "grad")
    if x.dtype != dy.dtype:
        raise TypeError("conv3d3_wgrad_det: x and dy must share one 16-bit dtype")
    if ws.numel() < conv3d3_wgrad_ws_floats(NB, D, H, W, Cin, Cout) or grad.numel() != 27 * Cout * Cin:
        raise ValueError("conv3d3_wgrad_det: workspace / gradient size")
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv3d_3x3x3_wgrad_slabs", _p(x), _p(dy), _p(ws), NB, D, H, W, Cin, Cin if in_stride is None else in_stride,
              in_coff, Cout, Cout if out_stride is None else out_stride, out_coff, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("wgrad3x3_halo", ev, 2.0 * NB * D * H * W * Cout * 27 * Cin)
    parts = int(_lib.load().gs_conv3d_3x3x3_wgrad_parts(NB, D, H, W, Cin, Cout))
    _lib.call("gs_wgrad_reduce_unpack", _p(ws), parts, _p(grad), Cout, Cin, 27, 0, float(gscale), _stream())


def upsample2x_bilinear_fwd(x, y, N, IH, IW, C, OH, OW, in_stride=None, in_coff=0, out_stride=None, out_coff=0,
                            ooy=0, oox=0):
    """nn.Upsample(scale_factor=2, bilinear, align_corners=True) into a channel slice of the [N,OH,OW,*] buffer y."""
    _dev(x)
    if x.dtype != y.dtype:
        raise TypeError("upsample2x_bilinear_fwd: x and y must share one 16-bit dtype")
    _lib.call("gs_upsample2x_bilinear_fwd", _p(x), _p(y), N, IH, IW, C, C if in_stride is None else in_stride, in_coff,
              OH, OW, C if out_stride is None else out_stride, out_coff, ooy, oox, dt_code(x), _stream())


def upsample2x_bilinear_bwd(dy, dx, N, IH, IW, C, OH, OW, dy_stride=None, dy_coff=0, dx_stride=None, dx_coff=0,
                            ooy=0, oox=0):
    _dev(dy)
    if dy.dtype != dx.dtype:
        raise TypeError("upsample2x_bilinear_bwd: dy and dx must share one 16-bit dtype")
    _lib.call("gs_upsample2x_bilinear_bwd", _p(dy), _p(dx), N, IH, IW, C, C if dy_stride is None else dy_stride, dy_coff,
              OH, OW, C if dx_stride is None else dx_stride, dx_coff, ooy, oox, dt_code(dy), _stream())


def conv3x3_wgrad_parts(N, H, W, Cin, Cout) -> int:
    return int(_lib.load().gs_conv3x3_wgrad_parts(N, H, W, Cin, Cout))


def conv3x3_wgrad_family(W, Cout) -> int:
    """Kernel of the 3x3 weight gradient for this shape: 0 register-staged (W < 24), 1 LDS-DMA, 2 its 128-cout form."""
    return int(_lib.load().gs_conv3x3_wgrad_family(W, Cout))


def conv3x3_wgrad_ws_floats(N, H, W, Cin, Cout) -> int:
    return int(_lib.load().gs_conv3x3_wgrad_ws_floats(N, H, W, Cin, Cout))


def conv3x3_wgrad_det(x, dy, ws, grad, N, H, W, Cin, Cout, gscale, in_stride=None, in_coff=0, out_stride=None,
                      out_coff=0):
    """Deterministic 3x3 weight gradient straight into the reference layout: split-K parts in fp32 slabs (ws, no zero
    fill), then an ordered reduction fused with the scale + [Cout][Cin][3][3] unpack.  No atomics."""
    _dev(x)
    _f32(ws, "ws"); _f32(grad, "grad")
    if x.dtype != dy.dtype:
        raise TypeError("conv3x3_wgrad_det: x and dy must share one 16-bit dtype")
    if ws.numel() < conv3x3_wgrad_ws_floats(N, H, W, Cin, Cout) or grad.numel() != 9 * Cout * Cin:
        raise ValueError("conv3x3_wgrad_det: workspace / gradient size")
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv3x3_wgrad_slabs", _p(x), _p(dy), _p(ws), N, H, W, Cin, Cin if in_stride is None else in_stride,
              in_coff, Cout, Cout if out_stride is None else out_stride, out_coff, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("wgrad3x3_halo", ev, 2.0 * N * H * W * Cout * 9 * Cin,
                   2.0 * N * H * W * (Cin + Cout) + 4.0 * 9 * Cin * Cout)
    parts = int(_lib.load().gs_conv3x3_wgrad_parts(N, H, W, Cin, Cout))
    _lib.call("gs_wgrad_reduce_unpack", _p(ws), parts, _p(grad), Cout, Cin, 9, 0, float(gscale), _stream())


def conv_igemm_mtiles(g: GsConvGeom) -> int:
    return _lib.load().gs_conv_igemm_mtiles(g)


def conv_wgrad_single_pass(g: GsConvGeom) -> bool:
    """True when the weight gradient of this geometry is computed without a K split, i.e. conv_wgrad(assign=True) may
    write into an un-zeroed dw."""
    return bool(_lib.load().gs_conv_wgrad_single_pass(g))


def conv_wgrad(g: GsConvGeom, x, dy, dw, assign: bool = False):
    """dw[tap][Cout][Cin] (fp32) += weight gradient (caller zeroes dw); assign=True writes instead (single-pass only)."""
    _dev(x)
    _f32(dw, "dw")
    if x.dtype != dy.dtype:
        raise TypeError("conv_wgrad: x and dy must share one 16-bit dtype")
    if dw.numel() < g.ntaps * g.Cout * g.Cin:
        raise ValueError("conv_wgrad: dw too small")
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv_wgrad_assign" if assign else "gs_conv_wgrad", g, _p(x), _p(dy), _p(dw), dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("igemm_wgrad", ev, _geom_flops(g), _geom_bytes(g, True))


def conv_wgrad_parts(g: GsConvGeom) -> int:
    return int(_lib.load().gs_conv_wgrad_parts(g))


def conv_wgrad_ws_floats(g: GsConvGeom) -> int:
    return int(_lib.load().gs_conv_wgrad_ws_floats(g))


def conv_wgrad_det(g: GsConvGeom, x, dy, ws, grad, A, B, taps, gscale, transposed=False, packed=False):
    """Deterministic generic weight gradient straight into the reference layout grad[A][B][taps] (transposed: [B][A][taps];
    packed: the kernel layout [taps][A][B] is kept): K parts in fp32 slabs (ws, no zero fill, no atomics) + the ordered
    reduction fused with scale and unpack."""
    _dev(x)
    _f32(ws, "ws"); _f32(grad, "grad")
    if x.dtype != dy.dtype:
        raise TypeError("conv_wgrad_det: x and dy must share one 16-bit dtype")
    if A != g.Cout or B != g.Cin or grad.numel() != taps * A * B or ws.numel() < conv_wgrad_ws_floats(g):
        raise ValueError("conv_wgrad_det: workspace / gradient size")
    if packed:
        A, taps = taps * A, 1              # [taps*A][B][1] is the slab layout itself: a plain ordered sum
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv_wgrad_slabs", g, _p(x), _p(dy), _p(ws), dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("igemm_wgrad", ev, _geom_flops(g), _geom_bytes(g, True))
    parts = int(_lib.load().gs_conv_wgrad_parts(g))
    _lib.call("gs_wgrad_reduce_unpack", _p(ws), parts, _p(grad), A, B, taps, 1 if transposed else 0, float(gscale), _stream())


def upconv2x2_wgrad_ws_floats(N, IH, IW, Cin, Cout) -> int:
    """workspace floats of upconv2x2_wgrad_det's LDS-DMA path (0: shape not covered, the generic engine is used)"""
    return int(_lib.load().gs_upconv2x2_wgrad_ws_floats(N, IH, IW, Cin, Cout))


def upconv2x2_wgrad_det(geom, x, dy, ws, grad, N, IH, IW, Cin, Cout, OH, OW, x_stride, dy_stride, dy_coff, ooy, oox, gscale):
    """Deterministic weight gradient of ConvTranspose2d(k 2, s 2) into grad [Cin][Cout][2][2]: x = the layer's input (pixel
    stride x_stride), dy = d(output) inside a [N,OH,OW,dy_stride] buffer at channel dy_coff.  The LDS-DMA pointwise GEMM
    (csrc/upwgrad.hip) where it covers the shape, else the generic engine on `geom` (the layer seen from its output side)."""
    _dev(x)
    _f32(ws, "ws"); _f32(grad, "grad")
    if x.dtype != dy.dtype:
        raise TypeError("upconv2x2_wgrad_det: x and dy must share one 16-bit dtype")
    lib = _lib.load()
    parts = int(lib.gs_upconv2x2_wgrad_parts(N, IH, IW, Cin, Cout))
    if parts > 0 and grad.numel() == 4 * Cin * Cout and ws.numel() >= parts * 4 * Cin * Cout:
        ev = TIMER.start() if TIMER is not None else None
        rc = lib.gs_upconv2x2_wgrad_slabs(_p(x), _p(dy), _p(ws), N, IH, IW, Cin, x_stride, 0, Cout, OH, OW, dy_stride, dy_coff,
                                          ooy, oox, dt_code(x), _stream())
        if rc == 0:
            if ev is not None:
                TIMER.stop("igemm_wgrad", ev, 2.0 * N * IH * IW * Cin * 4 * Cout,
                           2.0 * N * IH * IW * (Cin + 4 * Cout) + 4.0 * 4 * Cin * Cout)
            _lib.call("gs_wgrad_reduce_unpack", _p(ws), parts, _p(grad), Cin, Cout, 4, 0, float(gscale), _stream())
            return
        if rc != _lib.GS_EUNSUPPORTED:
            _lib.check(rc, "gs_upconv2x2_wgrad_slabs")
    conv_wgrad_det(geom, dy, x, ws, grad, Cin, Cout, 4, gscale)


def conv_wgrad_det_batch(geoms, x, dy, ws, grad, gscale=1.0, reduce=True):
    """Deterministic weight gradients of up to four GEMMs (the sub-pixel classes of one merged transposed conv) in ONE
    launch, in the kernel layout grad[n][taps][Cout][Cin]: K parts in fp32 slabs (ws) + one ordered reduction over all
    classes; a layer that does not split K writes grad directly (ws unused).  reduce=False (K split only): the slabs
    [parts][n][taps][Cout][Cin] stay in ws for a consumer that sums them itself (upconv_split_wgrad(nparts=...)); grad may be
    None then."""
    _dev(x)
    _f32(grad, "grad")
    if x.dtype != dy.dtype:
        raise TypeError("conv_wgrad_det_batch: x and dy must share one 16-bit dtype")
    n, g0 = len(geoms), geoms[0]
    per = g0.ntaps * g0.Cout * g0.Cin
    parts = int(_lib.load().gs_conv_wgrad_parts(g0))
    if not reduce and parts <= 1:
        raise ValueError("conv_wgrad_det_batch: reduce=False needs a K split (conv_wgrad_parts > 1)")
    if reduce and (grad.numel() != n * per or not grad.is_contiguous()):
        raise ValueError("conv_wgrad_det_batch: grad must be contiguous [n][taps][Cout][Cin]")
    garr = (ctypes.POINTER(GsConvGeom) * n)(*[ctypes.pointer(g) for g in geoms])
    if parts > 1:
        _f32(ws, "ws")
        if ws.numel() < parts * n * per:
            raise ValueError("conv_wgrad_det_batch: workspace too small")
    target = grad if parts == 1 else ws
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv_wgrad_slabs_batch", n, garr, _p(x), _p(dy), _p(target), dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("igemm_wgrad", ev, sum(_geom_flops(g) for g in geoms), sum(_geom_bytes(g, True) for g in geoms))
    if parts > 1 and reduce:
        _lib.call("gs_wgrad_reduce_unpack", _p(ws), parts, _p(grad), n * g0.ntaps * g0.Cout, g0.Cin, 1, 0, float(gscale), _stream())
    elif parts == 1 and gscale != 1.0:
        grad.mul_(gscale)
    return parts


def bn_partials_numel(ntiles: int, C: int) -> int:
    return int(_lib.load().gs_bn_partials_floats(ntiles, C))


# ---------------------------------------------------------------------------- direct convs
def conv_smallcin_fwd(x, w, bias, y, bn_partials, k, stride, pad, act=ACT_NONE):
    _dev(x)
    _f32(x, "x"); _f32(w, "w"); _f32(bias, "bias"); _f32(bn_partials, "bn_partials")
    N, Cin, IH, IW = x.shape
    _, OH, OW, Cout = y.shape
    _lib.call("gs_conv_smallcin_fwd", _p(x), _p(w), _p(bias), _p(y), _p(bn_partials), N, Cin, IH, IW, Cout, OH, OW,
              k, stride, pad, act, dt_code(y), _stream())


def conv_smallcin_mtiles(N, OH, OW) -> int:
    return _lib.load().gs_conv_smallcin_mtiles(N, OH, OW)


def _direct_wgrad_ws(N, OH, OW, Cin, Cout, k, dev):
    n = int(_lib.load().gs_conv_direct_wgrad_ws_floats(N, OH, OW, Cin, Cout, k))
    return torch.empty(n, dtype=torch.float32, device=dev)


def conv_smallcin_wgrad(x, dy, dw, k, stride, pad, gscale):
    _f32(x, "x"); _f32(dw, "dw")
    N, Cin, IH, IW = x.shape
    _, OH, OW, Cout = dy.shape
    ws = _direct_wgrad_ws(N, OH, OW, Cin, Cout, k, x.device)
    _lib.call("gs_conv_smallcin_wgrad", _p(x), _p(dy), _p(dw), _p(ws), N, Cin, IH, IW, Cout, OH, OW, k, stride, pad,
              float(gscale), dt_code(dy), _stream())


def stem_bn_bwd_wgrad(y, dz, dz_stride, dz_coff, x, scale, shift, mean, invstd, c1, c2, act, dw, gscale) -> bool:
    """BatchNorm/activation backward apply + weight gradient of the one-channel 3x3 stem in one pass (dw += ...; the gradient
    w.r.t. the convolution's output stays in registers).  Returns False when the shape is outside the kernel (very wide
    images): the caller then runs bn_act_bwd_apply + conv_smallcin_wgrad."""
    _dev(y)
    _f32(x, "x"); _f32(dw, "dw")
    for n, t in (("scale", scale), ("shift", shift), ("mean", mean), ("invstd", invstd), ("c1", c1), ("c2", c2)):
        _f32(t, n)
    N, H, W, C = y.shape
    if C != 64 or tuple(x.shape) != (N, 1, H, W) or dw.numel() != 576 or y.dtype != dz.dtype:
        raise ValueError("stem_bn_bwd_wgrad: y [N,H,W,64], x [N,1,H,W], dw [64,1,3,3], one 16-bit dtype")
    if not (y.is_contiguous() and x.is_contiguous() and dw.is_contiguous()):
        raise ValueError("stem_bn_bwd_wgrad: y, x, dw must be contiguous")
    ws = _direct_wgrad_ws(N, H, W, 1, 64, 3, y.device)
    rc = _lib.load().gs_stem_bn_bwd_wgrad(_p(y), _p(dz), dz_stride, dz_coff, _p(x), _p(scale), _p(shift), _p(mean), _p(invstd),
                                          _p(c1), _p(c2), act, _p(dw), _p(ws), N, H, W, float(gscale), dt_code(y), _stream())
    if rc == _lib.GS_EUNSUPPORTED:
        return False
    if rc != 0:
        _lib.check(rc, "gs_stem_bn_bwd_wgrad")
    return True


# ---- the one-channel stem without its convolution output in memory (see include/gsseg.h)
def _stem_check(x, w, who):
    _dev(x)
    _f32(x, "x"); _f32(w, "w")
    if x.dim() != 4 or x.shape[1] != 1 or tuple(w.shape) != (64, 1, 3, 3) or not (x.is_contiguous() and w.is_contiguous()):
        raise ValueError(f"{who}: x [N,1,H,W] and w [64,1,3,3], contiguous fp32")
    return x.shape[0], x.shape[2], x.shape[3]


def stem_stats(x, w, bn_partials, tap_sums=None):
    """BatchNorm tile partials of conv(x, w) from the image alone; tap_sums [mtiles][54] fp32 (optional) receives each tile's
    nine tap sums and 45 Gram entries for stem_bwd_finalize."""
    N, H, W = _stem_check(x, w, "stem_stats")
    _f32(bn_partials, "bn_partials"); _f32(tap_sums, "tap_sums")
    mt = conv_smallcin_mtiles(N, H, W)
    if bn_partials.numel() < bn_partials_numel(mt, 64) or (tap_sums is not None and tap_sums.numel() < mt * 54):
        raise ValueError("stem_stats: bn_partials / tap_sums too small")
    _lib.call("gs_stem_stats", _p(x), _p(w), _p(bn_partials), _p(tap_sums), N, H, W, _stream())


def stem_bwd_onepass(x, z, dz, dz_stride, dz_coff, act, s1_partials, ws, z_stride=64) -> bool:
    """One pass over z (its sign = the activation's mask) and dz: s1_partials [stem_bwd_tiles][64] (sum g) and the slabs of
    A = sum g x_tap in ws [stem_bwd_tiles][576].  False: image too wide for the LDS strip.  z: dense [N,H,W,64], or (z_stride
    > 64) the first 64 channels of a wider buffer, e.g. the hi plane of a pair."""
    _dev(x)
    _f32(x, "x"); _f32(s1_partials, "s1_partials"); _f32(ws, "ws")
    N, H, W = x.shape[0], x.shape[2], x.shape[3]
    nt = stem_bwd_tiles(N, H, W)
    if (x.shape[1] != 1 or not x.is_contiguous() or s1_partials.numel() < nt * 64 or ws.numel() < nt * 576
            or tuple(z.shape) != (N, H, W, z_stride) or not z.is_contiguous() or z.dtype != dz.dtype or z_stride % 8 or z_stride < 64):
        raise ValueError("stem_bwd_onepass: x [N,1,H,W], z dense [N,H,W,z_stride], buffers of stem_bwd_tiles * 64 / 576 floats")
    rc = _lib.load().gs_stem_bwd_onepass_strided(_p(x), _p(z), z_stride, _p(dz), dz_stride, dz_coff, act, _p(s1_partials), _p(ws),
                                                 N, H, W, dt_code(z), _stream())
    if rc == _lib.GS_EUNSUPPORTED:
        return False
    if rc != 0:
        _lib.check(rc, "gs_stem_bwd_onepass")
    return True


def stem_bwd_finalize(ws, s1_partials, tap_sums, w, scale, mean, invstd, train_stats, gscale, dw, dgamma, dbeta, N, H, W):
    """BatchNorm weight / bias gradients (overwritten) and the stem weight gradient (accumulated) from the one-pass sums."""
    for n, t in (("ws", ws), ("s1_partials", s1_partials), ("tap_sums", tap_sums), ("w", w), ("dw", dw), ("dgamma", dgamma),
                 ("dbeta", dbeta)):
        _f32(t, n)
    nt = stem_bwd_tiles(N, H, W)
    if (dw.numel() != 576 or ws.numel() < nt * 576 or s1_partials.numel() < nt * 64
            or (tap_sums is not None and tap_sums.numel() < conv_smallcin_mtiles(N, H, W) * 54)):
        raise ValueError("stem_bwd_finalize: buffer sizes")
    _lib.call("gs_stem_bwd_finalize", _p(ws), _p(s1_partials), _p(tap_sums), _p(w), _p(scale), _p(mean), _p(invstd),
              int(bool(train_stats)), float(gscale), _p(dw), _p(dgamma), _p(dbeta), N, H, W, _stream())


def stem_fwd_bn(x, w, scale, shift, act, z):
    N, H, W = _stem_check(x, w, "stem_fwd_bn")
    _f32(scale, "scale"); _f32(shift, "shift")
    if tuple(z.shape) != (N, H, W, 64) or not z.is_contiguous():
        raise ValueError("stem_fwd_bn: z must be dense [N,H,W,64]")
    _lib.call("gs_stem_fwd_bn", _p(x), _p(w), _p(scale), _p(shift), act, _p(z), N, H, W, dt_code(z), _stream())


def stem_fwd_bn_pair(x, w, scale, shift, act, zpair, write_lo=True):
    """The stem in one pass into a pair buffer zpair [N,H,W,128] = [hi (64) | lo (64)]; write_lo=False leaves the lo plane alone."""
    N, H, W = _stem_check(x, w, "stem_fwd_bn_pair")
    _f32(scale, "scale"); _f32(shift, "shift")
    if tuple(zpair.shape) != (N, H, W, 128) or not zpair.is_contiguous():
        raise ValueError("stem_fwd_bn_pair: zpair must be dense [N,H,W,128]")
    lo = zpair.data_ptr() + 64 * zpair.element_size() if write_lo else None
    _lib.call("gs_stem_fwd_bn_pair", _p(x), _p(w), _p(scale), _p(shift), act, _p(zpair), lo, 128, N, H, W, dt_code(zpair), _stream())


def stem_bwd_tiles(N, H, W) -> int:
    return int(_lib.load().gs_stem_bwd_tiles(N, H, W))


def conv_smallcin_dgrad(dy, w, dx, k, stride, pad, gscale):
    _f32(w, "w"); _f32(dx, "dx")
    N, Cin, IH, IW = dx.shape
    _, OH, OW, Cout = dy.shape
    _lib.call("gs_conv_smallcin_dgrad", _p(dy), _p(w), _p(dx), N, Cin, IH, IW, Cout, OH, OW, k, stride, pad,
              float(gscale), dt_code(dy), _stream())


def conv_smallcout_fwd(x, w, bias, y, k=1, stride=1, pad=0):
    _dev(x)
    _f32(w, "w"); _f32(bias, "bias"); _f32(y, "y")
    N, IH, IW, Cin = x.shape
    _, Cout, OH, OW = y.shape
    _lib.call("gs_conv_smallcout_fwd", _p(x), _p(w), _p(bias), _p(y), N, IH, IW, Cin, Cout, OH, OW, k, stride, pad,
              dt_code(x), _stream())


def conv_smallcout_bwd(x, w, dy, dx, dw, db, k=1, stride=1, pad=0, gscale=1.0):
    _f32(w, "w"); _f32(dy, "dy"); _f32(dw, "dw"); _f32(db, "db")
    ref = x if x is not None else dx
    N, IH, IW, Cin = ref.shape
    _, Cout, OH, OW = dy.shape
    ws = _direct_wgrad_ws(N, OH, OW, Cin, Cout, k, ref.device) if dw is not None else None
    _lib.call("gs_conv_smallcout_bwd", _p(x), _p(w), _p(dy), _p(dx), _p(dw), _p(db), _p(ws), N, IH, IW, Cin, Cout,
              OH, OW, k, stride, pad, float(gscale), dt_code(ref), _stream())


# ---------------------------------------------------------------------------- BatchNorm / activation
def bn_finalize(partials, ntiles, C, count, gamma, beta, running_mean, running_var, momentum, eps,
                scale, shift, mean, invstd):
    for n, t in (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var),
                 ("scale", scale), ("shift", shift), ("mean", mean), ("invstd", invstd)):
        _f32(t, n)
    _lib.call("gs_bn_finalize", _p(partials), ntiles, C, float(count), _p(gamma), _p(beta), _p(running_mean),
              _p(running_var), float(momentum), float(eps), _p(scale), _p(shift), _p(mean), _p(invstd), _stream())
    # the kernel wrote the running statistics through raw pointers: tell torch (version counters key the engines' caches)
    for t in (running_mean, running_var):
        if t is not None:
            torch.autograd.graph.increment_version(t)


def bn_eval_coeffs(C, gamma, beta, running_mean, running_var, eps, scale, shift, mean, invstd):
    _lib.call("gs_bn_eval_coeffs", C, _p(gamma), _p(beta), _p(running_mean), _p(running_var), float(eps),
              _p(scale), _p(shift), _p(mean), _p(invstd), _stream())


def bn_act_apply(y, scale, shift, act, z, z_stride, z_coff, zp=None, keep_mask=None, keep_scale=1.0):
    N, H, W, C = y.shape
    if not y.is_contiguous():
        raise ValueError("bn_act_apply: y must be dense NHWC")
    _lib.call("gs_bn_act_apply", _p(y), _p(scale), _p(shift), act, _p(z), z_stride, z_coff, _p(zp), _p(keep_mask),
              float(keep_scale), N, H, W, C, dt_code(y), _stream())


def bn_bwd_tiles(N, H, W) -> int:
    return _lib.load().gs_bn_bwd_tiles(N, H, W)


def bn_bwd_tiles_used(N, H, W, pooled: bool) -> int:
    return _lib.load().gs_bn_bwd_tiles_used(N, H, W, int(pooled))


BN_BWD_NORMAL, BN_BWD_SLIM = 0, 1


def bn_bwd_set_form(form: int = BN_BWD_NORMAL) -> None:
    """Form of the plain bn_act_bwd_reduce / bn_act_bwd_apply launches (dz_a only, identity / ReLU, no pool): BN_BWD_SLIM
    is the <= 96-VGPR kernel that fits on a CU beside a weight-gradient block of another stream (bit-identical output)."""
    _lib.call("gs_bn_bwd_set_form", int(form))


def bn_set_traversal(mask: int = -1) -> None:
    """Tail-first traversal of the BatchNorm passes (bit mask: 1 forward apply, 2 backward reduce, 4 backward apply); -1 = the
    GSSEG_BN_REV environment value.  Results do not depend on it."""
    _lib.call("gs_bn_set_traversal", int(mask))


@contextlib.contextmanager
def bn_bwd_form(form: int):
    """bn_bwd_set_form(form) around a block of launches; the normal form again afterwards (nothing to do for the normal form)."""
    if form == BN_BWD_NORMAL:
        yield
        return
    bn_bwd_set_form(form)
    try:
        yield
    finally:
        bn_bwd_set_form(BN_BWD_NORMAL)


def bn_act_bwd_reduce(y, dz_a, sa, ca, dzp, scale, shift, mean, invstd, act, partials, dz_b=None, act_b=ACT_NONE,
                      keep_mask=None, keep_scale=1.0):
    N, H, W, C = y.shape
    _lib.call("gs_bn_act_bwd_reduce", _p(y), _p(dz_a), sa, ca, _p(dzp), _p(dz_b), act_b, _p(keep_mask),
              float(keep_scale), _p(scale), _p(shift), _p(mean), _p(invstd), act, _p(partials), N, H, W, C,
              dt_code(y), _stream())


def bn_bwd_coeffs(partials, ntiles, C, count, gscale, dgamma, dbeta, c1, c2):
    _lib.call("gs_bn_bwd_coeffs", _p(partials), ntiles, C, float(count), float(gscale), _p(dgamma), _p(dbeta),
              _p(c1), _p(c2), _stream())


def bn_act_bwd_apply(y, dz_a, sa, ca, dzp, scale, shift, mean, invstd, c1, c2, act, bn, dy, dz_b=None,
                     act_b=ACT_NONE, keep_mask=None, keep_scale=1.0):
    N, H, W, C = y.shape
    _lib.call("gs_bn_act_bwd_apply", _p(y), _p(dz_a), sa, ca, _p(dzp), _p(dz_b), act_b, _p(keep_mask),
              float(keep_scale), _p(scale), _p(shift), _p(mean), _p(invstd), _p(c1), _p(c2), act, int(bn), _p(dy),
              N, H, W, C, dt_code(y), _stream())


def maxpool3d_fwd(z, zp, NB, D, H, W, C, z_stride=None, z_coff=0):
    _dev(z)
    _lib.call("gs_maxpool3d_fwd", _p(z), C if z_stride is None else z_stride, z_coff, _p(zp), NB, D, H, W, C,
              dt_code(z), _stream())


def maxpool2x2_fwd(z, zp, N, H, W, C, z_stride=None, z_coff=0):
    """MaxPool2d(2) of a (strided) NHWC tensor into a dense one: the inference path's stand-alone pool."""
    _dev(z)
    if z.dtype != zp.dtype:
        raise TypeError("maxpool2x2_fwd: z and zp must share one 16-bit dtype")
    _lib.call("gs_maxpool2x2_fwd", _p(z), C if z_stride is None else z_stride, z_coff, _p(zp), N, H, W, C,
              dt_code(z), _stream())


def maxpool2x2_fwd_pair(z_hi, z_lo, z_stride, zp_hi, zp_lo, zp_stride, N, H, W, C):
    """MaxPool2d(2) on pairs (folded-BatchNorm inference of the pair forward): z_hi / z_lo two planes with pixel stride z_stride,
    pooled pair zp_hi / zp_lo (zp_lo may be None) with pixel stride zp_stride; the maximum is taken over the pair VALUES."""
    _dev(z_hi)
    if not (z_hi.dtype == z_lo.dtype == zp_hi.dtype):
        raise TypeError("maxpool2x2_fwd_pair: the planes must share one 16-bit dtype")
    _lib.call("gs_maxpool2x2_fwd_pair", _p(z_hi), _p(z_lo), z_stride, _p(zp_hi), _p(zp_lo), zp_stride, N, H, W, C, dt_code(z_hi), _stream())


def maxpool3d_bwd(z, dzp, dres, dz, NB, D, H, W, C, z_stride=None, z_coff=0, res_stride=0, res_coff=0):
    _lib.call("gs_maxpool3d_bwd", _p(z), C if z_stride is None else z_stride, z_coff, _p(dzp), _p(dres), res_stride,
              res_coff, _p(dz), NB, D, H, W, C, dt_code(z), _stream())


def head1x1_bn_fwd(y_conv, scale, shift, act, w, bias, logits):
    """1x1 head on z = act(y_conv * scale + shift) formed on the load path (the last stage's activation is never stored)."""
    _dev(y_conv)
    _f32(scale, "scale"); _f32(shift, "shift"); _f32(w, "w"); _f32(bias, "bias"); _f32(logits, "logits")
    N, H, W, C = y_conv.shape
    ncls = logits.shape[1]
    if C != 64 or tuple(logits.shape) != (N, ncls, H, W) or w.numel() != ncls * 64 or not (y_conv.is_contiguous() and logits.is_contiguous()):
        raise ValueError("head1x1_bn_fwd: y_conv [N,H,W,64], logits [N,ncls,H,W], w [ncls,64]")
    _lib.call("gs_head1x1_bn_fwd", _p(y_conv), _p(scale), _p(shift), act, _p(w), _p(bias), _p(logits), N, H, W, ncls,
              dt_code(y_conv), _stream())


def head1x1_bn_wgrad(y_conv, scale, shift, act, w, dl, dw, db, gscale=1.0):
    _dev(y_conv)
    _f32(scale, "scale"); _f32(shift, "shift"); _f32(w, "w"); _f32(dl, "dl"); _f32(dw, "dw"); _f32(db, "db")
    N, H, W, C = y_conv.shape
    ncls = dl.shape[1]
    if C != 64 or tuple(dl.shape) != (N, ncls, H, W) or dw.numel() != ncls * 64 or not (y_conv.is_contiguous() and dl.is_contiguous()):
        raise ValueError("head1x1_bn_wgrad: y_conv [N,H,W,64], dl [N,ncls,H,W], dw [ncls,64]")
    ws = _direct_wgrad_ws(N, H, W, 64, ncls, 1, y_conv.device)
    _lib.call("gs_head1x1_bn_wgrad", _p(y_conv), _p(scale), _p(shift), act, _p(w), _p(dl), _p(dw), _p(db), _p(ws), N, H, W,
              ncls, float(gscale), dt_code(y_conv), _stream())


def bn_act_bwd_reduce_head(y, dl, w_head, scale, shift, mean, invstd, act, partials):
    """bn_act_bwd_reduce with the gradient source dz = dl . w_head formed on the fly (the stage in front of a pointwise head)."""
    _dev(y)
    _f32(dl, "dl"); _f32(w_head, "w_head"); _f32(partials, "partials")
    N, H, W, C = y.shape
    ncls = dl.shape[1]
    if tuple(dl.shape) != (N, ncls, H, W) or w_head.numel() != ncls * C or not (dl.is_contiguous() and w_head.is_contiguous()):
        raise ValueError("bn_act_bwd_reduce_head: dl [N,ncls,H,W] and w_head [ncls,C] contiguous fp32")
    _lib.call("gs_bn_act_bwd_reduce_head", _p(y), _p(dl), _p(w_head), ncls, _p(scale), _p(shift), _p(mean), _p(invstd), act,
              _p(partials), N, H, W, C, dt_code(y), _stream())


def bn_act_bwd_apply_head(y, dl, w_head, scale, shift, mean, invstd, c1, c2, act, dy):
    _dev(y)
    _f32(dl, "dl"); _f32(w_head, "w_head")
    N, H, W, C = y.shape
    ncls = dl.shape[1]
    if tuple(dl.shape) != (N, ncls, H, W) or w_head.numel() != ncls * C or not (dl.is_contiguous() and w_head.is_contiguous()):
        raise ValueError("bn_act_bwd_apply_head: dl [N,ncls,H,W] and w_head [ncls,C] contiguous fp32")
    _lib.call("gs_bn_act_bwd_apply_head", _p(y), _p(dl), _p(w_head), ncls, _p(scale), _p(shift), _p(mean), _p(invstd),
              _p(c1), _p(c2), act, _p(dy), N, H, W, C, dt_code(y), _stream())


def bn_partials_colsum(partials, ntiles, Cfull, coff, C, gscale, out):
    """out[c] = gscale * sum over tiles of partials[tile][0][coff + c]: the column sums of a tensor, taken from the tile
    partials of the convolution that wrote it (ConvTranspose2d bias gradient without a pass over the tensor)."""
    _f32(partials, "partials"); _f32(out, "out")
    if partials.numel() < bn_partials_numel(ntiles, Cfull) or out.numel() < C:
        raise ValueError("bn_partials_colsum: buffer too small")
    _lib.call("gs_bn_partials_colsum", _p(partials), ntiles, Cfull, coff, C, float(gscale), _p(out), _stream())


def colsum(t, pix_stride, coff, N, H, W, y0, x0, h, w, C, gscale, ws, out):
    _f32(ws, "ws"); _f32(out, "out")
    if ws.numel() < 1024 * C:
        raise ValueError("colsum: workspace must hold 1024*C floats")
    _lib.call("gs_colsum", _p(t), pix_stride, coff, N, H, W, y0, x0, h, w, C, float(gscale), _p(ws), _p(out),
              dt_code(t), _stream())


# ---------------------------------------------------------------------------- InstanceNorm (csrc/instnorm.hip)
def in_ws_numel(N, H, W, C) -> int:
    """fp32 elements of the workspace gs_in_stats / gs_in_act_bwd need for this shape (0: none)"""
    return int(_lib.load().gs_in_ws_floats(N, H, W, C))


def in_workspace(N, H, W, C, dev):
    n = in_ws_numel(N, H, W, C)
    return torch.empty(n, dtype=torch.float32, device=dev) if n else None


def in_stats(y, eps, mean, invstd, ws=None):
    """per (sample, channel) mean and 1 / sqrt(biased variance + eps) of y [N,H,W,C] -> fp32 [N,C] each"""
    N, H, W, C = y.shape
    if not y.is_contiguous():
        raise ValueError("in_stats: y must be dense NHWC")
    _f32(mean, "mean"); _f32(invstd, "invstd"); _f32(ws, "ws")
    if mean.numel() != N * C or invstd.numel() != N * C or (ws.numel() if ws is not None else 0) < in_ws_numel(N, H, W, C):
        raise ValueError("in_stats: mean / invstd must hold N*C floats and ws in_ws_numel(N, H, W, C)")
    _lib.call("gs_in_stats", _p(y), float(eps), _p(mean), _p(invstd), _p(ws), N, H, W, C, dt_code(y), _stream())


def in_act_apply(y, mean, invstd, act, z, z_stride, z_coff, keep_mask=None, keep_scale=1.0, z2=None, act2=ACT_NONE,
                 z2_stride=0, z2_coff=0):
    N, H, W, C = y.shape
    if not y.is_contiguous():
        raise ValueError("in_act_apply: y must be dense NHWC")
    _f32(mean, "mean"); _f32(invstd, "invstd")
    if z.dtype != y.dtype or (z2 is not None and z2.dtype != y.dtype):
        raise TypeError("in_act_apply: y, z and z2 must share one 16-bit dtype")
    _lib.call("gs_in_act_apply", _p(y), _p(mean), _p(invstd), act, _p(z), z_stride, z_coff, _p(keep_mask), float(keep_scale),
              _p(z2), act2, z2_stride, z2_coff, N, H, W, C, dt_code(y), _stream())


def in_act_bwd(y, mean, invstd, dz_a, sa, ca, act, dy, gmeans, ws=None, dz_b=None, act_b=ACT_NONE, keep_mask=None, keep_scale=1.0):
    """dy of act(instance_norm(y)) [two consumers / dropout]; gmeans fp32 [2,N,C] receives mean_plane(g), mean_plane(g * xh)"""
    N, H, W, C = y.shape
    _f32(mean, "mean"); _f32(invstd, "invstd"); _f32(gmeans, "gmeans"); _f32(ws, "ws")
    if gmeans.numel() != 2 * N * C or (ws.numel() if ws is not None else 0) < in_ws_numel(N, H, W, C):
        raise ValueError("in_act_bwd: gmeans must hold 2*N*C floats and ws in_ws_numel(N, H, W, C)")
    if dz_a.dtype != y.dtype or dy.dtype != y.dtype or (dz_b is not None and dz_b.dtype != y.dtype):
        raise TypeError("in_act_bwd: y, dz_a, dz_b and dy must share one 16-bit dtype")
    _lib.call("gs_in_act_bwd", _p(y), _p(mean), _p(invstd), _p(dz_a), sa, ca, act, _p(keep_mask), float(keep_scale), _p(dz_b), act_b,
              _p(dy), _p(gmeans), _p(ws), N, H, W, C, dt_code(y), _stream())


# ---------------------------------------------------------------------------- ReflectionPad2d passes (csrc/reflect.hip)
NORM_NONE, NORM_BATCH, NORM_INSTANCE = 0, 1, 2


def reflect_norm_apply(y, coef_a, coef_b, norm, act, z, pad, res=None, res_pad=0, keep_mask=None, keep_scale=1.0):
    """z [N,H+2p,W+2p,C] = [res +] act(norm(y)) [* keep * keep_scale], interior and reflected border in one pass (pad 0: dense).
    norm: NORM_NONE / NORM_BATCH (coef_a / coef_b = scale / shift [C]) / NORM_INSTANCE (mean / invstd [N,C]); res: a tensor padded
    by res_pad whose interior is added (the residual stream)."""
    _dev(y)
    N, H, W, C = y.shape
    _f32(coef_a, "coef_a"); _f32(coef_b, "coef_b")
    if not (y.is_contiguous() and z.is_contiguous()) or (res is not None and not res.is_contiguous()):
        raise ValueError("reflect_norm_apply: y, z and res must be dense NHWC")
    if z.dtype != y.dtype or (res is not None and res.dtype != y.dtype):
        raise TypeError("reflect_norm_apply: y, z and res must share one 16-bit dtype")
    if tuple(z.shape) != (N, H + 2 * pad, W + 2 * pad, C):
        raise ValueError(f"reflect_norm_apply: z must be [N, H+2*pad, W+2*pad, C], got {tuple(z.shape)}")
    if res is not None and tuple(res.shape) != (N, H + 2 * res_pad, W + 2 * res_pad, C):
        raise ValueError(f"reflect_norm_apply: res must be [N, H+2*res_pad, W+2*res_pad, C], got {tuple(res.shape)}")
    want = {NORM_NONE: 0, NORM_BATCH: C, NORM_INSTANCE: N * C}.get(norm)
    if want is None or (coef_a.numel() if coef_a is not None else 0) != want or (coef_b.numel() if coef_b is not None else 0) != want:
        raise ValueError("reflect_norm_apply: coefficients must hold C (batch) / N*C (instance) floats, none without a norm")
    if keep_mask is not None and (keep_mask.dtype != torch.uint8 or keep_mask.numel() != y.numel() or not keep_mask.is_contiguous()):
        raise ValueError("reflect_norm_apply: keep_mask must be a dense uint8 [N,H,W,C]")
    _lib.call("gs_reflect_norm_apply", _p(y), _p(coef_a), _p(coef_b), norm, act, _p(res), res_pad, _p(keep_mask), float(keep_scale),
              _p(z), pad, N, H, W, C, dt_code(y), _stream())


def reflect_fold_add(dpad, out, pad, add=None):
    """out [N,H,W,C] = fold(dpad [N,H+2p,W+2p,C]) [+ add]: the backward of a reflection pad, fused with the residual stream's
    gradient; fixed summation order."""
    _dev(dpad)
    N, H, W, C = out.shape
    if tuple(dpad.shape) != (N, H + 2 * pad, W + 2 * pad, C) or (add is not None and add.shape != out.shape):
        raise ValueError("reflect_fold_add: dpad must be [N, H+2*pad, W+2*pad, C] and add like out")
    if not (dpad.is_contiguous() and out.is_contiguous()) or (add is not None and not add.is_contiguous()):
        raise ValueError("reflect_fold_add: dense NHWC tensors")
    if dpad.dtype != out.dtype or (add is not None and add.dtype != out.dtype):
        raise TypeError("reflect_fold_add: dpad, add and out must share one 16-bit dtype")
    _lib.call("gs_reflect_fold_add", _p(dpad), _p(add), _p(out), pad, N, H, W, C, dt_code(out), _stream())


def reflect_pad_image(x, xp, pad):
    """xp fp32 [N,C,H+2p,W+2p] = ReflectionPad2d(pad)(x fp32 NCHW)"""
    _dev(x)
    _f32(x, "x"); _f32(xp, "xp")
    N, C, H, W = x.shape
    if tuple(xp.shape) != (N, C, H + 2 * pad, W + 2 * pad):
        raise ValueError("reflect_pad_image: xp must be [N, C, H+2*pad, W+2*pad]")
    _lib.call("gs_reflect_pad_image", _p(x), _p(xp), pad, N, C, H, W, _stream())


def reflect_fold_image(dxp, dx, pad):
    """dx fp32 [N,C,H,W] = fold(dxp fp32 [N,C,H+2p,W+2p]): backward of reflect_pad_image"""
    _dev(dxp)
    _f32(dxp, "dxp"); _f32(dx, "dx")
    N, C, H, W = dx.shape
    if tuple(dxp.shape) != (N, C, H + 2 * pad, W + 2 * pad):
        raise ValueError("reflect_fold_image: dxp must be [N, C, H+2*pad, W+2*pad]")
    _lib.call("gs_reflect_fold_image", _p(dxp), _p(dx), pad, N, C, H, W, _stream())


def tanh_fwd(x, t):
    _dev(x)
    _f32(x, "x"); _f32(t, "t")
    if t.numel() != x.numel():
        raise ValueError("tanh_fwd: sizes differ")
    _lib.call("gs_tanh_fwd", _p(x), _p(t), x.numel(), _stream())


def tanh_bwd(t, dout, gscale, d):
    """d = gscale * dout * (1 - t) * (1 + t)"""
    _dev(t)
    _f32(t, "t"); _f32(dout, "dout"); _f32(d, "d")
    if dout.numel() != t.numel() or d.numel() != t.numel():
        raise ValueError("tanh_bwd: sizes differ")
    _lib.call("gs_tanh_bwd", _p(t), _p(dout), float(gscale), _p(d), t.numel(), _stream())


# ---------------------------------------------------------------------------- the 7x7 ends (csrc/ends.hip)
def _ends_w(w, w_img_major, cimg, c16, k, who):
    _f32(w, "w")
    want = (cimg, c16, k, k) if w_img_major else (c16, cimg, k, k)
    if tuple(w.shape) != want or not w.is_contiguous():
        raise ValueError(f"{who}: weight must be a dense {want}, got {tuple(w.shape)}")


def conv_ends_mtiles(N, OH, OW) -> int:
    return _lib.load().gs_conv_ends_mtiles(N, OH, OW)


def conv_ends_to_c16(img, w, out, bn_partials, pad=0, flip=False, w_img_major=False):
    """out 16-bit [N,OH,OW,C16] = conv(img fp32 [N,Cimg,IH,IW]), k x k stride 1, OH = IH + 2 pad - k + 1; any C16 % 8 == 0.
    (pad 0, stem weight): the stem forward, with BatchNorm partials; (pad k-1, flip, head weight): the head's data gradient."""
    _dev(img)
    _f32(img, "img"); _f32(bn_partials, "bn_partials")
    N, Cimg, IH, IW = img.shape
    _, OH, OW, C16 = out.shape
    k = w.shape[-1]
    _ends_w(w, w_img_major, Cimg, C16, k, "conv_ends_to_c16")
    if not (img.is_contiguous() and out.is_contiguous()) or out.shape[0] != N:
        raise ValueError("conv_ends_to_c16: dense img [N,Cimg,IH,IW] and out [N,OH,OW,C16]")
    _lib.call("gs_conv_ends_to_c16", _p(img), _p(w), _p(out), _p(bn_partials), N, Cimg, IH, IW, C16, OH, OW, k, pad, int(flip),
              int(w_img_major), dt_code(out), _stream())


def conv_ends_to_img(t16, w, bias, out, pad=0, flip=False, w_img_major=True, gscale=1.0):
    """out fp32 [N,Cimg,OH,OW] = gscale * conv(t16 [N,IH,IW,C16]) + bias.  (pad 0, head weight): the head forward;
    (pad k-1, flip, stem weight): the stem's data gradient."""
    _dev(t16)
    _f32(out, "out"); _f32(bias, "bias")
    N, IH, IW, C16 = t16.shape
    _, Cimg, OH, OW = out.shape
    k = w.shape[-1]
    _ends_w(w, w_img_major, Cimg, C16, k, "conv_ends_to_img")
    if not (t16.is_contiguous() and out.is_contiguous()) or out.shape[0] != N or (bias is not None and bias.numel() != Cimg):
        raise ValueError("conv_ends_to_img: dense t16 [N,IH,IW,C16], out [N,Cimg,OH,OW], bias [Cimg]")
    _lib.call("gs_conv_ends_to_img", _p(t16), _p(w), _p(bias), _p(out), N, IH, IW, C16, Cimg, OH, OW, k, pad, int(flip),
              int(w_img_major), float(gscale), dt_code(t16), _stream())


def conv_ends_wgrad(t16, img, dw, db, pad=0, flip=False, w_img_major=False, gscale=1.0):
    """dw (in the weight's own layout) = gscale * sum_p t16[p][c16] * img[cimg][p + tap - pad]; db [Cimg] = gscale * sum img.
    (t16 = dy, img = padded input, pad 0): the stem; (t16 = padded input, img = d out, pad k-1, flip, head weight): the head."""
    _dev(t16)
    _f32(img, "img"); _f32(dw, "dw"); _f32(db, "db")
    N, TH, TW, C16 = t16.shape
    _, Cimg, BH, BW = img.shape
    k = dw.shape[-1]
    _ends_w(dw, w_img_major, Cimg, C16, k, "conv_ends_wgrad")
    if not (t16.is_contiguous() and img.is_contiguous()) or img.shape[0] != N or (db is not None and db.numel() != Cimg):
        raise ValueError("conv_ends_wgrad: dense t16 [N,TH,TW,C16], img [N,Cimg,BH,BW], db [Cimg]")
    ws = torch.empty(int(_lib.load().gs_conv_ends_wgrad_ws_floats(N, TH, TW, Cimg, C16, k)), dtype=torch.float32, device=t16.device)
    _lib.call("gs_conv_ends_wgrad", _p(t16), _p(img), _p(dw), _p(db), _p(ws), N, TH, TW, C16, Cimg, BH, BW, k, pad, int(flip),
              int(w_img_major), float(gscale), dt_code(t16), _stream())


def geom_convT3_class(N, IH, IW, Cin, Cout, py, px, **kw) -> GsConvGeom:
    """Sub-pixel class (py,px) of ConvTranspose2d(3, stride 2, padding 1, output_padding 1): 1 / 2 / 2 / 4 taps, output 2IH x 2IW
    (the extra row / column of output_padding is the trailing one); weight slots index the [9][Cout][Cin] pack."""
    return geom_convT_class(N, IH, IW, Cin, Cout, 3, 1, py, px, OH=2 * IH, OW=2 * IW, **kw)


# ---------------------------------------------------------------------------- packing / layout
def pack_weight(w, w_fwd, w_dgrad, transposed: bool):
    _dev(w)
    _f32(w, "weight")
    if transposed:
        Cin, Cout = w.shape[0], w.shape[1]
    else:
        Cout, Cin = w.shape[0], w.shape[1]
    taps = w.shape[2] * w.shape[3]
    ref = w_fwd if w_fwd is not None else w_dgrad
    _lib.call("gs_pack_weight", _p(w), _p(w_fwd), _p(w_dgrad), Cout, Cin, taps, int(transposed), dt_code(ref), _stream())


def pack_weight_multi(items):
    """items: (w, w_fwd, w_dgrad, transposed) tuples as for pack_weight (3x3 convs and k2/s2 transposed convs): one launch."""
    if not items:
        return
    descs = (_lib.GsPackDesc * len(items))()
    ref = None
    for d, (w, w_fwd, w_dgrad, transposed) in zip(descs, items):
        _dev(w)
        _f32(w, "weight")
        r = w_fwd if w_fwd is not None else w_dgrad
        if ref is None:
            ref = r
        elif r.dtype != ref.dtype:
            raise TypeError("pack_weight_multi: all packs must share one 16-bit dtype")
        cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
        d.w, d.w_fwd, d.w_dgrad = _p(w), _p(w_fwd), _p(w_dgrad)
        d.Cout, d.Cin, d.taps, d.transposed = cout, cin, w.shape[2] * w.shape[3], int(transposed)
    _lib.call("gs_pack_weight_multi", len(items), descs, dt_code(ref), _stream())


def unpack_wgrad(dw, grad, A, B, taps, transposed: bool, gscale):
    _f32(dw, "dw"); _f32(grad, "grad")
    _lib.call("gs_unpack_wgrad", _p(dw), _p(grad), A, B, taps, int(transposed), float(gscale), _stream())


def nchw_to_nhwc(src, dst, dst_stride=None, dst_coff=0):
    _f32(src, "src")
    N, C, H, W = src.shape
    _lib.call("gs_nchw_to_nhwc", _p(src), _p(dst), N, C, H, W, C if dst_stride is None else dst_stride, dst_coff,
              dt_code(dst), _stream())


def nhwc_to_nchw(src, dst, src_stride=None, src_coff=0, gscale=1.0):
    _f32(dst, "dst")
    N, C, H, W = dst.shape
    _lib.call("gs_nhwc_to_nchw", _p(src), C if src_stride is None else src_stride, src_coff, _p(dst), N, C, H, W,
              float(gscale), dt_code(src), _stream())


# ---------------------------------------------------------------------------- Pix2Pix mixed up-conv
def upconv_merge_pack(w4, w6, w8, softmax3, pack_fwd=None, pack_dgrad=None, merged_f32=None):
    _dev(w8)
    for n, t in (("w4", w4), ("w6", w6), ("w8", w8), ("softmax3", softmax3), ("merged", merged_f32)):
        _f32(t, n)
    Cin, Cout = w8.shape[0], w8.shape[1]
    ref = pack_fwd if pack_fwd is not None else pack_dgrad
    code = dt_code(ref) if ref is not None else GS_F16
    _lib.call("gs_upconv_merge_pack", _p(w4), _p(w6), _p(w8), _p(softmax3), _p(pack_fwd), _p(pack_dgrad),
              _p(merged_f32), Cin, Cout, code, _stream())


def upconv8_image_fits(Cin: int, Cout: int) -> bool:
    """LDS budget of the direct outermost-layer kernel (gs_upconv8_image_fwd)."""
    return Cin % 8 == 0 and 1 <= Cout <= 4 and (144 * (Cin + 8) + 64 * Cout * Cin) * 2 <= 64 * 1024


def upconv8_image_fwd(x, pack_fwd, bias, out, u, N, h, w, Cin, Cout, act, in_stride=None, in_coff=0):
    """Merged 8x8/s2/p3 transposed conv to a 1..4-channel fp32 NCHW image (+bias, activation); u: optional 16-bit NHWC
    pre-activation [N,2h,2w,8]."""
    _dev(x)
    _f32(bias, "bias"); _f32(out, "out")
    if x.dtype != pack_fwd.dtype or (u is not None and u.dtype != x.dtype):
        raise TypeError("upconv8_image_fwd: x, pack and u must share one 16-bit dtype")
    if pack_fwd.numel() != 4 * 16 * 8 * Cin or out.numel() != N * Cout * 4 * h * w:
        raise ValueError("upconv8_image_fwd: pack / output size")
    _lib.call("gs_upconv8_image_fwd", _p(x), Cin if in_stride is None else in_stride, in_coff, _p(pack_fwd), 8, _p(bias),
              _p(out), _p(u), N, h, w, Cin, Cout, act, dt_code(x), _stream())


def upconv8_image_wgrad_ok(Cin, Cout) -> bool:
    return bool(_lib.load().gs_upconv8_image_wgrad_ok(int(Cin), int(Cout)))


def upconv8_image_wgrad(x, du, dwm, N, h, w, Cin):
    """Weight gradient of the merged 8x8/s2/p3 transposed conv to ONE image channel: x [N,h,w,>=Cin] 16-bit (channels from 0), du
    [N,2h,2w,cpad] 16-bit (channel 0), dwm fp32 [4][16][1][Cin] (un-scaled sums, the layout upconv_split_wgrad reads)."""
    _dev(x)
    _f32(dwm, "dwm")
    if x.dtype != du.dtype or x.dim() != 4 or du.dim() != 4 or tuple(x.shape[:3]) != (N, h, w) or tuple(du.shape[:3]) != (N, 2 * h, 2 * w):
        raise ValueError("upconv8_image_wgrad: x [N,h,w,C] and du [N,2h,2w,cpad] of one 16-bit dtype")
    if not (x.is_contiguous() and du.is_contiguous()) or dwm.numel() != 64 * Cin or not dwm.is_contiguous():
        raise ValueError("upconv8_image_wgrad: dense x / du, dwm [4][16][1][Cin]")
    ws = torch.empty(int(_lib.load().gs_upconv8_image_wgrad_ws_floats(N, h, w, Cin)), dtype=torch.float32, device=x.device)
    _lib.call("gs_upconv8_image_wgrad", _p(x), x.shape[3], _p(du), du.shape[3], _p(ws), _p(dwm), N, h, w, Cin, dt_code(x), _stream())


def upconv_split_wgrad_parts_ok(Cin, Cout) -> bool:
    return bool(_lib.load().gs_upconv_split_wgrad_parts_ok(int(Cin), int(Cout)))


def upconv_split_wgrad(dwm, w4, w6, w8, softmax3, gscale, dw4, dw6, dw8, dots3, nparts=1):
    """merged weight gradient [4][16][Cout][Cin] -> dW4 / dW6 / dW8 (+ the three architecture dot products).  nparts > 1: dwm is
    the stack of split-K slabs of conv_wgrad_det_batch(reduce=False), summed in part order on the way."""
    for n, t in (("dwm", dwm), ("dw4", dw4), ("dw6", dw6), ("dw8", dw8), ("dots3", dots3)):
        _f32(t, n)
    Cin, Cout = w8.shape[0], w8.shape[1]
    # deterministic form: per-block partial dot products in a scratch tensor, summed in block order
    ws = torch.empty(int(_lib.load().gs_upconv_split_wgrad_ws_floats(Cin, Cout)), dtype=torch.float32, device=dwm.device)
    if nparts > 1:
        if dwm.numel() < nparts * 64 * Cin * Cout:
            raise ValueError("upconv_split_wgrad: the slab stack is too small")
        _lib.call("gs_upconv_split_wgrad_parts", _p(dwm), int(nparts), 64 * Cin * Cout, _p(w4), _p(w6), _p(w8), _p(softmax3),
                  float(gscale), _p(dw4), _p(dw6), _p(dw8), _p(dots3), _p(ws), Cin, Cout, _stream())
        return
    _lib.call("gs_upconv_split_wgrad_det", _p(dwm), _p(w4), _p(w6), _p(w8), _p(softmax3), float(gscale), _p(dw4), _p(dw6),
              _p(dw8), _p(dots3), _p(ws), Cin, Cout, _stream())


def fake_postprocess(x, out, gamma_lut):
    """gs_fake_postprocess: min-max -> uint8 -> equalise -> gamma -> float of an fp32 batch [N,C,H,W]; every
    (image, channel) plane has its own histogram (torchvision equalises channel by channel), min/max are global."""
    _dev(x)
    _f32(x, "x"); _f32(out, "out"); _f32(gamma_lut, "gamma_lut")
    if not x.is_contiguous() or out.shape != x.shape or gamma_lut.numel() != 256:
        raise ValueError("fake_postprocess: contiguous x, out of the same shape and a 256-entry gamma table")
    N = x.shape[0] * (x.shape[1] if x.dim() == 4 else 1)
    hw = x.numel() // N
    ws = torch.empty(int(_lib.load().gs_fake_postprocess_ws_floats(N)), dtype=torch.float32, device=x.device)
    _lib.call("gs_fake_postprocess", _p(x), _p(out), _p(ws), _p(gamma_lut), N, hw, _stream())


def isic_fake_trans(x, out, equalize_on, bits, sharpness_on, sharpness_factor, autocontrast_on, saturation_factor):
    """gs_isic_fake_trans on an fp32 batch [N,C,H,W]; saturation_factor None = no saturation step.  The blend ratios are
    passed as (float32(r), float32(1.0 - r)) with the subtraction in double, as torchvision's `_blend` evaluates them."""
    _dev(x)
    _f32(x, "x"); _f32(out, "out")
    if x.dim() != 4 or not x.is_contiguous() or out.shape != x.shape or not out.is_contiguous():
        raise ValueError("isic_fake_trans: contiguous x, out [N,C,H,W] of one shape")
    N, C, H, W = x.shape
    ws = torch.empty(int(_lib.load().gs_isic_fake_trans_ws_bytes(N * C, H * W)), dtype=torch.uint8, device=x.device)
    sat_on = saturation_factor is not None and C == 3
    sr = float(saturation_factor) if sat_on else 1.0
    _lib.call("gs_isic_fake_trans", _p(x), _p(out), _p(ws), N, C, H, W, int(bool(equalize_on)), int(bits),
              int(bool(sharpness_on)), float(sharpness_factor), float(1.0 - float(sharpness_factor)), int(bool(autocontrast_on)),
              int(sat_on), sr, float(1.0 - sr), _stream())


# ---------------------------------------------------------------------------- losses
LOSS_WS = 4 * 1024


def seg_loss_fwd(logits, mask_u8, ws, out):
    _dev(logits)
    _f32(logits, "logits"); _f32(ws, "ws"); _f32(out, "out")
    if mask_u8.dtype != torch.uint8 or not mask_u8.is_contiguous():
        raise TypeError("mask must be contiguous uint8 [N,H,W]")
    N, C, H, W = logits.shape
    if mask_u8.numel() != N * H * W:
        raise ValueError("mask / logits shape mismatch")
    _lib.call("gs_seg_loss_fwd", _p(logits), _p(mask_u8), N, C, H, W, _p(ws), _p(out), _stream())


def seg_loss_bwd(logits, mask_u8, out, gout, gscale, dlogits):
    N, C, H, W = logits.shape
    _f32(dlogits, "dlogits"); _f32(gout, "gout")
    _lib.call("gs_seg_loss_bwd", _p(logits), _p(mask_u8), _p(out), _p(gout), float(gscale), _p(dlogits), N, C, H, W,
              _stream())


def _wce_shapes(logits, target_u8, weight, who):
    if logits.dim() < 3:
        raise ValueError(f"{who}: logits must be [N,C,*spatial] with at least one spatial dim, got {tuple(logits.shape)}")
    N, C = logits.shape[0], logits.shape[1]
    S = logits.numel() // (N * C) if N * C else 0
    if target_u8.dtype != torch.uint8 or not target_u8.is_contiguous() or target_u8.device != logits.device:
        raise TypeError(f"{who}: target must be contiguous uint8 [N,*spatial] on the logits' device")
    if target_u8.numel() != N * S:
        raise ValueError(f"{who}: target {tuple(target_u8.shape)} does not match logits {tuple(logits.shape)}")
    if weight is not None:
        _f32(weight, "weight")
        if weight.numel() != C or weight.device != logits.device:
            raise ValueError(f"{who}: weight must hold one fp32 value per class ({C}) on the logits' device")
    return N, C, S


def wce_ws_floats():
    return int(_lib.load().gs_wce_ws_floats())


def wce_fwd(logits, target_u8, weight, ws, out, labels=None):
    """gs_wce_fwd: class-weighted cross-entropy of fp32 logits [N,C,*spatial] against uint8 targets [N,*spatial]; out[8] = loss,
    numerator, W, 1, 0...; labels (uint8, one byte per voxel, or None): the arg-max label map from the same pass."""
    _dev(logits)
    _f32(logits, "logits"); _f32(ws, "ws"); _f32(out, "out")
    N, C, S = _wce_shapes(logits, target_u8, weight, "wce_fwd")
    if ws.numel() < wce_ws_floats() or out.numel() < 8:
        raise ValueError("wce_fwd: ws must hold gs_wce_ws_floats() floats and out 8")
    if labels is not None and (labels.dtype != torch.uint8 or not labels.is_contiguous() or labels.numel() != N * S
                               or labels.device != logits.device):
        raise TypeError("wce_fwd: labels must be contiguous uint8 with one byte per voxel on the logits' device")
    _lib.call("gs_wce_fwd", _p(logits), _p(target_u8), _p(weight), N, C, S, _p(ws), _p(out), _p(labels), _stream())


def wce_bwd(logits, target_u8, weight, out, gout, gscale, dlogits):
    """gs_wce_bwd: dlogits (overwritten) = gout * gscale * out[3] * w[t] * (softmax - onehot) / out[2]; gout a device scalar or None."""
    _dev(logits)
    _f32(logits, "logits"); _f32(out, "out"); _f32(gout, "gout"); _f32(dlogits, "dlogits")
    N, C, S = _wce_shapes(logits, target_u8, weight, "wce_bwd")
    if dlogits.shape != logits.shape or dlogits.device != logits.device or out.numel() < 8:
        raise ValueError("wce_bwd: dlogits must have the logits' shape and device, out 8 floats")
    _lib.call("gs_wce_bwd", _p(logits), _p(target_u8), _p(weight), _p(out), _p(gout), float(gscale), _p(dlogits), N, C, S,
              _stream())


def dice_loss_fwd(p, t, ws, out):
    _dev(p)
    _f32(p, "input"); _f32(t, "target")
    _lib.call("gs_dice_loss_fwd", _p(p), _p(t), p.numel(), _p(ws), _p(out), _stream())


def dice_loss_bwd(t, out, gout, dp):
    _lib.call("gs_dice_loss_bwd", _p(t), _p(out), _p(gout), _p(dp), t.numel(), _stream())


def dice_coeff_batched(p, t, out):
    """Per-item Dice coefficients of p, t [B, n_per] fp32 in one launch pair: out[0] = mean, out[1 + b] = dice_b."""
    _dev(p)
    _f32(p, "p"); _f32(t, "t"); _f32(out, "out")
    B, n_per = p.shape
    if t.shape != p.shape or out.numel() < 1 + B:
        raise ValueError("dice_coeff_batched: p, t must be [B, n] of one shape and out hold 1 + B floats")
    ws = torch.empty(int(_lib.load().gs_dice_batched_ws_floats(B)), dtype=torch.float32, device=p.device)
    _lib.call("gs_dice_coeff_batched", _p(p), _p(t), B, n_per, _p(ws), _p(out), _stream())


def eval_dice(logits, mask_u8, out):
    """Fused evaluation head (unet/evaluate.py:29-43): threshold / arg-max + per-(sample, foreground class) Dice, mean in out[0]."""
    _dev(logits)
    _f32(logits, "logits"); _f32(out, "out")
    N, C, H, W = logits.shape
    if mask_u8.dtype != torch.uint8 or not mask_u8.is_contiguous() or mask_u8.numel() != N * H * W:
        raise TypeError("eval_dice: mask must be contiguous uint8 [N,H,W]")
    B = N * max(1, C - 1)
    if out.numel() < 1 + B:
        raise ValueError("eval_dice: out must hold 1 + N*max(1,C-1) floats")
    ws = torch.empty(int(_lib.load().gs_dice_batched_ws_floats(B)), dtype=torch.float32, device=logits.device)
    _lib.call("gs_eval_dice", _p(logits), _p(mask_u8), N, C, H * W, _p(ws), _p(out), _stream())


def jaccard_seg_loss_fwd(logits, mask_u8, out):
    _dev(logits)
    _f32(logits, "logits"); _f32(out, "out")
    N, C, H, W = logits.shape
    if C != 1:
        raise ValueError("the Jaccard loss of train_end2end_isic.py is the one-class form")
    if mask_u8.dtype != torch.uint8 or not mask_u8.is_contiguous() or mask_u8.numel() != N * H * W:
        raise TypeError("mask must be contiguous uint8 [N,H,W]")
    if out.numel() < int(_lib.load().gs_jaccard_loss_out_floats(N)):
        raise ValueError("jaccard_seg_loss_fwd: out too small")
    ws = torch.empty(int(_lib.load().gs_dice_batched_ws_floats(N)), dtype=torch.float32, device=logits.device)
    _lib.call("gs_jaccard_seg_loss_fwd", _p(logits), _p(mask_u8), N, H * W, _p(ws), _p(out), _stream())


def jaccard_seg_loss_bwd(logits, mask_u8, out, gout, gscale, dlogits):
    _f32(gout, "gout"); _f32(dlogits, "dlogits")
    N, C, H, W = logits.shape
    _lib.call("gs_jaccard_seg_loss_bwd", _p(logits), _p(mask_u8), _p(out), _p(gout), float(gscale), _p(dlogits), N, H * W,
              _stream())


def eval_jaccard(logits, mask_u8, out):
    """Fused ISIC validation metric (train_end2end_isic.py:58-84): threshold + per-sample Jaccard index, mean in out[0]."""
    _dev(logits)
    _f32(logits, "logits"); _f32(out, "out")
    N, C, H, W = logits.shape
    if C != 1 or mask_u8.dtype != torch.uint8 or not mask_u8.is_contiguous() or mask_u8.numel() != N * H * W or out.numel() < 1 + N:
        raise ValueError("eval_jaccard: one-class logits, contiguous uint8 mask [N,H,W], out of 1 + N floats")
    ws = torch.empty(int(_lib.load().gs_dice_batched_ws_floats(N)), dtype=torch.float32, device=logits.device)
    _lib.call("gs_eval_jaccard", _p(logits), _p(mask_u8), N, H * W, _p(ws), _p(out), _stream())


def mean_loss_fwd(x, t, cval, mode, ws, out):
    _dev(x)
    _f32(x, "x"); _f32(t, "target")
    _lib.call("gs_mean_loss_fwd", _p(x), _p(t), float(cval), mode, x.numel(), _p(ws), _p(out), _stream())


def mean_loss_bwd(x, t, cval, mode, gout, gscale, dx):
    _lib.call("gs_mean_loss_bwd", _p(x), _p(t), float(cval), mode, x.numel(), _p(gout), float(gscale), _p(dx), _stream())


# ---------------------------------------------------------------------------- precise mode (hi/lo 16-bit pairs)
# Tensors named *_hi / *_lo are the two planes of a pair; they may be channel slices of one buffer (the conv kernels
# want [hi | lo] side by side: in_wrap = channels of both planes) or two dense tensors.  Strides are in elements.
def pack_weight_split(w, pack, transposed: bool):
    """fp32 conv weight [Cout][Cin][kh][kw] (transposed: [Cin][Cout][kh][kw]) -> pack [taps][Cout][3*Cin] = [hi | hi | lo]."""
    _dev(w)
    _f32(w, "w")
    taps = w.shape[2] * w.shape[3]
    cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    if pack.numel() != taps * cout * 3 * cin or not pack.is_contiguous():
        raise ValueError("pack_weight_split: pack must be contiguous [taps][Cout][3*Cin]")
    _lib.call("gs_pack_weight_split", _p(w), _p(pack), cout, cin, taps, 1 if transposed else 0, dt_code(pack), _stream())


def conv3x3_precise(x, w, y_hi, y_lo, N, H, W, Cin, Cout, in_stride, in_coff=0, out_stride=None, out_coff=0,
                    bias=None, bn_partials=None, act=ACT_NONE, taps=TAPS3_FWD):
    """3x3/s1/p1 convolution on pairs: x holds the [hi | lo] planes of Cin channels each (2*Cin consecutive channels at
    in_coff), w = pack_weight_split pack [9][Cout][3*Cin]; the result leaves as y_hi / y_lo (same out_stride / out_coff)."""
    _dev(x)
    _f32(bias, "bias"); _f32(bn_partials, "bn_partials")
    if not (x.dtype == w.dtype == y_hi.dtype == y_lo.dtype):
        raise TypeError("conv3x3_precise: x, w, y must share one 16-bit dtype")
    if Cin % 64 != 0 or w.numel() != 9 * Cout * 3 * Cin:
        raise ValueError("conv3x3_precise: Cin must be a multiple of 64 and w the [9][Cout][3*Cin] split pack")
    if bn_partials is not None and bn_partials.numel() < bn_partials_numel(conv3x3_stat_rows(N, H, W, Cin, Cout, pair=True), Cout):
        raise ValueError("conv3x3_precise: bn_partials too small")
    dy, dx = _tap_arrays(taps)
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv3x3_precise", _p(x), _p(w), _p(y_hi), _p(y_lo), _p(bias), _p(bn_partials), N, H, W, 3 * Cin,
              in_stride, in_coff, 2 * Cin, Cout, Cout if out_stride is None else out_stride, out_coff, dy, dx, act,
              dt_code(x), _stream())
    if ev is not None:                       # algorithmic work of the convolution (the kernel executes 3x the MFMAs)
        TIMER.stop("conv3x3_halo_precise", ev, 2.0 * N * H * W * Cout * 9 * Cin,
                   2.0 * (N * H * W * 2 * (Cin + Cout) + 9 * 3 * Cin * Cout))


def upconv2x2_fwd_precise(x, w, bias, y_hi, y_lo, N, IH, IW, Cin, Cout, OH, OW, in_stride, in_coff=0, out_stride=None,
                          out_coff=0, ooy=0, oox=0):
    """ConvTranspose2d(k 2, s 2) on pairs: x = [hi | lo] planes (2*Cin channels at in_coff), w = pack_weight_split(transposed)
    [4][Cout][3*Cin]; output pair y_hi / y_lo (same stride / offset), e.g. the up half of both planes of a concat buffer."""
    _dev(x)
    _f32(bias, "bias")
    if not (x.dtype == w.dtype == y_hi.dtype == y_lo.dtype):
        raise TypeError("upconv2x2_fwd_precise: x, w, y must share one 16-bit dtype")
    if w.numel() != 4 * Cout * 3 * Cin:
        raise ValueError("upconv2x2_fwd_precise: w must be the [4][Cout][3*Cin] split pack")
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_upconv2x2_fwd_precise", _p(x), _p(w), _p(bias), _p(y_hi), _p(y_lo), N, IH, IW, 3 * Cin, in_stride,
              in_coff, 2 * Cin, Cout, OH, OW, Cout if out_stride is None else out_stride, out_coff, ooy, oox,
              dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("igemm_fwd_precise", ev, 2.0 * N * IH * IW * Cin * 4 * Cout,
                   2.0 * (N * IH * IW * 2 * (Cin + 4 * Cout) + 4 * 3 * Cin * Cout))


def pack_weight_segs(items):
    """Segment packs for the mixed-precision pair forward, all in ONE launch.  items: (w, pack, transposed, segs) with
    segs = [(kind, ci0, len), ...] (kind 0 = hi(w), 1 = lo(w), 2 = zeros); pack = contiguous [taps][Cout][sum len] 16-bit."""
    if not items:
        return
    descs = (_lib.GsSegPackDesc * len(items))()
    ref = items[0][1]
    for d, (w, pack, transposed, segs) in zip(descs, items):
        _dev(w)
        _f32(w, "weight")
        if pack.dtype != ref.dtype:
            raise TypeError("pack_weight_segs: all packs must share one 16-bit dtype")
        cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
        taps = w.shape[2] * w.shape[3]
        if not 1 <= len(segs) <= _lib.GS_SEG_MAX:
            raise ValueError("pack_weight_segs: 1..4 segments")
        ktot = sum(s_[2] for s_ in segs)
        if pack.numel() != taps * cout * ktot or not pack.is_contiguous() or not w.is_contiguous():
            raise ValueError("pack_weight_segs: pack must be contiguous [taps][Cout][sum of segment lengths]")
        d.w, d.pack = _p(w), _p(pack)
        d.Cout, d.Cin, d.taps, d.transposed, d.nseg = cout, cin, taps, int(transposed), len(segs)
        for j, (kind, ci0, ln) in enumerate(segs):
            d.kind[j], d.ci0[j], d.len[j] = int(kind), int(ci0), int(ln)
    _lib.call("gs_pack_weight_segs", len(items), descs, dt_code(ref), _stream())


LO_DENSE, LO_FRAGMENT = 0, 1


def conv3x3_pair_lo_layout(N, H, W, K, Cout) -> int:
    """Layout of the conv-output lo plane a conv3x3_segs launch of these dimensions (K = its K extent) may use: LO_DENSE (NHWC) or
    LO_FRAGMENT (as the lanes of the 8-wave LDS-DMA form hold the tile, include/gsseg.h) -- only for launches with statistics, no
    bias, no activation and a dense output.  Ask once per stage and pass the answer to the conv AND to the reader of y_lo."""
    return int(_lib.load().gs_conv3x3_pair_lo_layout(N, H, W, K, Cout))


def pair_lo_set_layout(mode: int = -1) -> None:
    """Process-wide: -1 automatic, 0 dense lo planes everywhere (tests and A/B runs; restore -1)."""
    _lib.call("gs_pair_lo_set_layout", int(mode))


def conv3x3_segs(x, w, y_hi, y_lo, N, H, W, K, wrap, Cin, Cout, in_stride, in_coff=0, out_stride=None, out_coff=0,
                 bias=None, bn_partials=None, act=ACT_NONE, taps=TAPS3_FWD, lo_layout=LO_DENSE):
    """3x3/s1/p1 convolution of the pair forward with a free choice of MFMA segments: the K extent (a multiple of 64,
    wrap <= K <= 2*wrap) runs over the input channels [in_coff, in_coff + wrap) of x and wraps to in_coff once; w is the
    matching pack_weight_segs pack [9][Cout][K]; Cin = the layer's channels (for the FLOP count only).  Result: pair
    y_hi / y_lo; lo_layout = LO_FRAGMENT (conv3x3_pair_lo_layout): y_lo is a plain buffer in fragment order."""
    _dev(x)
    _f32(bias, "bias"); _f32(bn_partials, "bn_partials")
    if not (x.dtype == w.dtype == y_hi.dtype == y_lo.dtype):
        raise TypeError("conv3x3_segs: x, w, y must share one 16-bit dtype")
    if K % 64 != 0 or wrap % 64 != 0 or not (wrap <= K <= 2 * wrap) or w.numel() != 9 * Cout * K:
        raise ValueError("conv3x3_segs: K / wrap must be multiples of 64 with wrap <= K <= 2*wrap and w the [9][Cout][K] pack")
    if bn_partials is not None and bn_partials.numel() < bn_partials_numel(conv3x3_stat_rows(N, H, W, Cin, Cout, pair=True), Cout):
        raise ValueError("conv3x3_segs: bn_partials too small (conv3x3_stat_rows(pair=True) rows of [2][Cout])")
    dy, dx = _tap_arrays(taps)
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv3x3_precise_lo", _p(x), _p(w), _p(y_hi), _p(y_lo), _p(bias), _p(bn_partials), N, H, W, K,
              in_stride, in_coff, wrap, Cout, Cout if out_stride is None else out_stride, out_coff, dy, dx, act,
              dt_code(x), int(lo_layout), _stream())
    if ev is not None:                       # algorithmic work of the convolution (the kernel executes K / Cin times the MFMAs)
        TIMER.stop("conv3x3_halo_precise", ev, 2.0 * N * H * W * Cout * 9 * Cin,
                   2.0 * (N * H * W * 2 * (Cin + Cout) + 9 * K * Cout))


def conv3d3_segs(x, w, y_hi, y_lo, NB, D, H, W, K, wrap, Cin, Cout, in_stride, in_coff=0, bn_partials=None, wrap_to=0, bias=None,
                 act=ACT_NONE, out_stride=None, out_coff=0):
    """Conv3d(k3, p1) of the pair forward (UNet3D): conv3x3_segs with depth -- x holds `wrap` channels per voxel ([hi | lo] planes or
    a part of them), K (a multiple of 64, wrap <= K <= 2*wrap) runs over them and wraps once, w = pack_weight_segs pack
    [27][Cout][K]; Cin = the layer's channels (FLOP count only).  wrap_to: the wrapped part of K continues at this input channel (a
    multiple of 64) instead of channel 0.  Result: dense pair y_hi / y_lo [NB*D, H, W, Cout]; with out_stride / out_coff both planes are
    views written at channel out_coff of pixels of out_stride elements.  bias (fp32 [Cout]) and act run in the epilogue (the folded
    inference forward: conv + bias + ReLU write the z pair)."""
    _dev(x)
    _f32(bn_partials, "bn_partials"); _f32(bias, "bias")
    ostr = Cout if out_stride is None else out_stride
    if not (x.dtype == w.dtype == y_hi.dtype == y_lo.dtype):
        raise TypeError("conv3d3_segs: x, w, y must share one 16-bit dtype")
    if K % 64 != 0 or wrap % 64 != 0 or not (wrap <= K <= 2 * wrap) or w.numel() != 27 * Cout * K:
        raise ValueError("conv3d3_segs: K / wrap must be multiples of 64 with wrap <= K <= 2*wrap and w the [27][Cout][K] pack")
    if bn_partials is not None and bn_partials.numel() < bn_partials_numel(conv3x3_stat_rows(NB * D, H, W, K, Cout, pair=True), Cout):
        raise ValueError("conv3d3_segs: bn_partials too small (conv3x3_stat_rows(NB*D, H, W, K, Cout, pair=True) rows)")
    dz, dy, dx = _TAPS3D[1]
    ev = TIMER.start() if TIMER is not None else None
    if wrap_to:
        if wrap_to % 64 != 0 or wrap_to + (K - wrap) > wrap:
            raise ValueError("conv3d3_segs: wrap_to must be a multiple of 64 with wrap_to + K - wrap <= wrap")
        _lib.call("gs_conv3d_3x3x3_precise_to", _p(x), _p(w), _p(y_hi), _p(y_lo), _p(bias), _p(bn_partials), NB, D, H, W, K, in_stride,
                  in_coff, wrap, wrap_to, Cout, ostr, out_coff, dz, dy, dx, act, dt_code(x), _stream())
    else:
        _lib.call("gs_conv3d_3x3x3_precise", _p(x), _p(w), _p(y_hi), _p(y_lo), _p(bias), _p(bn_partials), NB, D, H, W, K, in_stride,
                  in_coff, wrap, Cout, ostr, out_coff, dz, dy, dx, act, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("conv3x3_halo_precise", ev, 2.0 * NB * D * H * W * Cout * 27 * Cin,
                   2.0 * (NB * D * H * W * 2 * (Cin + Cout) + 27 * K * Cout))


def maxpool3d_fwd_pair(z_hi, z_lo, z_stride, zp_hi, zp_lo, zp_stride, NB, D, H, W, C):
    """MaxPool3d(2) on a pair: z_hi / z_lo are views whose first element is the first channel of the plane (pixel stride z_stride);
    zp_hi / zp_lo (None: not stored) likewise with zp_stride."""
    _lib.call("gs_maxpool3d_fwd_pair", _p(z_hi), _p(z_lo), z_stride, _p(zp_hi), _p(zp_lo), zp_stride, NB, D, H, W, C,
              dt_code(z_hi), _stream())


def upsample2x_bilinear_fwd_pair(x_hi, x_lo, y_hi, y_lo, N, IH, IW, C, OH, OW, in_stride, out_stride, out_coff=0, ooy=0, oox=0):
    """bilinear x2 (align_corners=True) of a pair: views x_hi / x_lo (pixel stride in_stride) -> y_hi / y_lo (None: not stored;
    pixel stride out_stride, channel offset out_coff inside the [N,OH,OW,*] buffers, pad offset (ooy, oox))."""
    _dev(x_hi)
    _lib.call("gs_upsample2x_bilinear_fwd_pair", _p(x_hi), _p(x_lo), _p(y_hi), _p(y_lo), N, IH, IW, C, in_stride, 0, OH, OW,
              out_stride, out_coff, ooy, oox, dt_code(x_hi), _stream())


def upconv2x2_fwd_segs(x, w, bias, y_hi, y_lo, N, IH, IW, K, wrap, Cin, Cout, OH, OW, in_stride, in_coff=0, out_stride=None,
                       out_coff=0, ooy=0, oox=0):
    """ConvTranspose2d(k 2, s 2) of the pair forward with a free choice of segments (see conv3x3_segs); w = [4][Cout][K]."""
    _dev(x)
    _f32(bias, "bias")
    if not (x.dtype == w.dtype == y_hi.dtype == y_lo.dtype):
        raise TypeError("upconv2x2_fwd_segs: x, w, y must share one 16-bit dtype")
    if w.numel() != 4 * Cout * K or not (wrap <= K <= 2 * wrap):
        raise ValueError("upconv2x2_fwd_segs: w must be the [4][Cout][K] pack, wrap <= K <= 2*wrap")
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_upconv2x2_fwd_precise", _p(x), _p(w), _p(bias), _p(y_hi), _p(y_lo), N, IH, IW, K, in_stride,
              in_coff, wrap, Cout, OH, OW, Cout if out_stride is None else out_stride, out_coff, ooy, oox,
              dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("igemm_fwd_precise", ev, 2.0 * N * IH * IW * Cin * 4 * Cout,
                   2.0 * (N * IH * IW * 2 * (Cin + 4 * Cout) + 4 * K * Cout))


def conv_smallcin_fwd_split(x, w, y_hi, y_lo, bn_partials, k, pad):
    """First conv (fp32 NCHW image, fp32 weights, stride 1) -> dense pair y_hi / y_lo [N,H,W,Cout]."""
    _dev(x)
    _f32(x, "x"); _f32(w, "w"); _f32(bn_partials, "bn_partials")
    N, Cin, H, W = x.shape
    Cout = y_hi.shape[3]
    if tuple(y_hi.shape) != (N, H, W, Cout) or y_lo.shape != y_hi.shape or not (y_hi.is_contiguous() and y_lo.is_contiguous()):
        raise ValueError("conv_smallcin_fwd_split: y_hi / y_lo must be dense [N,H,W,Cout]")
    _lib.call("gs_conv_smallcin_fwd_split", _p(x), _p(w), _p(y_hi), _p(y_lo), _p(bn_partials), N, Cin, H, W, Cout, k, pad,
              dt_code(y_hi), _stream())


def conv_widecin_mtiles(N, H, W) -> int:
    """BatchNorm partial rows conv_widecin_fwd_split writes: one per 8 x 32 pixel patch."""
    return _lib.load().gs_conv_widecin_mtiles(N, H, W)


def conv_widecin_fwd_split(x, w, y_hi, y_lo, bn_partials=None):
    """First 3x3 conv (pad 1) on an fp32 NCHW image of 1..64 channels with fp32 weights [Cout,Cin,3,3], Cout in {32, 64, 96, 128}
    -> dense pair y_hi / y_lo [N,H,W,Cout]; bn_partials: None or conv_widecin_mtiles(N,H,W) * 2 * Cout floats."""
    _dev(x)
    _f32(x, "x"); _f32(w, "w")
    N, Cin, H, W = x.shape
    Cout = y_hi.shape[3]
    if tuple(y_hi.shape) != (N, H, W, Cout) or y_lo.shape != y_hi.shape or not (y_hi.is_contiguous() and y_lo.is_contiguous()):
        raise ValueError("conv_widecin_fwd_split: y_hi / y_lo must be dense [N,H,W,Cout]")
    if tuple(w.shape) != (Cout, Cin, 3, 3) or not (x.is_contiguous() and w.is_contiguous()):
        raise ValueError("conv_widecin_fwd_split: x dense [N,Cin,H,W], w dense [Cout,Cin,3,3]")
    if bn_partials is not None:
        _f32(bn_partials, "bn_partials")
        if bn_partials.numel() < conv_widecin_mtiles(N, H, W) * 2 * Cout:
            raise ValueError("conv_widecin_fwd_split: bn_partials needs conv_widecin_mtiles(N,H,W) * 2 * Cout floats")
    rc = _lib.load().gs_conv_widecin_fwd_split(_p(x), _p(w), _p(y_hi), _p(y_lo), _p(bn_partials), N, Cin, H, W, Cout,
                                               dt_code(y_hi), _stream())
    if rc == _lib.GS_EUNSUPPORTED:
        raise NotImplementedError(f"conv_widecin_fwd_split: Cin={Cin} (1..64) / Cout={Cout} (32, 64, 96, 128) not covered")
    _lib.check(rc, "gs_conv_widecin_fwd_split")


def bn_act_apply_split(y_hi, y_lo, scale, shift, act, z_hi, z_lo, z_stride, z_coff, zp_hi=None, zp_lo=None, zp_stride=0,
                       lo_layout=LO_DENSE):
    """z pair = act(scale * (y_hi + y_lo) + shift); y_hi / y_lo dense [N,H,W,C] (lo_layout = LO_FRAGMENT: y_lo as conv3x3_segs wrote
    it in that layout); optional 2x2 max-pooled pair."""
    N, H, W, C = y_hi.shape
    if not (y_hi.is_contiguous() and y_lo.is_contiguous()) or y_lo.shape != y_hi.shape:
        raise ValueError("bn_act_apply_split: y_hi / y_lo must be dense NHWC of one shape")
    _f32(scale, "scale"); _f32(shift, "shift")
    _lib.call("gs_bn_act_apply_split_lo", _p(y_hi), _p(y_lo), _p(scale), _p(shift), act, _p(z_hi), _p(z_lo), z_stride, z_coff,
              _p(zp_hi), _p(zp_lo), zp_stride, N, H, W, C, dt_code(y_hi), int(lo_layout), _stream())


def bn_act_apply_split_pool3d(y_hi, y_lo, scale, shift, act, z_hi, z_lo, z_stride, z_coff, zp_hi, zp_lo, zp_stride, NB, D, H, W):
    """bn_act_apply_split + MaxPool3d(2) of the pair in one pass: y_hi / y_lo dense [NB*D,H,W,C]; z pair as bn_act_apply_split; the
    pooled pair zp_hi / zp_lo (views of the first channel of each plane, pixel stride zp_stride) = the maximum of the stored pair values."""
    C = y_hi.shape[3]
    if tuple(y_hi.shape) != (NB * D, H, W, C) or y_lo.shape != y_hi.shape or not (y_hi.is_contiguous() and y_lo.is_contiguous()):
        raise ValueError("bn_act_apply_split_pool3d: y_hi / y_lo must be dense [NB*D,H,W,C]")
    _f32(scale, "scale"); _f32(shift, "shift")
    _lib.call("gs_bn_act_apply_split_pool3d", _p(y_hi), _p(y_lo), _p(scale), _p(shift), act, _p(z_hi), _p(z_lo), z_stride, z_coff,
              _p(zp_hi), _p(zp_lo), zp_stride, NB, D, H, W, C, dt_code(y_hi), _stream())


def head1x1_bn_fwd_split(y_hi, y_lo, scale, shift, act, w, bias, logits, lo_layout=LO_DENSE):
    """OutConv 1x1 on act(scale * (y_hi + y_lo) + shift) of a dense conv-output pair [N,H,W,64] -> fp32 NCHW logits
    (lo_layout = LO_FRAGMENT: y_lo in fragment order, 1..4 classes)."""
    _dev(y_hi)
    _f32(scale, "scale"); _f32(shift, "shift"); _f32(w, "w"); _f32(bias, "bias"); _f32(logits, "logits")
    N, H, W, C = y_hi.shape
    ncls = logits.shape[1]
    if (C != 64 or y_lo.shape != y_hi.shape or tuple(logits.shape) != (N, ncls, H, W) or w.numel() != ncls * 64
            or not 1 <= ncls <= 64 or (bias is not None and bias.numel() != ncls)
            or not (y_hi.is_contiguous() and y_lo.is_contiguous() and logits.is_contiguous())):
        raise ValueError("head1x1_bn_fwd_split: y pair [N,H,W,64] dense, logits [N,ncls,H,W] with 1..64 classes, w [ncls,64]")
    _lib.call("gs_head1x1_bn_fwd_split_lo", _p(y_hi), _p(y_lo), _p(scale), _p(shift), act, _p(w), _p(bias), _p(logits), N, H, W, 64,
              ncls, dt_code(y_hi), int(lo_layout), _stream())


def head1x1_fwd_split(x_hi, x_lo, w, bias, y):
    """OutConv 1x1 on a dense pair [N,H,W,64] -> fp32 NCHW logits, 1..64 classes (more than four: one launch of the wide kernel)."""
    _dev(x_hi)
    _f32(w, "w"); _f32(bias, "bias"); _f32(y, "y")
    N, H, W, Cin = x_hi.shape
    if not (x_hi.is_contiguous() and x_lo.is_contiguous()) or x_lo.shape != x_hi.shape:
        raise ValueError("head1x1_fwd_split: x_hi / x_lo must be dense NHWC of one shape")
    ncls = y.shape[1]
    if (tuple(y.shape) != (N, ncls, H, W) or not 1 <= ncls <= 64 or w.numel() != ncls * Cin
            or (bias is not None and bias.numel() != ncls)):
        raise ValueError("head1x1_fwd_split: logits [N,ncls,H,W] with 1..64 classes, w [ncls,Cin], bias [ncls]")
    _lib.call("gs_head1x1_fwd_split", _p(x_hi), _p(x_lo), _p(w), _p(bias), _p(y), N, H, W, Cin, y.shape[1], dt_code(x_hi),
              _stream())


def head1x1_wide_fwd(x, w, bias, y):
    """OutConv 1x1 on ONE dense 16-bit plane [N,H,W,64] -> fp32 NCHW logits, 1..64 classes in one launch (the 16-bit engines' head)."""
    _dev(x)
    _f32(w, "w"); _f32(bias, "bias"); _f32(y, "y")
    N, H, W, Cin = x.shape
    ncls = y.shape[1]
    if (Cin != 64 or not x.is_contiguous() or not y.is_contiguous() or tuple(y.shape) != (N, ncls, H, W) or not 1 <= ncls <= 64
            or w.numel() != ncls * 64 or (bias is not None and bias.numel() != ncls)):
        raise ValueError("head1x1_wide_fwd: x [N,H,W,64] dense, logits [N,ncls,H,W] with 1..64 classes, w [ncls,64], bias [ncls]")
    _lib.call("gs_head1x1_wide_fwd", _p(x), _p(w), _p(bias), _p(y), N, H, W, ncls, dt_code(x), _stream())


def head1x1_labels(x_hi, x_lo, w, bias, labels, scale=None, shift=None, act=ACT_NONE, lo_layout=LO_DENSE):
    """Labels straight from the pair head (GenSeg-3D/train_unet.py:39, unet/evaluate.py:29-40): x_hi / x_lo dense pair [..., 64]
    (scale / shift / act: BatchNorm + activation on the load path, x = a conv-output pair), w [ncls,64], 1..64 classes -> labels uint8,
    one per pixel in the order of the input pixels.  One class: sigmoid > 0.5; several: the first maximum.  No logits are stored."""
    _dev(x_hi)
    _f32(w, "w"); _f32(bias, "bias"); _f32(scale, "scale"); _f32(shift, "shift")
    M = x_hi.numel() // 64
    ncls = w.numel() // 64
    if (x_hi.shape[-1] != 64 or x_lo.shape != x_hi.shape or x_lo.dtype != x_hi.dtype or not (x_hi.is_contiguous() and x_lo.is_contiguous())
            or labels.dtype != torch.uint8 or labels.numel() != M or not labels.is_contiguous() or w.numel() != ncls * 64
            or not w.is_contiguous() or (bias is not None and bias.numel() != ncls) or (scale is None) != (shift is None)):
        raise ValueError("head1x1_labels: x pair [...,64] dense of one 16-bit dtype, labels uint8 with one byte per pixel, w [ncls,64], "
                         "bias [ncls], scale / shift together")
    if lo_layout != LO_DENSE:                # x_lo in fragment order: the image dimensions matter ([N,H,W,64] pair, 1..4 classes)
        if x_hi.dim() != 4:
            raise ValueError("head1x1_labels: a fragment-order lo plane needs the pair as [N,H,W,64]")
        _lib.call("gs_head1x1_labels_lo", _p(x_hi), _p(x_lo), _p(scale), _p(shift), act, _p(w), _p(bias), _p(labels), x_hi.shape[0],
                  x_hi.shape[1], x_hi.shape[2], ncls, dt_code(x_hi), int(lo_layout), _stream())
        return
    _lib.call("gs_head1x1_labels", _p(x_hi), _p(x_lo), _p(scale), _p(shift), act, _p(w), _p(bias), _p(labels), M, ncls,
              dt_code(x_hi), _stream())


def labels_from_logits(logits, labels):
    """The same predicate on stored fp32 NCHW logits [N,C,...] -> labels uint8 [N,...] (the engines whose head is not the pair
    head); 1..256 classes."""
    _dev(logits)
    _f32(logits, "logits")
    N, C = logits.shape[0], logits.shape[1]
    HW = logits.numel() // max(N * C, 1)
    if logits.dim() < 3 or not logits.is_contiguous() or labels.dtype != torch.uint8 or labels.numel() != N * HW or not labels.is_contiguous():
        raise ValueError("labels_from_logits: logits dense fp32 [N,C,...], labels uint8 with one byte per pixel")
    _lib.call("gs_labels_from_logits", _p(logits), _p(labels), N, C, HW, _stream())


def head1x1_wide_bwd(z, w, dl, dz, dw, db, gscale=1.0):
    """Backward of the pointwise head with 1..64 classes: dl fp32 [N,ncls,H,W] -> dz dense [N,H,W,64] 16-bit (one launch; None: not
    formed) and dw [ncls,64] / db [ncls] fp32 += gscale * their sums (per-block slabs, ordered reduction; both None: not formed).
    z: the head's stored 16-bit input [N,H,W,64] (None when dw is None)."""
    _dev(dl)
    _f32(w, "w"); _f32(dl, "dl"); _f32(dw, "dw"); _f32(db, "db")
    ref = z if z is not None else dz
    if ref is None or dl.dim() != 4:
        raise ValueError("head1x1_wide_bwd: needs z or dz, and dl [N,ncls,H,W]")
    N, H, W, Cin = ref.shape
    ncls = dl.shape[1]
    if (Cin != 64 or tuple(dl.shape) != (N, ncls, H, W) or not dl.is_contiguous() or not 1 <= ncls <= 64 or w.numel() != ncls * 64
            or any(t is not None and (tuple(t.shape) != (N, H, W, 64) or not t.is_contiguous() or t.dtype != ref.dtype) for t in (z, dz))
            or (dw is None) != (db is None) or (dw is None and dz is None) or (dw is not None and z is None)
            or (dw is not None and (dw.numel() != ncls * 64 or db.numel() != ncls or not dw.is_contiguous() or not db.is_contiguous()))):
        raise ValueError("head1x1_wide_bwd: z / dz [N,H,W,64] dense of one 16-bit dtype, dl [N,ncls,H,W] with 1..64 classes, w [ncls,64], "
                         "dw [ncls,64] and db [ncls] together (with z) or both None")
    ws = None
    if dw is not None:
        ws = torch.empty(int(_lib.load().gs_head1x1_wide_bwd_ws_floats(N, H, W, ncls)), dtype=torch.float32, device=dl.device)
    _lib.call("gs_head1x1_wide_bwd", _p(z), _p(w), _p(dl), _p(dz), _p(dw), _p(db), _p(ws), N, H, W, ncls, float(gscale),
              dt_code(ref), _stream())


# ---------------------------------------------------------------------------- "q" stages: FP8 correction segment of the pair forward
# (include/gsseg.h, csrc/common.hpp): the lo plane of a pair travels as a Q PLANE -- per 32 channels 64 bytes [lo8 | hi8] of e4m3 --
# and a conv stage runs x_hi.w_hi on the 16-bit MFMA plus ONE block-scaled e4m3 segment for x_lo.w_hi + x_hi.w_lo.
def conv3x3_q8_ok(W, Cin, Cout) -> bool:
    """does the "q" form of a 3x3 / 3x3x3 conv exist for this shape (LDS-DMA kernel: W >= 24, Cin % 64 == 0, Cout % 8 == 0)?"""
    return USE_HALO_CONV and bool(_lib.load().gs_conv3x3_q8_ok(W, Cin, Cout))


def pack_weight_q8(items):
    """items: (w fp32 [Cout][Cin][taps...], pack [taps][Cout][2*Cin] 16-bit elements = 4*Cin bytes per row, wexp int32 [Cout]); one launch."""
    if not items:
        return
    descs = (_lib.GsQ8PackDesc * len(items))()
    ref = items[0][1]
    for d, (w, pack, wexp) in zip(descs, items):
        _dev(w)
        _f32(w, "weight")
        cout, cin = w.shape[0], w.shape[1]
        taps = w.numel() // (cout * cin)
        if pack.numel() != taps * cout * 2 * cin or not pack.is_contiguous() or pack.dtype != ref.dtype:
            raise ValueError("pack_weight_q8: pack must be contiguous [taps][Cout][2*Cin] of the engine's 16-bit dtype")
        if wexp.dtype != torch.int32 or wexp.numel() != cout or not wexp.is_contiguous():
            raise ValueError("pack_weight_q8: wexp must be int32 [Cout]")
        d.w, d.pack, d.wexp, d.Cout, d.Cin, d.taps = _p(w), _p(pack), _p(wexp), cout, cin, taps
    _lib.call("gs_pack_weight_q8", len(items), descs, dt_code(ref), _stream())


def conv3x3_q8(x, w, wexp, y_hi, y_lo, N, H, W, Cin, Cout, in_stride, in_coff=0, bn_partials=None):
    """3x3/s1/p1 conv as a "q" stage: x = [hi plane (Cin) | q plane] at in_coff (pixel stride in_stride), w / wexp from pack_weight_q8;
    result: dense pair y_hi / y_lo [N,H,W,Cout]."""
    _dev(x)
    _f32(bn_partials, "bn_partials")
    if not (x.dtype == w.dtype == y_hi.dtype == y_lo.dtype == torch.float16):
        raise TypeError("conv3x3_q8: fp16 tensors only")
    if w.numel() != 9 * Cout * 2 * Cin:
        raise ValueError("conv3x3_q8: w must be the [9][Cout][2*Cin] q pack")
    if bn_partials is not None and bn_partials.numel() < bn_partials_numel(conv3x3_stat_rows(N, H, W, 2 * Cin, Cout, pair="q"), Cout):
        raise ValueError("conv3x3_q8: bn_partials too small")
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv3x3_q8", _p(x), _p(w), _p(wexp), _p(y_hi), _p(y_lo), _p(bn_partials), N, H, W, Cin, in_stride, in_coff,
              Cout, Cout, 0, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("conv3x3_halo_precise", ev, 2.0 * N * H * W * Cout * 9 * Cin,
                   2.0 * (N * H * W * 2 * (Cin + Cout) + 9 * 2 * Cin * Cout))


def conv3d3_q8(x, w, wexp, y_hi, y_lo, NB, D, H, W, Cin, Cout, in_stride, in_coff=0, bn_partials=None):
    """Conv3d(k3, p1) as a "q" stage (see conv3x3_q8); w = [27][Cout][2*Cin] q pack."""
    _dev(x)
    _f32(bn_partials, "bn_partials")
    if not (x.dtype == w.dtype == y_hi.dtype == y_lo.dtype == torch.float16):
        raise TypeError("conv3d3_q8: fp16 tensors only")
    if w.numel() != 27 * Cout * 2 * Cin:
        raise ValueError("conv3d3_q8: w must be the [27][Cout][2*Cin] q pack")
    if bn_partials is not None and bn_partials.numel() < bn_partials_numel(conv3x3_stat_rows(NB * D, H, W, 2 * Cin, Cout, pair="q"), Cout):
        raise ValueError("conv3d3_q8: bn_partials too small")
    ev = TIMER.start() if TIMER is not None else None
    _lib.call("gs_conv3d_3x3x3_q8", _p(x), _p(w), _p(wexp), _p(y_hi), _p(y_lo), _p(bn_partials), NB, D, H, W, Cin, in_stride,
              in_coff, Cout, Cout, 0, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("conv3x3_halo_precise", ev, 2.0 * NB * D * H * W * Cout * 27 * Cin,
                   2.0 * (NB * D * H * W * 2 * (Cin + Cout) + 27 * 2 * Cin * Cout))


def bn_act_apply_split_q8(y_hi, y_lo, scale, shift, act, z_hi, z_lo, z_q8, z_stride, z_coff, zp_hi=None, zp_lo=None, zp_q8=False,
                          zp_stride=0):
    """bn_act_apply_split with q planes: z_q8 / zp_q8 say whether z_lo / zp_lo are q planes (pointers at the plane's byte 0; z_coff
    selects the chunk) or 16-bit lo planes."""
    N, H, W, C = y_hi.shape
    if not (y_hi.is_contiguous() and y_lo.is_contiguous()) or y_lo.shape != y_hi.shape:
        raise ValueError("bn_act_apply_split_q8: y_hi / y_lo must be dense NHWC of one shape")
    _f32(scale, "scale"); _f32(shift, "shift")
    _lib.call("gs_bn_act_apply_split_q8", _p(y_hi), _p(y_lo), _p(scale), _p(shift), act, _p(z_hi), _p(z_lo), int(bool(z_q8)), z_stride,
              z_coff, _p(zp_hi), _p(zp_lo), int(bool(zp_q8)), zp_stride, N, H, W, C, dt_code(y_hi), _stream())


def stem_fwd_bn_pair_q8(x, w, scale, shift, act, zpair):
    """stem_fwd_bn_pair writing [hi plane (64) | q plane] into zpair [N,H,W,128]."""
    _stem_check(x, w, "stem_fwd_bn_pair_q8")
    _f32(scale, "scale"); _f32(shift, "shift")
    N, _, H, W = x.shape
    if tuple(zpair.shape) != (N, H, W, 128) or not zpair.is_contiguous():
        raise ValueError("stem_fwd_bn_pair_q8: zpair must be dense [N,H,W,128]")
    _lib.call("gs_stem_fwd_bn_pair_q8", _p(x), _p(w), _p(scale), _p(shift), act, _p(zpair), _p(zpair[..., 64:]), 128, N, H, W,
              dt_code(zpair), _stream())


def q8_from_hi(buf, q_plane, pixels, C, pix_stride, coff):
    """q plane (hi8 from the stored hi plane, lo8 = 0) of channels [coff, coff + C) of a buffer whose hi plane starts at `buf` and
    whose q plane starts at `q_plane` (both with pixel stride pix_stride 16-bit elements)."""
    _dev(buf)
    _lib.call("gs_q8_from_hi", _p(buf), _p(q_plane), int(pixels), C, pix_stride, coff, dt_code(buf), _stream())


def maxpool3d_fwd_pair_q8(z_hi, z_lo, z_q8, zq_coff, z_stride, zp_hi, zp_lo, zp_q8, zp_stride, NB, D, H, W, C):
    """maxpool3d_fwd_pair with q planes: z_q8 -> z_lo is the input buffer's q plane (byte 0), the pooled channels start at its channel
    zq_coff; zp_q8 -> zp_lo is the pooled buffer's q plane."""
    _lib.call("gs_maxpool3d_fwd_pair_q8", _p(z_hi), _p(z_lo), int(bool(z_q8)), zq_coff, z_stride, _p(zp_hi), _p(zp_lo), int(bool(zp_q8)),
              zp_stride, NB, D, H, W, C, dt_code(z_hi), _stream())


# ---------------------------------------------------------------------------- image-side convs of images and volumes (csrc/ends_img.hip)
def _img_shapes(who, x_shape, w, t16, k, stride, pad, rank):
    """(N, Cin, IH, IW, Cout, OH, OW) of an image (rank 2) or (N, Cin, ID, IH, IW, Cout, OD, OH, OW) of a volume (rank 3), in the order
    of the C ABI's arguments"""
    if len(x_shape) != rank + 2:
        raise ValueError(f"{who}: the {'volume must be [N,Cin,D,H,W]' if rank == 3 else 'image must be [N,Cin,H,W]'}, "
                         f"got {tuple(x_shape)}")
    N, Cin, *isz = x_shape
    od = [conv_out_size(i, k, stride, pad) for i in isz[:-2]]                # [OD] of a volume, [] of an image
    if t16.dim() != 4 or not t16.is_contiguous() or t16.shape[0] != (N * od[0] if od else N):
        raise ValueError(f"{who}: the 16-bit tensor must be dense [{'N*OD' if od else 'N'},OH,OW,Cout]")
    _, OH, OW, Cout = t16.shape
    if tuple(w.shape) != (Cout, Cin) + (k,) * len(isz):
        raise ValueError(f"{who}: w must be [Cout={Cout}, Cin={Cin}, {', '.join([str(k)] * len(isz))}], got {tuple(w.shape)}")
    return (N, Cin, *isz, Cout, *od, OH, OW)


def _call_or_unsupported(name, what, *args):
    """a C ABI call whose GS_EUNSUPPORTED becomes a NotImplementedError naming what is not covered"""
    rc = getattr(_lib.load(), name)(*args)
    if rc == _lib.GS_EUNSUPPORTED:
        raise NotImplementedError(f"{name}: {what} not covered")
    _lib.check(rc, name)


def _img_call(name, ptrs, dims, k, stride, pad, *tail):
    """name(*ptrs, *dims, k, stride, pad, *tail, stream) with dims as _img_shapes returns them"""
    Cin, Cout = dims[1], dims[len(dims) // 2 + 1]
    what = (f"Cin={Cin} ({'5..16' if len(dims) == 7 else '1..16'}), Cout={Cout} (a multiple of 8 up to 128), "
            f"k/stride/pad={k}/{stride}/{pad} (4/2/1 or 1/1/0)")
    _call_or_unsupported(name, what, *[_p(t) for t in ptrs], *dims, k, stride, pad, *tail, _stream())


def _img_wgrad_ws(who, ws, dev, *sizes):
    """the weight gradient's slab workspace: allocated when ws is None, else checked against gs_<who>_ws_floats(*sizes)"""
    need = int(getattr(_lib.load(), f"gs_{who}_ws_floats")(*sizes))
    if ws is None:
        return torch.empty(need, dtype=torch.float32, device=dev)
    if ws.numel() < need:
        raise ValueError(f"{who}: ws needs gs_{who}_ws_floats floats")
    return ws


def conv_imgwide_fwd(x, w, bias, y, k, stride, pad, act=ACT_NONE):
    """y [N,OH,OW,Cout] 16-bit = act(conv(x fp32 [N,Cin,IH,IW], w fp32 [Cout,Cin,k,k]) + bias), Cin 5..16; act ACT_NONE / ACT_LEAKY02."""
    _dev(x)
    _f32(x, "x"); _f32(w, "w"); _f32(bias, "bias")
    dims = _img_shapes("conv_imgwide_fwd", x.shape, w, y, k, stride, pad, 2)
    _img_call("gs_conv_imgwide_fwd", (x, w, bias, y), dims, k, stride, pad, act, dt_code(y))


def conv_imgwide_wgrad_ws(N, OH, OW, Cin, Cout, k, dev):
    return _img_wgrad_ws("conv_imgwide_wgrad", None, dev, N, OH, OW, Cin, Cout, k)


def conv_imgwide_wgrad(x, dy, dw, k, stride, pad, gscale, ws=None):
    """dw fp32 [Cout,Cin,k,k] = gscale * sum dy * x (overwrites; deterministic slab reduction)."""
    _dev(x)
    _f32(x, "x"); _f32(dw, "dw"); _f32(ws, "ws")
    dims = N, Cin, IH, IW, Cout, OH, OW = _img_shapes("conv_imgwide_wgrad", x.shape, dw, dy, k, stride, pad, 2)
    ws = _img_wgrad_ws("conv_imgwide_wgrad", ws, x.device, N, OH, OW, Cin, Cout, k)
    _img_call("gs_conv_imgwide_wgrad", (x, dy, dw, ws), dims, k, stride, pad, float(gscale), dt_code(dy))


def conv_imgwide_dgrad(dy, w, dx, k, stride, pad, gscale):
    """dx fp32 [N,Cin,IH,IW] = gscale * conv_transpose(dy, w) (overwrites)."""
    _dev(dy)
    _f32(w, "w"); _f32(dx, "dx")
    dims = _img_shapes("conv_imgwide_dgrad", dx.shape, w, dy, k, stride, pad, 2)
    _img_call("gs_conv_imgwide_dgrad", (dy, w, dx), dims, k, stride, pad, float(gscale), dt_code(dy))


def conv3d_img_fwd(x, w, bias, y, k, stride, pad, act=ACT_NONE):
    """y [N*OD,OH,OW,Cout] 16-bit = act(conv3d(x fp32 [N,Cin,D,H,W], w fp32 [Cout,Cin,k,k,k]) + bias), Cin 1..16; act ACT_NONE /
    ACT_LEAKY02."""
    _dev(x)
    _f32(x, "x"); _f32(w, "w"); _f32(bias, "bias")
    dims = _img_shapes("conv3d_img_fwd", x.shape, w, y, k, stride, pad, 3)
    _img_call("gs_conv3d_img_fwd", (x, w, bias, y), dims, k, stride, pad, act, dt_code(y))


def conv3d_img_wgrad_ws(N, OD, OH, OW, Cin, Cout, k, dev):
    return _img_wgrad_ws("conv3d_img_wgrad", None, dev, N, OD, OH, OW, Cin, Cout, k)


def conv3d_img_wgrad(x, dy, dw, k, stride, pad, gscale, ws=None):
    """dw fp32 [Cout,Cin,k,k,k] = gscale * sum dy * x (overwrites; deterministic slab reduction)."""
    _dev(x)
    _f32(x, "x"); _f32(dw, "dw"); _f32(ws, "ws")
    dims = N, Cin, ID, IH, IW, Cout, OD, OH, OW = _img_shapes("conv3d_img_wgrad", x.shape, dw, dy, k, stride, pad, 3)
    ws = _img_wgrad_ws("conv3d_img_wgrad", ws, x.device, N, OD, OH, OW, Cin, Cout, k)
    _img_call("gs_conv3d_img_wgrad", (x, dy, dw, ws), dims, k, stride, pad, float(gscale), dt_code(dy))


def conv3d_img_dgrad(dy, w, dx, k, stride, pad, gscale):
    """dx fp32 [N,Cin,D,H,W] = gscale * conv_transpose3d(dy, w) (overwrites)."""
    _dev(dy)
    _f32(w, "w"); _f32(dx, "dx")
    dims = _img_shapes("conv3d_img_dgrad", dx.shape, w, dy, k, stride, pad, 3)
    _img_call("gs_conv3d_img_dgrad", (dy, w, dx), dims, k, stride, pad, float(gscale), dt_code(dy))


# ---------------------------------------------------------------------------- one-channel head of the 3-D discriminators (csrc/ends3d.hip)
def _head3d_shapes(who, t16, w, l, k, pad):
    if l.dim() != 5 or l.shape[1] != 1 or not l.is_contiguous():
        raise ValueError(f"{who}: the logits must be contiguous [N,1,OD,OH,OW]")
    N, _, OD, OH, OW = l.shape
    D = OD - 2 * pad + k - 1
    if t16.dim() != 4 or not t16.is_contiguous() or t16.shape[0] != N * D:
        raise ValueError(f"{who}: the 16-bit tensor must be dense [N*D,H,W,Cin]")
    _, H, W, Cin = t16.shape
    if tuple(w.shape) != (1, Cin, k, k, k):
        raise ValueError(f"{who}: w must be [1, Cin={Cin}, {k}, {k}, {k}], got {tuple(w.shape)}")
    return N, D, H, W, Cin, OD, OH, OW


def _head3d_call(name, Cin, k, pad, *args):
    _call_or_unsupported(name, f"Cin={Cin} (a multiple of 8 up to 1024), k/pad={k}/{pad} (4/1 or 1/0)", *args)


def conv3d_head_fwd(x, w, bias, y, k, pad):
    """logits y fp32 [N,1,OD,OH,OW] = conv3d(x 16-bit [N*D,H,W,Cin], w fp32 [1,Cin,k,k,k], stride 1) + bias."""
    _dev(x)
    _f32(w, "w"); _f32(bias, "bias"); _f32(y, "y")
    N, D, H, W, Cin, OD, OH, OW = _head3d_shapes("conv3d_head_fwd", x, w, y, k, pad)
    _head3d_call("gs_conv3d_head_fwd", Cin, k, pad, _p(x), _p(w), _p(bias), _p(y), N, D, H, W, Cin, OD, OH, OW, k, pad, dt_code(x),
                 _stream())


def conv3d_head_bwd(x, w, dl, dz, dw, db, k, pad, gscale=1.0, ws=None):
    """dl fp32 [N,1,OD,OH,OW] -> dz 16-bit [N*D,H,W,Cin] (or None); dw [1,Cin,k,k,k] and db [1] += gscale * sums (or both None)."""
    _f32(w, "w"); _f32(dl, "dl"); _f32(dw, "dw"); _f32(db, "db"); _f32(ws, "ws")
    ref = x if x is not None else dz
    _dev(ref)
    N, D, H, W, Cin, OD, OH, OW = _head3d_shapes("conv3d_head_bwd", ref, w, dl, k, pad)
    if dw is not None:
        need = int(_lib.load().gs_conv3d_head_bwd_ws_floats(N, OD, OH, OW, Cin, k))
        if ws is None:
            ws = torch.empty(need, dtype=torch.float32, device=ref.device)
        elif ws.numel() < need:
            raise ValueError("conv3d_head_bwd: ws needs gs_conv3d_head_bwd_ws_floats floats")
    _head3d_call("gs_conv3d_head_bwd", Cin, k, pad, _p(x), _p(w), _p(dl), _p(dz), _p(dw), _p(db), _p(ws), N, D, H, W, Cin, OD, OH, OW,
                 k, pad, float(gscale), dt_code(ref), _stream())


# ---------------------------------------------------------------------------- 3-D Pix2Pix cells (csrc/cell3d.hip)
# The mixed stride-2 Conv3d cell as a 64-tap stride-1 conv over the parity-gathered volume, and the linear additive upsample.
def cell3d_gathered_size(d: int) -> int:
    """entries per axis of the gathered tensor x'[a] = x[2a + p - 1]: ceil((d + 1) / 2)"""
    return d // 2 + 1


def cell3d_reachable_taps(d: int):
    """taps kz of the 8 / stride 2 / pad 3 conv that meet data on an axis of d entries: some output o has 0 <= 2o + kz - 3 < d"""
    return [kz for kz in range(8) if any(0 <= 2 * o + kz - 3 < d for o in range(d // 2))]


def cell3d_boxes(D: int, H: int, W: int, full: bool = False):
    """(dt0, nd, k0, nk): per axis, the box of gathered taps dt = (k >> 1) - 1 in -1..2 and the box of taps k in 0..7 that can meet
    data (full=True: all of them).  Taps outside never multiply anything but padding; packs and launches leave them out."""
    dt0, nd, k0, nk = [], [], [], []
    for d in (D, H, W):
        ks = list(range(8)) if full else cell3d_reachable_taps(d)
        if not ks:
            raise NotImplementedError("mixed Conv3d cell: every spatial size must be >= 2")
        lo, hi = (ks[0] >> 1) - 1, (ks[-1] >> 1) - 1
        dt0.append(lo); nd.append(hi - lo + 1); k0.append(ks[0]); nk.append(len(ks))
    return tuple(dt0), tuple(nd), tuple(k0), tuple(nk)


def _i3(v):
    return (ctypes.c_int32 * 3)(*[int(i) for i in v])


def _cell3d_call(name, *args):
    rc = getattr(_lib.load(), name)(*args)
    if rc == _lib.GS_EUNSUPPORTED:
        msg = _lib.load().gs_last_error()
        raise NotImplementedError(msg.decode() if msg else name)
    _lib.check(rc, name)


def geom_cell3d_fwd(N, D, H, W, Cin, Cout, dt0, nd, **kw) -> GsConvGeom:
    """the mixed cell over the gathered tensor x' [N*GD,GH,GW,8 Cin]: stride 1, taps dt of the box in (z, y, x) row-major order =
    the order of the forward pack and of the weight gradient [taps][Cout][8 Cin]"""
    GD, GH, GW = cell3d_gathered_size(D), cell3d_gathered_size(H), cell3d_gathered_size(W)
    OD, OH, OW = D // 2, H // 2, W // 2
    t3 = [(dt0[0] + a, dt0[1] + b, dt0[2] + c) for a in range(nd[0]) for b in range(nd[1]) for c in range(nd[2])]
    return make_geom(N, GH, GW, 8 * Cin, OH, OW, Cout, OH, OW, [(y, x) for (_, y, x) in t3], tap_dz=[z for (z, _, _) in t3],
                     Dg=OD, Din=GD, Dout=OD, **kw)


def geom_cell3d_dgrad_class(N, D, H, W, Cin, Cout, k0, nk, pz, py, px, **kw):
    """geom_conv3d_s2_dgrad_class(k=8, pad=3) restricted to the tap box k0 .. k0 + nk of a compact [nk taps][Cin][Cout] pack; None
    when no tap of the class lies in the box (the class's voxels then receive no gradient: the caller zero-fills dx)"""
    OD, OH, OW = D // 2, H // 2, W // 2
    sel = [(kz, ky, kx) for kz in range(k0[0], k0[0] + nk[0]) for ky in range(k0[1], k0[1] + nk[1]) for kx in range(k0[2], k0[2] + nk[2])
           if (pz + 3 - kz) % 2 == 0 and (py + 3 - ky) % 2 == 0 and (px + 3 - kx) % 2 == 0]
    dg, ihg, iwg = (D - pz + 1) // 2, (H - py + 1) // 2, (W - px + 1) // 2
    if not sel or dg <= 0 or ihg <= 0 or iwg <= 0:
        return None
    taps = [((py + 3 - ky) // 2, (px + 3 - kx) // 2) for (_, ky, kx) in sel]
    dz = [(pz + 3 - kz) // 2 for (kz, _, _) in sel]
    slots = [((kz - k0[0]) * nk[1] + ky - k0[1]) * nk[2] + kx - k0[2] for (kz, ky, kx) in sel]
    return make_geom(N, OH, OW, Cout, ihg, iwg, Cin, H, W, taps, osy=2, osx=2, ooy=py, oox=px, tap_w=slots, tap_dz=dz,
                     Dg=dg, Din=OD, Dout=D, osz=2, ooz=pz, **kw)


def cell3d_gather(src, out, N, D, H, W, Cin, in_stride=None, in_coff=0):
    """src: 16-bit [N*D,H,W,*] (Cin % 8 == 0, channel slice in_coff .. in_coff + Cin of in_stride) or an fp32 NCDHW volume with Cin
    1..4 -> out 16-bit [N*GD,GH,GW,8 Cin], out[a,(pz,py,px,c)] = src[2a+pz-1, 2i+py-1, 2j+px-1, c], zero outside the volume."""
    _dev(src)
    need = N * cell3d_gathered_size(D) * cell3d_gathered_size(H) * cell3d_gathered_size(W) * 8 * Cin
    if out.numel() != need or not out.is_contiguous():
        raise ValueError("cell3d_gather: out must be dense [N*GD,GH,GW,8*Cin]")
    if src.dtype == torch.float32:
        if tuple(src.shape) != (N, Cin, D, H, W) or not src.is_contiguous():
            raise ValueError("cell3d_gather: an fp32 source is a contiguous [N,Cin,D,H,W] volume")
        _cell3d_call("gs_cell3d_gather", None, _p(src), _p(out), N, D, H, W, Cin, 0, 0, dt_code(out), _stream())
        return
    if src.dtype != out.dtype:
        raise TypeError("cell3d_gather: a 16-bit source and out must share one dtype")
    stride = Cin if in_stride is None else in_stride
    if src.numel() < N * D * H * W * stride:
        raise ValueError("cell3d_gather: the source is smaller than [N*D,H,W,in_stride]")
    _cell3d_call("gs_cell3d_gather", _p(src), None, _p(out), N, D, H, W, Cin, stride, in_coff, dt_code(out), _stream())


def cell3d_merge_pack(w4, w6, w8, softmax3, pack_fwd=None, pack_dgrad=None, dt0=(-1, -1, -1), nd=(4, 4, 4), k0=(0, 0, 0),
                      nk=(8, 8, 8), cin_pad=None):
    """(sm0 w4 + sm1 w6) + sm2 w8 (k4 embedded at offset 2, k6 at 1) -> pack_fwd [prod(nd)][Cout][8 Cin] and / or pack_dgrad
    [prod(nk)][cin_pad][Cout], each over its tap box, rounded once."""
    _dev(w8)
    for n, t in (("w4", w4), ("w6", w6), ("w8", w8), ("softmax3", softmax3)):
        _f32(t, n)
    Cout, Cin = w8.shape[0], w8.shape[1]
    if tuple(w4.shape) != (Cout, Cin, 4, 4, 4) or tuple(w6.shape) != (Cout, Cin, 6, 6, 6) or tuple(w8.shape) != (Cout, Cin, 8, 8, 8) \
            or softmax3.numel() != 3:
        raise ValueError("cell3d_merge_pack: w4 / w6 / w8 are [Cout][Cin][k][k][k] for k = 4, 6, 8; softmax3 has 3 entries")
    cin_pad = (Cin + 7) // 8 * 8 if cin_pad is None else cin_pad
    ref = pack_fwd if pack_fwd is not None else pack_dgrad
    if ref is None:
        raise ValueError("cell3d_merge_pack: no pack to write")
    if pack_fwd is not None and (pack_fwd.numel() != nd[0] * nd[1] * nd[2] * Cout * 8 * Cin or not pack_fwd.is_contiguous()):
        raise ValueError("cell3d_merge_pack: pack_fwd must be dense [prod(nd)][Cout][8*Cin]")
    if pack_dgrad is not None and (pack_dgrad.numel() != nk[0] * nk[1] * nk[2] * cin_pad * Cout or not pack_dgrad.is_contiguous()
                                   or pack_dgrad.dtype != ref.dtype):
        raise ValueError("cell3d_merge_pack: pack_dgrad must be dense [prod(nk)][cin_pad][Cout] of the forward pack's dtype")
    _cell3d_call("gs_cell3d_merge_pack", _p(w4), _p(w6), _p(w8), _p(softmax3), _p(pack_fwd), _p(pack_dgrad), Cin, Cout, cin_pad,
                 _i3(dt0), _i3(nd), _i3(k0), _i3(nk), dt_code(ref), _stream())


def cell3d_split_wgrad(dwm, w4, w6, w8, softmax3, gscale, dw4, dw6, dw8, dots3, dt0=(-1, -1, -1), nd=(4, 4, 4)):
    """merged weight gradient fp32 [prod(nd)][Cout][8 Cin] -> dw4 / dw6 / dw8 (gscale * sm_j * centred crop) and
    dots3[j] = gscale * <dwm, embed(w_j)>; deterministic."""
    _dev(dwm)
    for n, t in (("dwm", dwm), ("w4", w4), ("w6", w6), ("w8", w8), ("softmax3", softmax3), ("dw4", dw4), ("dw6", dw6), ("dw8", dw8),
                 ("dots3", dots3)):
        _f32(t, n)
    Cout, Cin = w8.shape[0], w8.shape[1]
    if dwm.numel() != nd[0] * nd[1] * nd[2] * Cout * 8 * Cin or dots3.numel() != 3 or any(
            a.shape != b.shape for a, b in ((dw4, w4), (dw6, w6), (dw8, w8))):
        raise ValueError("cell3d_split_wgrad: dwm is [prod(nd)][Cout][8*Cin]; dw_j has the shape of w_j; dots3 has 3 entries")
    ws = torch.empty(max(int(_lib.load().gs_cell3d_split_wgrad_ws_floats(Cin, Cout)), 1), dtype=torch.float32, device=dwm.device)
    _cell3d_call("gs_cell3d_split_wgrad", _p(dwm), _p(w4), _p(w6), _p(w8), _p(softmax3), float(gscale), _p(dw4), _p(dw6), _p(dw8),
                 _p(dots3), _p(ws), Cin, Cout, _i3(dt0), _i3(nd), _stream())


def upsample_add3d_fwd(x, y, N, D, H, W, C, in_stride=None, in_coff=0, out_stride=None, out_coff=0):
    """x 16-bit [N*D,H,W,C] -> y [N*2D,2H,2W,C/4]: trilinear x2 (align_corners=False) of the sum of each 4 consecutive channels."""
    _dev(x)
    if x.dtype != y.dtype:
        raise TypeError("upsample_add3d_fwd: x and y must share one 16-bit dtype")
    xs, ys = C if in_stride is None else in_stride, C // 4 if out_stride is None else out_stride
    if x.numel() < N * D * H * W * xs or y.numel() < 8 * N * D * H * W * ys:
        raise ValueError("upsample_add3d_fwd: tensors smaller than [N*D,H,W,in_stride] / [N*2D,2H,2W,out_stride]")
    ev = TIMER.start() if TIMER is not None else None
    _cell3d_call("gs_upsample_add3d_fwd", _p(x), _p(y), N, D, H, W, C, xs, in_coff, ys, out_coff, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("upsample_add3d", ev, 2.0 * N * 8 * D * H * W * (C // 4) * 8 + N * D * H * W * C * 0.75, 2.0 * N * D * H * W * C * 3)


def upsample_add3d_bwd(dy, dx, N, D, H, W, C, dy_stride=None, dy_coff=0, dx_stride=None, dx_coff=0):
    """the exact adjoint: dy 16-bit [N*2D,2H,2W,C/4] -> dx [N*D,H,W,C], the four members of a channel group alike."""
    _dev(dy)
    if dy.dtype != dx.dtype:
        raise TypeError("upsample_add3d_bwd: dy and dx must share one 16-bit dtype")
    ys, xs = C // 4 if dy_stride is None else dy_stride, C if dx_stride is None else dx_stride
    if dx.numel() < N * D * H * W * xs or dy.numel() < 8 * N * D * H * W * ys:
        raise ValueError("upsample_add3d_bwd: tensors smaller than [N*D,H,W,dx_stride] / [N*2D,2H,2W,dy_stride]")
    ev = TIMER.start() if TIMER is not None else None
    _cell3d_call("gs_upsample_add3d_bwd", _p(dy), _p(dx), N, D, H, W, C, ys, dy_coff, xs, dx_coff, dt_code(dy), _stream())
    if ev is not None:
        TIMER.stop("upsample_add3d", ev, 2.0 * N * D * H * W * (C // 4) * 64, 2.0 * N * D * H * W * C * 3)


# ---------------------------------------------------------------------------- 3-D Pix2Pix generator tail (csrc/gen3d.hip)
# Conv3d(C_in -> C_out, k 3, stride 1, pad 1) + bias + tanh from the 16-bit upsample output to the fp32 NCDHW image.
def _tail3d_shapes(who, t16, w, img):
    if img.dim() != 5 or not img.is_contiguous() or img.dtype != torch.float32:
        raise ValueError(f"{who}: the image must be a contiguous fp32 [N,C_out,D,H,W] tensor")
    N, Cout, D, H, W = img.shape
    if t16.dim() != 4 or not t16.is_contiguous() or tuple(t16.shape[:3]) != (N * D, H, W):
        raise ValueError(f"{who}: the 16-bit tensor must be dense [N*D,H,W,C_in] = [{N * D},{H},{W},C_in], got {tuple(t16.shape)}")
    Cin = t16.shape[3]
    if tuple(w.shape) != (Cout, Cin, 3, 3, 3) or not w.is_contiguous():
        raise ValueError(f"{who}: w must be contiguous [C_out={Cout}, C_in={Cin}, 3, 3, 3], got {tuple(w.shape)}")
    return N, D, H, W, Cin, Cout


def conv3d_tail_fwd(x, w, bias, out, act):
    """out fp32 [N,C_out,D,H,W] = act(conv3d(x 16-bit [N*D,H,W,C_in], w fp32 [C_out,C_in,3,3,3], stride 1, pad 1) + bias); C_in a
    multiple of 8 up to 64, C_out 1..4, act ACT_NONE / ACT_TANH."""
    _dev(x)
    _f32(w, "w"); _f32(bias, "bias")
    N, D, H, W, Cin, Cout = _tail3d_shapes("conv3d_tail_fwd", x, w, out)
    if bias is not None and bias.numel() != Cout:
        raise ValueError("conv3d_tail_fwd: bias must have C_out entries")
    ev = TIMER.start() if TIMER is not None else None
    _cell3d_call("gs_conv3d_tail_fwd", _p(x), _p(w), _p(bias), _p(out), N, D, H, W, Cin, Cout, act, dt_code(x), _stream())
    if ev is not None:
        TIMER.stop("conv3d_tail", ev, 2.0 * N * D * H * W * 27 * Cin * Cout, N * D * H * W * (2.0 * Cin + 4.0 * Cout))


def conv3d_tail_bwd(x, w, t, dout, dx, dw, db, act, gscale=1.0, ws=None):
    """du = gscale * dout * (1 - t^2) (act ACT_NONE: gscale * dout; t may be None) -> dx 16-bit [N*D,H,W,C_in] (or None), dw
    [C_out,C_in,3,3,3] and db [C_out] (fp32, overwritten, deterministic; or both None)."""
    _f32(w, "w"); _f32(t, "t"); _f32(dw, "dw"); _f32(db, "db"); _f32(ws, "ws")
    ref = x if x is not None else dx
    if ref is None:
        raise ValueError("conv3d_tail_bwd: x or dx must be given")
    _dev(ref)
    N, D, H, W, Cin, Cout = _tail3d_shapes("conv3d_tail_bwd", ref, w, dout)
    if t is not None and (tuple(t.shape) != tuple(dout.shape) or not t.is_contiguous()):
        raise ValueError("conv3d_tail_bwd: t must be contiguous with dout's shape")
    if dx is not None and (dx.dtype != ref.dtype or tuple(dx.shape) != tuple(ref.shape) or not dx.is_contiguous()):
        raise ValueError("conv3d_tail_bwd: dx must be dense [N*D,H,W,C_in] of x's dtype")
    if dw is not None:
        if db is None or tuple(dw.shape) != tuple(w.shape) or db.numel() != Cout or not dw.is_contiguous():
            raise ValueError("conv3d_tail_bwd: dw has w's shape and comes with db [C_out]")
        need = int(_lib.load().gs_conv3d_tail_bwd_ws_floats(N, D, H, W, Cin, Cout))
        if ws is None:
            ws = torch.empty(need, dtype=torch.float32, device=ref.device)
        elif ws.numel() < need:
            raise ValueError("conv3d_tail_bwd: ws needs gs_conv3d_tail_bwd_ws_floats floats")
    ev = TIMER.start() if TIMER is not None else None
    _cell3d_call("gs_conv3d_tail_bwd", _p(x), _p(w), _p(t), _p(dout), _p(dx), _p(dw), _p(db), _p(ws), N, D, H, W, Cin, Cout, act,
                 float(gscale), dt_code(ref), _stream())
    if ev is not None:
        TIMER.stop("conv3d_tail", ev, 4.0 * N * D * H * W * 27 * Cin * Cout, N * D * H * W * (4.0 * Cin + 8.0 * Cout))
