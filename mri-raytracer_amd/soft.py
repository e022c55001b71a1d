"""The soft prediction overlay: a K1 frame whose prediction-overlay event is driven by per-sample class probabilities, and the
gradient of that frame with respect to the samples' logits.

``render_brats_soft`` / ``render_brats_soft_backward`` are the ctypes paths to ``mrirt_render_brats_soft`` /
``mrirt_render_brats_soft_backward`` (csrc/brats_soft.hip), and ``render_brats_soft_autograd`` renders the frame with a
``torch.autograd`` graph to ``logits`` behind it — the link between the frame and the INR training step
(``mrirt.inr.render_brats_inr_autograd``).  LINEAR fp32 grids, unshaded, whole frames (include/mrirt.h states the contract).
The logits of sample k of pixel p = y * W + x are row ``offsets[p] + k``: the numbering of ``mrirt_brats_sample_counts`` /
``mrirt_brats_emit_samples``.  The kernels go by ``offsets`` alone and cannot see where ``logits`` ends: the caller vouches
that every ray's rows exist.  As everywhere in the package there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Mapping, Optional, Sequence

import torch

from . import _lib, torch_ops
from .params import render_ext
from .render import Grid, _alloc_out, _as_device_tensor, _bind_brats, _on_stream, _ptr, _require_gpu, _stream_ptr

MAX_CLASSES = 16


def _bind_soft(params, intensities, logits, offsets, labels, ext, dev):
    P, E, vols, lab, _, _ = _bind_brats(params, intensities, labels, None, ext, dev, pred_stream=True)
    W, H = int(P.imageSize[0]), int(P.imageSize[1])
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() != 2 \
            or not logits.is_contiguous():
        raise TypeError("logits: expected a contiguous device float32 tensor (rows, classes)")
    if not 1 <= int(logits.shape[1]) <= MAX_CLASSES:
        raise ValueError(f"logits: 1..{MAX_CLASSES} classes, got {int(logits.shape[1])}")
    if not isinstance(offsets, torch.Tensor) or not offsets.is_cuda or offsets.dtype != torch.int64 or not offsets.is_contiguous() \
            or offsets.numel() != W * H:
        raise TypeError(f"offsets: expected a contiguous device int64 tensor of {W * H} elements (one per pixel)")
    vp = (C.c_void_p * 4)(*[C.c_void_p(t.data_ptr()) if t is not None else None for t in vols])
    return P, E, vp, lab, W, H


def render_brats_soft(params: Mapping[str, Any], intensities: Sequence, logits: torch.Tensor, offsets: torch.Tensor, labels=None,
                      ext: Optional[Mapping[str, Any]] = None, out: Optional[torch.Tensor] = None, stream=None,
                      return_stats: bool = False):
    """The soft-overlay frame, fp32 (H, W, 4).  ``logits``: device fp32 (rows, C), ``offsets``: device int64 (H * W).
    ``params["showPred"]`` is ignored (the soft event takes that overlay's place).  ``return_stats``: also the number of
    composited samples (one host read)."""
    dev = _require_gpu()
    with _on_stream(stream):
        P, E, vp, lab, W, H = _bind_soft(params, intensities, logits, offsets, labels, ext, dev)
        o, pitch = _alloc_out(W, H, E, dev, out)
        st = torch.zeros(1, dtype=torch.int64, device=dev) if return_stats else None
        rc = _lib.lib().mrirt_render_brats_soft(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(logits), int(logits.shape[1]),
                                                _ptr(offsets), _ptr(o), pitch, _ptr(st), _stream_ptr(stream))
        _lib.check(rc, "mrirt_render_brats_soft")
    if return_stats:
        return o, dict(live_samples=int(st.cpu()[0]))
    return o


def render_brats_soft_backward(params: Mapping[str, Any], intensities: Sequence, logits: torch.Tensor, offsets: torch.Tensor,
                               grad_out: torch.Tensor, labels=None, ext: Optional[Mapping[str, Any]] = None,
                               out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """dL/dlogits, fp32 shaped like ``logits``, of the frame ``render_brats_soft(...)`` for the upstream ``grad_out`` =
    dL/dframe (device fp32 (H, W, 4), alpha ignored).  Every row a ray owns is overwritten; rows no ray owns keep what ``out``
    held (a fresh result is allocated zeroed)."""
    dev = _require_gpu()
    with _on_stream(stream):
        P, E, vp, lab, W, H = _bind_soft(params, intensities, logits, offsets, labels, ext, dev)
        g = grad_out
        if not isinstance(g, torch.Tensor) or not g.is_cuda or g.dtype != torch.float32 or tuple(g.shape) != (H, W, 4):
            raise TypeError(f"grad_out: expected a device float32 tensor of shape ({H}, {W}, 4)")
        if g.stride(2) != 1 or g.stride(1) != 4 or g.stride(0) % 4 != 0 or g.stride(0) < 4 * W or g.data_ptr() % 16 != 0:
            g = g.contiguous()
        if out is None:
            out = torch.zeros_like(logits)
        elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != tuple(logits.shape):
            raise TypeError("out: expected a contiguous device float32 tensor shaped like logits")
        rc = _lib.lib().mrirt_render_brats_soft_backward(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(logits), int(logits.shape[1]),
                                                         _ptr(offsets), _ptr(g), g.stride(0) // 4, _ptr(out), _stream_ptr(stream))
        _lib.check(rc, "mrirt_render_brats_soft_backward")
    return out


class _RenderBratsSoft(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, ext, labels, offsets, logits, v0, v1, v2, v3):
        blobs = (torch_ops.pack_brats_params(params), torch_ops.pack_render_ext(ext))
        z = logits.detach().contiguous()
        frame = torch.ops.mrirt.render_brats_soft(blobs[0], blobs[1], z, offsets, v0, v1, v2, v3, labels)
        ctx.blobs, ctx.held = blobs, (labels, offsets, v0, v1, v2, v3)
        ctx.save_for_backward(z)
        return frame

    @staticmethod
    def backward(ctx, grad_frame):
        (z,) = ctx.saved_tensors
        lab, offsets, v0, v1, v2, v3 = ctx.held
        dl = torch.ops.mrirt.render_brats_soft_backward(ctx.blobs[0], ctx.blobs[1], grad_frame.contiguous(), z, offsets, v0, v1, v2, v3, lab)
        return (None, None, None, None, dl, None, None, None, None)


def render_brats_soft_autograd(params: Mapping[str, Any], vols: Sequence[Optional[torch.Tensor]], logits: torch.Tensor,
                               offsets: torch.Tensor, labels=None, ext: Optional[Mapping[str, Any]] = None) -> torch.Tensor:
    """The ``render_brats_soft`` frame, fp32 (H, W, 4), with a ``torch.autograd`` graph to ``logits`` (device fp32 (rows, C)):
    the same bits as ``render_brats_soft``, backward through ``torch.ops.mrirt.render_brats_soft_backward``.  ``vols``: up to
    four device fp32 tensors of X*Y*Z voxels (fixed occluders here: ``render_brats_autograd`` differentiates them),
    ``labels``: the ground-truth overlay's int32 grid when ``showSeg``.  ``ext`` may choose the camera mode and the ERT
    threshold; layouts other than LINEAR, shading, tiles, FAST math and fp16 output are refused."""
    dev = _require_gpu()
    vols = list(vols) + [None] * (4 - len(vols))
    if len(vols) != 4:
        raise ValueError("vols: at most four modalities")
    for m, v in enumerate(vols):
        if isinstance(v, Grid):
            raise TypeError(f"vols[{m}]: pass the device tensor")
        if v is not None and (not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32 or not v.is_contiguous()):
            raise TypeError(f"vols[{m}]: expected a contiguous device float32 tensor")
    E = render_ext(dict(ext or {}))
    if E.layout != _lib.LAYOUT_LINEAR or E.labelLayout != _lib.LAYOUT_LINEAR:
        raise ValueError("render_brats_soft_autograd: LINEAR grids only")
    if E.shadeMode != 0 or E.tileSize != 0 or E.outFormat != _lib.OUT_RGBA32F or E.math != _lib.MATH_STRICT:
        raise ValueError("render_brats_soft_autograd: unshaded whole frames in STRICT math and fp32 only")
    if isinstance(labels, Grid) and labels.layout != "linear":
        raise ValueError("render_brats_soft_autograd: LINEAR label grids only")
    lab = _as_device_tensor(labels, torch.int32, dev, "gLabels")
    flat = [None if v is None else v.detach().reshape(-1) for v in vols]
    return _RenderBratsSoft.apply(dict(params), dict(ext or {}), lab, offsets, logits, *flat)
