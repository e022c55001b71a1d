"""K1 backward: how a ``render_brats`` frame changes with the voxels and with the window / level / opacity / gamma.

``render_brats_backward`` is the ctypes path to ``mrirt_render_brats_backward`` (csrc/brats_backward.hip), and
``render_brats_autograd`` renders the frame with a ``torch.autograd`` graph behind it, so a volume or a transfer function can be
fitted to target views.  LINEAR fp32 grids, unshaded, whole frames (include/mrirt.h says what is differentiated and what is a
constant).  As everywhere in the package there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, List, Mapping, Optional, Sequence, Tuple

import torch

from . import _lib, torch_ops
from .params import render_ext
from .render import Grid, _as_device_tensor, _bind_brats, _on_stream, _ptr, _require_gpu, _stream_ptr, render_brats

TF_FIELDS = ("ww", "wl", "intensityAlpha", "gamma")        # the order of grad_tf


def render_brats_backward(params: Mapping[str, Any], intensities: Sequence, grad_out: torch.Tensor, labels=None, preds=None,
                          ext: Optional[Mapping[str, Any]] = None, stream=None,
                          accumulate_into: Optional[Tuple[Sequence[Optional[torch.Tensor]], Optional[torch.Tensor]]] = None
                          ) -> Tuple[List[Optional[torch.Tensor]], torch.Tensor]:
    """Gradients of the frame ``render_brats(params, intensities, labels, preds, ext=ext)`` (LINEAR grids) for the upstream
    ``grad_out`` = dL/dframe, a device fp32 (H, W, 4) tensor whose alpha channel is ignored.

    Returns ``(grad_vols, grad_tf)``: per modality a fp32 tensor of X*Y*Z voxel gradients (``None`` for a disabled modality)
    and a float64 tensor dL/d(ww, wl, intensityAlpha, gamma).  The outputs are allocated zeroed unless ``accumulate_into =
    (grad_vols, grad_tf)`` hands in the tensors to add to (summing over views; a ``None`` entry is not computed)."""
    dev = _require_gpu()
    with _on_stream(stream):
        P, E, vols, lab, prd, _ = _bind_brats(params, intensities, labels, preds, ext, dev)
        W, H = int(P.imageSize[0]), int(P.imageSize[1])
        nvox = int(P.dims[0]) * int(P.dims[1]) * int(P.dims[2])
        g = grad_out
        if not isinstance(g, torch.Tensor) or not g.is_cuda or g.dtype != torch.float32 or tuple(g.shape) != (H, W, 4):
            raise TypeError(f"grad_out: expected a device float32 tensor of shape ({H}, {W}, 4)")
        if g.stride(2) != 1 or g.stride(1) != 4 or g.stride(0) % 4 != 0 or g.stride(0) < 4 * W or g.data_ptr() % 16 != 0:
            g = g.contiguous()
        if accumulate_into is None:
            gv = [torch.zeros(nvox, dtype=torch.float32, device=dev) if P.volEnabled[m] != 0 else None for m in range(4)]
            gtf = torch.zeros(4, dtype=torch.float64, device=dev)
        else:
            gv, gtf = list(accumulate_into[0]) + [None] * (4 - len(accumulate_into[0])), accumulate_into[1]
            for m, t in enumerate(gv):
                if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < nvox):
                    raise TypeError(f"accumulate_into: grad_vols[{m}] must be a contiguous device float32 tensor of {nvox} elements")
            if gtf is not None and (not gtf.is_cuda or gtf.dtype != torch.float64 or not gtf.is_contiguous() or gtf.numel() < 4):
                raise TypeError("accumulate_into: grad_tf must be a contiguous device float64 tensor of 4 elements")
        vp = (C.c_void_p * 4)(*[C.c_void_p(t.data_ptr()) if t is not None else None for t in vols])
        gp = (C.c_void_p * 4)(*[C.c_void_p(t.data_ptr()) if t is not None else None for t in gv])
        rc = _lib.lib().mrirt_render_brats_backward(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(prd), _ptr(g), g.stride(0) // 4,
                                                    gp, _ptr(gtf), _stream_ptr(stream))
        _lib.check(rc, "mrirt_render_brats_backward")
    return gv, gtf


class _RenderBrats(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, ext, labels, preds, tf, v0, v1, v2, v3):
        vols = [v0, v1, v2, v3]
        flat = [None if v is None else v.detach().reshape(-1) for v in vols]
        frame = render_brats(params, flat, labels, preds, ext=ext)
        ctx.blobs = (torch_ops.pack_brats_params(params), torch_ops.pack_render_ext(ext))
        ctx.held = (labels, preds)
        ctx.shapes = [None if v is None else v.shape for v in vols]
        ctx.tf_like = None if tf is None else (tf.dtype, tf.shape)
        ctx.save_for_backward(*[v for v in flat if v is not None])
        return frame

    @staticmethod
    def backward(ctx, grad_frame):
        saved = list(ctx.saved_tensors)
        flat = [None if s is None else saved.pop(0) for s in ctx.shapes]
        lab, prd = ctx.held
        gv = torch.ops.mrirt.render_brats_backward(ctx.blobs[0], ctx.blobs[1], grad_frame.contiguous(), *flat, lab, prd)
        gvols = [None if s is None or gv[m].numel() == 0 else gv[m].reshape(s) for m, s in enumerate(ctx.shapes)]
        gtf = None if ctx.tf_like is None else gv[4].to(ctx.tf_like[0]).reshape(ctx.tf_like[1])
        return (None, None, None, None, gtf, *gvols)


def render_brats_autograd(params: Mapping[str, Any], vols: Sequence[Optional[torch.Tensor]], tf: Optional[torch.Tensor] = None,
                          labels=None, preds=None, ext: Optional[Mapping[str, Any]] = None) -> torch.Tensor:
    """The ``render_brats`` frame, fp32 (H, W, 4), with a ``torch.autograd`` graph: the same bits as ``render_brats`` on LINEAR
    grids, and a backward pass (``torch.ops.mrirt.render_brats_backward``) that delivers dL/dvoxel to every ``vols[m]`` that
    requires grad and dL/d(ww, wl, intensityAlpha, gamma) to ``tf``.

    ``vols``: up to four device fp32 tensors of X*Y*Z voxels each (x fastest; any shape), ``None`` for an unused slot.  ``tf``:
    an optional device fp32 tensor ``(ww, wl, intensityAlpha, gamma)`` that overrides those four fields of ``params``; the kernels
    take them as launch constants, so reading ``tf`` to the host costs ONE synchronisation per call.  ``labels`` / ``preds`` are
    fixed occluders (int32 device tensors or LINEAR ``Grid``s).  ``ext`` may choose the camera mode and the ERT threshold; grid
    layouts other than LINEAR, shading, tiles, FAST math and fp16 output are refused."""
    dev = _require_gpu()
    vols = list(vols) + [None] * (4 - len(vols))
    if len(vols) != 4:
        raise ValueError("vols: at most four modalities")
    for m, v in enumerate(vols):
        if isinstance(v, Grid):
            raise TypeError(f"vols[{m}]: pass the device tensor (a Grid carries no graph)")
        if v is not None and (not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32 or not v.is_contiguous()):
            raise TypeError(f"vols[{m}]: expected a contiguous device float32 tensor")
    p = dict(params)
    if tf is not None:
        if not isinstance(tf, torch.Tensor) or not tf.is_cuda or not tf.is_floating_point() or tf.numel() != 4:
            raise TypeError("tf: expected a device floating-point tensor (ww, wl, intensityAlpha, gamma)")
        for k, x in zip(TF_FIELDS, tf.detach().reshape(-1).cpu().tolist()):       # the one synchronisation of the call
            p[k] = float(x)
    E = render_ext(dict(ext or {}))
    if E.layout != _lib.LAYOUT_LINEAR or E.labelLayout != _lib.LAYOUT_LINEAR:
        raise ValueError("render_brats_autograd: LINEAR grids only")
    if E.shadeMode != 0 or E.tileSize != 0 or E.outFormat != _lib.OUT_RGBA32F or E.math != _lib.MATH_STRICT:
        raise ValueError("render_brats_autograd: unshaded whole frames in STRICT math and fp32 only")
    for g in (labels, preds):
        if isinstance(g, Grid) and g.layout != "linear":
            raise ValueError("render_brats_autograd: LINEAR label grids only")
    lab = _as_device_tensor(labels, torch.int32, dev, "gLabels")
    prd = _as_device_tensor(preds, torch.int32, dev, "gPreds")
    return _RenderBrats.apply(p, dict(ext or {}), lab, prd, tf, *vols)
