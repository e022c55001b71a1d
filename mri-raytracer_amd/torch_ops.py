"""``torch.ops.mrirt.*`` — the C ABI of libmrirt.so registered as PyTorch custom operators.

Device tensors in, a device tensor out, launched on the current HIP stream, no implicit
synchronisation.  The operators are thin: parameter blocks travel as
CPU ``uint8`` tensors holding the C structs of include/mrirt.h byte for byte (``pack_brats_params``
& co. build them from the reference's ``gParams`` dicts), every size check the C side cannot make
(it only sees pointers) is made here, and the launch itself is the same ``mrirt_*`` entry point the
rest of the package calls.  There is no CPU implementation: the only other registration is the
shape function ("fake" kernel) that ``torch.compile`` / meta tensors need.  Every operator's outputs are allocated by one
``_*_outs`` function, which the real kernel calls on the operands' GPU and which is also its fake kernel.  All 19
operators also exist as a C++ extension (``load_native()`` -> ``torch.ops.mrirt_native.*``, csrc/torch_binding.cpp);
tests/test_torch_ops_contract.py holds the two lists to each other and is where a new operator is added first.

    blob = mrirt.torch_ops.pack_brats_params(gparams)
    ext  = mrirt.torch_ops.pack_render_ext({"layout": "vg", **mrirt.synth.SHADE_EXT})
    img  = torch.ops.mrirt.render_brats(blob, ext, grid.data, None, None, None, None, None)
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Any, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .params import brats_params, mesh_params, render_ext, sdf_params, volume_params
from .tiles import local_tile_count


def load_native():
    """``torch.ops.mrirt_native`` — the same 19 operators registered from C++ (csrc/torch_binding.cpp, a
    PyTorch-ROCm C++ extension linked to libmrirt.so; schemas as ``torch.ops.mrirt.*`` below).  Raises if
    libmrirt_torch.so has not been built (``__graft_entry__.build()``): like the HIP library, it has no fallback."""
    if not _lib.TORCH_SO_PATH.exists():
        raise ImportError(f"{_lib.TORCH_SO_PATH} is missing — build it with `python -c \"import __graft_entry__ as g; g.build()\"`.")
    _lib.lib()                                    # libmrirt.so first: the operator library links against it
    torch.ops.load_library(str(_lib.TORCH_SO_PATH))
    return torch.ops.mrirt_native


# --- parameter blocks <-> uint8 tensors ---------------------------------------------------------
def _blob(struct: C.Structure) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(bytes(struct), dtype=np.uint8).copy())


def _unblob(t: torch.Tensor, ctype):
    if t.device.type != "cpu" or t.dtype != torch.uint8 or t.numel() != C.sizeof(ctype):
        raise TypeError(f"expected a CPU uint8 tensor of {C.sizeof(ctype)} bytes ({ctype.__name__})")
    return ctype.from_buffer_copy(t.contiguous().numpy().tobytes())


def pack_brats_params(p: Mapping[str, Any]) -> torch.Tensor:
    """gParams dict of inr/viewer/brats_viewer.py:405-426 -> MrirtBratsParams bytes."""
    return _blob(brats_params(p))


def pack_render_ext(ext: Optional[Mapping[str, Any]] = None) -> torch.Tensor:
    return _blob(render_ext(ext))


def pack_volume_params(p: Mapping[str, Any]) -> torch.Tensor:
    """gParams dict of scripts/volumeRendering/app.py:331-345 -> MrirtVolumeParams bytes."""
    return _blob(volume_params(p))


def pack_sdf_params(p: Mapping[str, Any], eye, U, V, W) -> torch.Tensor:
    """gParams + gEye/gU/gV/gW of scripts/raymarch/app.py:199-221 -> MrirtSdfParams bytes."""
    return _blob(sdf_params(p, eye, U, V, W))


def pack_mesh_params(p: Mapping[str, Any]) -> torch.Tensor:
    """gParams dict of scripts/mesh_rt/app.py:224-232 -> MrirtMeshParams bytes."""
    return _blob(mesh_params(p))


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _one_device(named: Sequence) -> torch.device:
    """The GPU every device tensor of a call lives on (raises when they disagree).  The launch then happens with that
    GPU current (``torch.cuda.device``): the stream is ITS current stream and the output is allocated on it — with
    device 0 current and the grids on device 1 the kernel would otherwise be enqueued on device 0 with device-1
    pointers."""
    dev = None
    for what, t in named:
        if t is None:
            continue
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{what} is on {t.device} but another operand is on {dev}: every device tensor of one call "
                             "must live on the same GPU")
    if dev is None:
        raise ValueError("no device tensor bound")
    return dev


def _dev_flat(t: Optional[torch.Tensor], dtype, what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise TypeError(f"{what}: expected a contiguous device {dtype} tensor")
    return t


def _present(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None or t.numel() == 0 else t


# An operator's outputs are allocated by its ``_*_outs`` function, on the device it is given: the real kernel calls it with the
# operands' GPU current, and _shapes makes the same function the operator's fake kernel — so the two cannot disagree.
def _shapes(op, outs, like: Sequence[str], blocks: Mapping[str, Any] = {}):
    """Register the fake kernel of ``op``: ``outs`` is called with the operator's arguments by name (it names the ones it needs
    and swallows the rest; the parameter blobs named in ``blocks`` arrive as their C structs) and with ``dev``, the device of the
    first bound argument of ``like``."""
    names = [a.name for a in op._opoverload._schema.arguments]

    def fake(*args):
        kw = dict(zip(names, args))
        dev = next(kw[k] for k in like if kw[k] is not None).device
        kw.update({k: _unblob(kw[k], ctype) for k, ctype in blocks.items()})
        out = outs(dev=dev, **kw)
        return out if isinstance(out, torch.Tensor) else tuple(out)
    op.register_fake(fake)
    return fake


def _frame_outs(params, ext: _lib.RenderExt, dev, **_):
    """The frame of K1 / K2 / K4 (``params``: any parameter block with an imageSize): [H, W, 4], or this rank's tiles."""
    E, width, height = ext, int(params.imageSize[0]), int(params.imageSize[1])
    dt = torch.float16 if E.outFormat == _lib.OUT_RGBA16F else torch.float32
    if E.tileSize > 0:
        tiles = local_tile_count(width, height, E.tileSize, E.tileRank, E.tileWorld)
        return torch.empty((tiles, int(E.tileSize), int(E.tileSize), 4), dtype=dt, device=dev)
    return torch.empty((height, width, 4), dtype=dt, device=dev)


def _grid_need(dims: Sequence[int], layout: int) -> int:
    l = _lib.lib()
    d = (C.c_uint32 * 3)(*dims)
    if layout == _lib.LAYOUT_LINEAR:
        return dims[0] * dims[1] * dims[2]
    if layout == _lib.LAYOUT_BRICK:
        return int(l.mrirt_brick_elems(d))
    if layout == _lib.LAYOUT_VGA:                    # three axis-flat copies of the float4 voxels
        return 4 * int(l.mrirt_vga_elems(d))
    if layout == _lib.LAYOUT_LABCELL:                # both overlays' corner labels per cell: 8 bytes per element
        return 2 * int(l.mrirt_vec4_elems(d))
    return 4 * int(l.mrirt_vec4_elems(d))


def _linear_need(dims: Sequence[int], layout: int) -> int:
    return dims[0] * dims[1] * dims[2]               # the differentiable operators take LINEAR grids whatever ext says


# --- K1 -----------------------------------------------------------------------------------------
def _bind_k1(params, ext, vols, labels, preds, *, need, pred_overlay: bool, empty_is_absent: bool, one_grid_layout=None,
             cell_label_layout=None, grad_out: Optional[torch.Tensor] = None, extra: Sequence = ()):
    """The operand binding every K1 operator shares: the two parameter blocks, the four intensity grids, gLabels and gPreds
    checked for device, dtype, contiguity and size, all on one GPU.  ``need(dims, layout)`` is the element count a grid of that
    layout holds; ``pred_overlay`` says whether the operator draws the hard prediction overlay (showPred) at all;
    ``empty_is_absent`` lets an empty tensor stand for an absent grid.  With ``ext.layout == one_grid_layout`` gIntensity0 alone
    carries every modality, with ``ext.labelLayout == cell_label_layout`` gLabels carries the predictions too.  ``grad_out``:
    the fp32 [H, W, 4] frame gradient of a backward operator; ``extra``: further (name, device tensor) operands of the call
    for the one-device check.  Returns (P, E, the array of four grid pointers, (vols, labels, preds) as bound, the device)."""
    P, E = _unblob(params, _lib.BratsParams), _unblob(ext, _lib.RenderExt)
    g = _dev_flat(grad_out, torch.float32, "grad_out")
    if g is not None and tuple(g.shape) != (int(P.imageSize[1]), int(P.imageSize[0]), 4):
        raise ValueError(f"grad_out: expected ({int(P.imageSize[1])}, {int(P.imageSize[0])}, 4), got {tuple(g.shape)}")
    dims = [int(v) for v in P.dims]
    keep = _present if empty_is_absent else (lambda t: t)
    vols = [_dev_flat(keep(v), torch.float32, f"gIntensity{m}") for m, v in enumerate(vols)]
    lab = _dev_flat(keep(labels), torch.int32, "gLabels")
    prd = _dev_flat(keep(preds), torch.int32, "gPreds")
    vneed, lneed = need(dims, E.layout), need(dims, E.labelLayout)
    one_grid = E.layout == one_grid_layout
    for m, v in enumerate(vols):
        if (m == 0 if one_grid else P.volEnabled[m] != 0) and (v is None or v.numel() < vneed):
            raise ValueError(f"gIntensity{m} is {'the one grid of all modalities' if one_grid else 'enabled'} but holds "
                             f"{0 if v is None else v.numel()} < {vneed} elements")
    if P.showSeg != 0 and (lab is None or lab.numel() < lneed):
        raise ValueError("showSeg is set but gLabels is missing or too small")
    src = lab if E.labelLayout == cell_label_layout else prd
    if pred_overlay and P.showPred != 0 and (src is None or src.numel() < lneed):
        raise ValueError("showPred is set but gPreds (or the label-cell grid) is missing or too small")
    dev = _one_device([("grad_out", g), *extra] + [(f"gIntensity{m}", v) for m, v in enumerate(vols)] + [("gLabels", lab), ("gPreds", prd)])
    vp = (C.c_void_p * 4)(*[C.c_void_p(v.data_ptr()) if v is not None else None for v in vols])
    return P, E, vp, (vols, lab, prd), dev


@torch.library.custom_op("mrirt::render_brats", mutates_args=())
def render_brats(params: torch.Tensor, ext: torch.Tensor, vol0: Optional[torch.Tensor], vol1: Optional[torch.Tensor],
                 vol2: Optional[torch.Tensor], vol3: Optional[torch.Tensor], labels: Optional[torch.Tensor],
                 preds: Optional[torch.Tensor]) -> torch.Tensor:
    """brats_main (inr/viewer/brats_rt.slang:85-168) through mrirt_render_brats_ex.  With a MOD4 ext.layout vol0 is the float4
    grid of all four modalities (vol1..3 are ignored); with a LABCELL ext.labelLayout gLabels carries both overlays' grids
    (gPreds is ignored)."""
    P, E, vp, (_, lab, prd), dev = _bind_k1(params, ext, (vol0, vol1, vol2, vol3), labels, preds, need=_grid_need, pred_overlay=True,
                                            empty_is_absent=False, one_grid_layout=_lib.LAYOUT_MOD4,
                                            cell_label_layout=_lib.LAYOUT_LABCELL)
    with torch.cuda.device(dev):
        out = _frame_outs(P, E, dev)
        rc = _lib.lib().mrirt_render_brats_ex(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(prd), _ptr(out),
                                              int(P.imageSize[0]), None, _stream())
    _lib.check(rc, "mrirt_render_brats_ex")
    return out


# --- K1 backward --------------------------------------------------------------------------------
def _brats_backward_outs(params, vol0, vol1, vol2, vol3, dev, **_):
    """dL/dvol0..3 (empty for a modality that is disabled or not bound) and dL/d(ww, wl, intensityAlpha, gamma), zeroed."""
    nvox = int(params.dims[0]) * int(params.dims[1]) * int(params.dims[2])
    gv = [torch.zeros(nvox if (params.volEnabled[m] != 0 and _present(v) is not None) else 0, dtype=torch.float32, device=dev)
          for m, v in enumerate((vol0, vol1, vol2, vol3))]
    return gv + [torch.zeros(4, dtype=torch.float64, device=dev)]


@torch.library.custom_op("mrirt::render_brats_backward", mutates_args=())
def render_brats_backward(params: torch.Tensor, ext: torch.Tensor, grad_out: torch.Tensor, vol0: Optional[torch.Tensor],
                          vol1: Optional[torch.Tensor], vol2: Optional[torch.Tensor], vol3: Optional[torch.Tensor],
                          labels: Optional[torch.Tensor], preds: Optional[torch.Tensor]
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Gradients of one K1 frame on LINEAR fp32 grids through mrirt_render_brats_backward: ``grad_out`` is dL/dframe, fp32
    [H, W, 4] (alpha ignored).  Returns dL/dvol0..3 (fp32 [X*Y*Z]; an empty tensor for a modality that is disabled or not
    bound — an empty tensor also stands for an absent modality on the way in) and dL/d(ww, wl, intensityAlpha, gamma) as
    float64 [4].  Freshly zeroed outputs: summing over views is the caller's ``+=``."""
    P, E, vp, (vols, lab, prd), dev = _bind_k1(params, ext, (vol0, vol1, vol2, vol3), labels, preds, need=_linear_need, pred_overlay=True,
                                               empty_is_absent=True, grad_out=grad_out)
    with torch.cuda.device(dev):
        *gv, gtf = _brats_backward_outs(P, *vols, dev)
        gp = (C.c_void_p * 4)(*[C.c_void_p(t.data_ptr()) if t.numel() else None for t in gv])
        rc = _lib.lib().mrirt_render_brats_backward(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(prd), _ptr(grad_out),
                                                    int(P.imageSize[0]), gp, _ptr(gtf), _stream())
    _lib.check(rc, "mrirt_render_brats_backward")
    return gv[0], gv[1], gv[2], gv[3], gtf


# --- K1 soft prediction overlay -------------------------------------------------------------------
def _bind_soft(params, ext, logits, offsets, vols, labels, grad_out=None):
    """The checks the two soft-overlay operators add to _bind_k1 (LINEAR grids, no hard prediction overlay, an empty tensor stands
    for an absent grid); returns (P, E, vol pointers, labels, device)."""
    z = _dev_flat(logits, torch.float32, "logits")
    off = _dev_flat(offsets, torch.int64, "offsets")
    if z.dim() != 2 or not 1 <= int(z.shape[1]) <= 16:
        raise ValueError(f"logits: expected (rows, 1..16 classes), got {tuple(z.shape)}")
    P, E, vp, (_, lab, _), dev = _bind_k1(params, ext, vols, labels, None, need=_linear_need, pred_overlay=False, empty_is_absent=True,
                                          grad_out=grad_out, extra=[("logits", z), ("offsets", off)])
    if off.numel() != int(P.imageSize[0]) * int(P.imageSize[1]):
        raise ValueError(f"offsets: expected {int(P.imageSize[0]) * int(P.imageSize[1])} elements (one per pixel), got {off.numel()}")
    return P, E, vp, lab, dev


def _soft_outs(params, dev, **_):
    return torch.empty((int(params.imageSize[1]), int(params.imageSize[0]), 4), dtype=torch.float32, device=dev)


def _soft_backward_outs(logits: torch.Tensor, **_):
    return torch.zeros_like(logits)


@torch.library.custom_op("mrirt::render_brats_soft", mutates_args=())
def render_brats_soft(params: torch.Tensor, ext: torch.Tensor, logits: torch.Tensor, offsets: torch.Tensor,
                      vol0: Optional[torch.Tensor], vol1: Optional[torch.Tensor], vol2: Optional[torch.Tensor],
                      vol3: Optional[torch.Tensor], labels: Optional[torch.Tensor]) -> torch.Tensor:
    """The soft-overlay K1 frame through mrirt_render_brats_soft: ``logits`` fp32 [rows, C], ``offsets`` int64 [H * W] (row of
    the first sample of every pixel); LINEAR fp32 grids.  Returns fp32 [H, W, 4]."""
    P, E, vp, lab, dev = _bind_soft(params, ext, logits, offsets, (vol0, vol1, vol2, vol3), labels)
    with torch.cuda.device(dev):
        out = _soft_outs(P, dev)
        rc = _lib.lib().mrirt_render_brats_soft(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(logits), int(logits.shape[1]), _ptr(offsets),
                                                _ptr(out), int(P.imageSize[0]), None, _stream())
    _lib.check(rc, "mrirt_render_brats_soft")
    return out


@torch.library.custom_op("mrirt::render_brats_soft_backward", mutates_args=())
def render_brats_soft_backward(params: torch.Tensor, ext: torch.Tensor, grad_out: torch.Tensor, logits: torch.Tensor,
                               offsets: torch.Tensor, vol0: Optional[torch.Tensor], vol1: Optional[torch.Tensor],
                               vol2: Optional[torch.Tensor], vol3: Optional[torch.Tensor], labels: Optional[torch.Tensor]
                               ) -> torch.Tensor:
    """dL/dlogits of the soft-overlay frame through mrirt_render_brats_soft_backward: ``grad_out`` is dL/dframe, fp32
    [H, W, 4] (alpha ignored).  Returns fp32 shaped like ``logits``, allocated zeroed (rows no ray owns stay zero)."""
    P, E, vp, lab, dev = _bind_soft(params, ext, logits, offsets, (vol0, vol1, vol2, vol3), labels, grad_out=grad_out)
    with torch.cuda.device(dev):
        dl = _soft_backward_outs(logits)
        rc = _lib.lib().mrirt_render_brats_soft_backward(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(logits), int(logits.shape[1]),
                                                         _ptr(offsets), _ptr(grad_out), int(P.imageSize[0]), _ptr(dl), _stream())
    _lib.check(rc, "mrirt_render_brats_soft_backward")
    return dl


# --- K2 -----------------------------------------------------------------------------------------
_VOX_DTYPE = {_lib.VOX_U32X4: torch.int32, _lib.VOX_U8: torch.uint8, _lib.VOX_F32: torch.float32}


@torch.library.custom_op("mrirt::render_volume", mutates_args=())
def render_volume(params: torch.Tensor, ext: torch.Tensor, volume: torch.Tensor, mode: int) -> torch.Tensor:
    """volume_cs (scripts/volumeRendering/volume_render.slang:104-148) through mrirt_render_volume;
    ``mode``: 0 one-u32-per-voxel (the reference's upload), 1 bytes, 2 fp32."""
    P, E = _unblob(params, _lib.VolumeParams), _unblob(ext, _lib.RenderExt)
    if mode not in _VOX_DTYPE:
        raise ValueError("mode must be 0 (u32x4), 1 (u8) or 2 (f32)")
    vol = _dev_flat(volume, _VOX_DTYPE[mode], "gVolumeU8")
    nvox = int(P.volDim[0]) * int(P.volDim[1]) * int(P.volDim[2])
    if vol.numel() < nvox:
        raise ValueError(f"gVolumeU8 holds {vol.numel()} < {nvox} voxels")
    with torch.cuda.device(vol.device):
        out = _frame_outs(P, E, vol.device)
        rc = _lib.lib().mrirt_render_volume(C.byref(P), C.byref(E), _ptr(vol), int(mode), _ptr(out), int(P.imageSize[0]),
                                            None, _stream())
    _lib.check(rc, "mrirt_render_volume")
    return out


# --- K3 -----------------------------------------------------------------------------------------
def _sdf_outs(width: int, height: int, dev, **_):
    return torch.empty((height, width, 4), dtype=torch.float32, device=dev)


@torch.library.custom_op("mrirt::render_sdf", mutates_args=())
def render_sdf(params: torch.Tensor, width: int, height: int, like: torch.Tensor) -> torch.Tensor:
    """raymarch_cs (scripts/raymarch/raymarch.slang:60-99); ``like`` only names the device."""
    P = _unblob(params, _lib.SdfParams)
    if not like.is_cuda:
        raise TypeError("like: expected a device tensor")
    with torch.cuda.device(like.device):
        out = _sdf_outs(width, height, like.device)
        rc = _lib.lib().mrirt_render_sdf(C.byref(P), int(width), int(height), _ptr(out), int(width), _stream())
    _lib.check(rc, "mrirt_render_sdf")
    return out


# --- K4 -----------------------------------------------------------------------------------------
@torch.library.custom_op("mrirt::render_mesh", mutates_args=())
def render_mesh(params: torch.Tensor, ext: torch.Tensor, nodes: torch.Tensor, tris: torch.Tensor, verts: torch.Tensor,
                max_depth: int) -> torch.Tensor:
    """compute_main (scripts/mesh_rt/mesh_rt.slang:138-164) through mrirt_render_mesh.  nodes: float32 [2N x 4], tris: int32
    [M x 4], verts: float32 [V x 4] (mrirt.upload_mesh's buffers; the counts are taken from their sizes); max_depth: the
    tree's depth (``Mesh.depth``).  The kernel stops, and paints, any ray that meets a malformed buffer; it never reads
    outside these three tensors.  (The library refuses a tiled ext for K4.)"""
    P, E = _unblob(params, _lib.MeshParams), _unblob(ext, _lib.RenderExt)
    n = _dev_flat(nodes, torch.float32, "gBVHNodes")
    t = _dev_flat(tris, torch.int32, "gTris")
    v = _dev_flat(verts, torch.float32, "gVerts")
    dev = _one_device([("gBVHNodes", n), ("gTris", t), ("gVerts", v)])
    with torch.cuda.device(dev):
        out = _frame_outs(P, E, dev)
        rc = _lib.lib().mrirt_render_mesh(C.byref(P), C.byref(E), _ptr(n), n.numel() // 8, _ptr(t), t.numel() // 4, _ptr(v),
                                          v.numel() // 4, int(max_depth), _ptr(out), int(P.imageSize[0]), None, None, _stream())
    _lib.check(rc, "mrirt_render_mesh")
    return out


# --- INR ----------------------------------------------------------------------------------------
def _inr_desc(kind: int, num_layers: int, in_dim: int, out_dim: int, hidden: int, fourier_freqs: int, num_mods: int,
              w0: float = 0.0) -> _lib.InrDesc:
    d = _lib.InrDesc()
    d.kind, d.numLayers, d.inDim, d.outDim, d.hidden = kind, num_layers, in_dim, out_dim, hidden
    d.fourierFreqs, d.numMods, d.w0 = fourier_freqs, num_mods, w0
    return d


def _inr_inputs(kind: int, in_dim: int, num_mods: int, coords, feats, n: int):
    """coords [n, 3] (the coordinate kinds 0 / 1) and feats [n, num_mods] — or, for the raw kinds 2 / 3, the [n, in_dim] input matrix."""
    co = _dev_flat(coords, torch.float32, "coords")
    fe = _dev_flat(feats, torch.float32, "feats")
    if kind < 2 and (co is None or co.numel() < 3 * n):
        raise ValueError("coords must hold [n, 3] floats")
    width = in_dim if kind >= 2 else num_mods
    if width > 0 and (fe is None or fe.numel() < width * n):
        raise ValueError(f"feats must hold [n, {width}] floats")
    return co, fe


def _logits_outs(n: int, out_dim: int, dev, **_):
    return torch.empty((n, out_dim), dtype=torch.float32, device=dev)


@torch.library.custom_op("mrirt::inr_forward", mutates_args=())
def inr_forward(weights: torch.Tensor, biases: torch.Tensor, kind: int, num_layers: int, in_dim: int, out_dim: int,
                hidden: int, fourier_freqs: int, num_mods: int, w0: float, coords: Optional[torch.Tensor],
                feats: Optional[torch.Tensor], n: int) -> torch.Tensor:
    """Logits [n, out_dim] of the packed MLP (``mrirt.inr.pack_mlp(...).weights / .biases``) for n points:
    inr/inr/model.py:21-50 (kind 0), notebooks/neumors_inr.ipynb:1165-1178 (kind 1), or the raw-input
    forms (kinds 2/3: ``feats`` is the [n, in_dim] input matrix)."""
    d = _inr_desc(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, w0)
    need = int(_lib.lib().mrirt_inr_pack_bytes(C.byref(d)))
    if need <= 0:
        raise ValueError("unsupported network shape")
    if not weights.is_cuda or weights.dtype != torch.uint8 or weights.numel() < need:
        raise TypeError(f"weights: expected the {need}-byte packed image of mrirt_inr_pack_weights on the device")
    nb = (num_layers - 1) * hidden + ((out_dim + 31) // 32) * 32
    bz = _dev_flat(biases, torch.float32, "biases")
    if bz.numel() < nb:
        raise ValueError(f"biases holds {bz.numel()} < {nb} floats (each layer padded to a multiple of 32)")
    co, fe = _inr_inputs(kind, in_dim, num_mods, coords, feats, n)
    d.weights, d.biases = weights.data_ptr(), bz.data_ptr()
    dev = _one_device([("weights", weights), ("biases", bz), ("coords", co), ("feats", fe)])
    with torch.cuda.device(dev):
        out = _logits_outs(n, out_dim, dev)
        rc = _lib.lib().mrirt_inr_forward(C.byref(d), _ptr(co), _ptr(fe), int(n), _ptr(out), None, _stream())
    _lib.check(rc, "mrirt_inr_forward")
    return out


# --- exact distance transform / Hausdorff -------------------------------------------------------
def _edt_args(labels: Sequence, spacing: Sequence[float]):
    vols = [_dev_flat(v, torch.int16, what) for what, v in labels]
    if any(v.dim() != 3 or v.shape != vols[0].shape for v in vols):
        raise ValueError("label volumes must be (H, W, D) int16 tensors of one shape")
    if len(spacing) != 3:
        raise ValueError("spacing: expected three values")
    return vols, (C.c_uint32 * 3)(*vols[0].shape), (C.c_float * 3)(*[float(np.float32(s)) for s in spacing])


def _edt_outs(labels: torch.Tensor, dev, **_):
    return torch.empty(tuple(labels.shape), dtype=torch.float64, device=dev)


def _hausdorff_outs(num_classes: int, dev, **_):
    return torch.empty((max(num_classes, 0), 2), dtype=torch.float64, device=dev)


@torch.library.custom_op("mrirt::edt_squared", mutates_args=())
def edt_squared(labels: torch.Tensor, cls: int, spacing: Sequence[float]) -> torch.Tensor:
    """fp64 (H, W, D): squared distance of every voxel to the nearest voxel with ``labels == cls`` (+inf when there is
    none), coordinates ``float32(index) * float32(spacing)`` — mrirt_edt_squared, exact."""
    (lab,), hwd, sp = _edt_args([("labels", labels)], spacing)
    lib = _lib.lib()
    with torch.cuda.device(lab.device):
        nbytes = int(lib.mrirt_edt_scratch_bytes(hwd, 0))
        out = _edt_outs(lab, lab.device)
        scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=lab.device)
        rc = lib.mrirt_edt_squared(_ptr(lab), hwd, int(cls), sp, _ptr(out), _ptr(scratch), nbytes, _stream())
    _lib.check(rc, "mrirt_edt_squared")
    return out


@torch.library.custom_op("mrirt::hausdorff", mutates_args=())
def hausdorff(pred: torch.Tensor, truth: torch.Tensor, spacing: Sequence[float], num_classes: int) -> torch.Tensor:
    """fp64 (num_classes, 2) squared directed Hausdorff distances of two int16 (H, W, D) label volumes (mrirt_hausdorff):
    [c, 0] = max over (pred == c) of the squared distance to (truth == c), [c, 1] the other direction, NaN where the class
    is absent from either; inr/inr/model.py:164-195's value for class c is ``sqrt(max of the row)``."""
    (p, t), hwd, sp = _edt_args([("pred", pred), ("truth", truth)], spacing)
    dev = _one_device([("pred", p), ("truth", t)])
    lib = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = int(lib.mrirt_edt_scratch_bytes(hwd, int(num_classes)))
        out = _hausdorff_outs(int(num_classes), dev)
        scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=dev)
        rc = lib.mrirt_hausdorff(_ptr(p), _ptr(t), hwd, sp, int(num_classes), _ptr(out), _ptr(scratch), nbytes, _stream())
    _lib.check(rc, "mrirt_hausdorff")
    return out


# --- class surfaces of label volumes (naive surface nets) ---------------------------------------
def _surface_args(labels: torch.Tensor, class_mask: int):
    lab = _dev_flat(labels, torch.int16, "labels")
    if lab.dim() != 3:
        raise ValueError("labels must be an (H, W, D) int16 tensor")
    if not 0 <= int(class_mask) <= 0xFFFFFFFF:
        raise ValueError("class_mask: expected a uint32 bit set (bit l = label l is inside)")
    hwd = (C.c_uint32 * 3)(*lab.shape)
    nbytes = int(_lib.lib().mrirt_surface_scratch_bytes(hwd))
    if nbytes <= 0:
        raise ValueError(f"a volume of shape {tuple(lab.shape)} is outside the supported sizes")
    return lab, hwd, nbytes


def _surface_count_outs(dev, **_):
    return torch.empty(2, dtype=torch.int64, device=dev)


def _surface_extract_outs(num_verts: int, num_tris: int, dev, **_):
    return torch.zeros((num_verts, 3), dtype=torch.float32, device=dev), torch.zeros((num_tris, 3), dtype=torch.int32, device=dev)


@torch.library.custom_op("mrirt::surface_count", mutates_args=())
def surface_count(labels: torch.Tensor, class_mask: int) -> torch.Tensor:
    """int64 [2] on the device: vertices and triangles of the surface of the voxels whose label's bit is set in
    ``class_mask`` (mrirt_surface_count).  No host synchronisation."""
    lab, hwd, nbytes = _surface_args(labels, class_mask)
    with torch.cuda.device(lab.device):
        counts = _surface_count_outs(lab.device)
        scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=lab.device)
        rc = _lib.lib().mrirt_surface_count(_ptr(lab), hwd, int(class_mask), _ptr(scratch), nbytes, _ptr(counts), _stream())
    _lib.check(rc, "mrirt_surface_count")
    return counts


@torch.library.custom_op("mrirt::surface_extract", mutates_args=())
def surface_extract(labels: torch.Tensor, class_mask: int, spacing: Sequence[float], origin: Sequence[float], num_verts: int,
                    num_tris: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(verts float32 [num_verts, 3], tris int32 [num_tris, 3]) of mrirt_surface_extract; the two sizes are the static
    shapes of the outputs — the values of ``surface_count``.  With sizes smaller than the surface nothing is written (the
    tensors come back zeroed); larger ones leave the rows past the surface zero.  No host synchronisation."""
    lab, hwd, nbytes = _surface_args(labels, class_mask)
    if len(spacing) != 3 or len(origin) != 3:
        raise ValueError("spacing / origin: expected three values each")
    if num_verts < 0 or num_tris < 0:
        raise ValueError("num_verts / num_tris must not be negative")
    sp = (C.c_float * 3)(*[float(np.float32(v)) for v in spacing])
    org = (C.c_float * 3)(*[float(np.float32(v)) for v in origin])
    with torch.cuda.device(lab.device):
        verts, tris = _surface_extract_outs(int(num_verts), int(num_tris), lab.device)
        counts = torch.empty(2, dtype=torch.int64, device=lab.device)
        scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=lab.device)
        rc = _lib.lib().mrirt_surface_extract(_ptr(lab), hwd, int(class_mask), sp, org, _ptr(verts) if num_verts else None,
                                              int(num_verts), _ptr(tris) if num_tris else None, int(num_tris), _ptr(scratch),
                                              nbytes, _ptr(counts), _stream())
    _lib.check(rc, "mrirt_surface_extract")
    return verts, tris


# --- INR training step (fp32; csrc/inr_train.hip) -----------------------------------------------
def _train_desc(kind: int, num_layers: int, in_dim: int, out_dim: int, hidden: int, fourier_freqs: int, num_mods: int, n: int):
    d = _inr_desc(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods)
    nbytes = int(_lib.lib().mrirt_inr_train_scratch_bytes(C.byref(d), int(n)))
    if nbytes <= 0:
        raise ValueError("unsupported network kind / shape / n for the training step (ReLU kinds only)")
    nw = in_dim * hidden + (num_layers - 2) * hidden * hidden + hidden * out_dim
    nb = (num_layers - 1) * hidden + out_dim
    return d, nbytes, nw, nb


def _forward_f32_outs(n: int, out_dim: int, nbytes: int, dev):
    return _logits_outs(n, out_dim, dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _backward_outs(nw: int, nb: int, dev):
    return torch.empty(nw, dtype=torch.float32, device=dev), torch.empty(nb, dtype=torch.float32, device=dev)


@torch.library.custom_op("mrirt::inr_forward_f32", mutates_args=())
def inr_forward_f32(weights: torch.Tensor, biases: torch.Tensor, kind: int, num_layers: int, in_dim: int, out_dim: int,
                    hidden: int, fourier_freqs: int, num_mods: int, coords: Optional[torch.Tensor], feats: Optional[torch.Tensor],
                    n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(logits fp32 [n, out_dim], scratch uint8) of mrirt_inr_forward_f32: ``weights`` fp32 row-major [in, out] per layer,
    concatenated unpadded, ``biases`` concatenated unpadded; kind 0 (coords [n, 3] + feats [n, num_mods]) or 2 (feats is the
    [n, in_dim] input matrix).  ``scratch`` holds the activations ``inr_backward`` reads."""
    d, nbytes, nw, nb = _train_desc(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, n)
    w = _dev_flat(weights, torch.float32, "weights")
    b = _dev_flat(biases, torch.float32, "biases")
    if w.numel() < nw or b.numel() < nb:
        raise ValueError(f"weights / biases hold {w.numel()} / {b.numel()} floats, the network has {nw} / {nb}")
    co, fe = _inr_inputs(kind, in_dim, num_mods, coords, feats, n)
    dev = _one_device([("weights", w), ("biases", b), ("coords", co), ("feats", fe)])
    with torch.cuda.device(dev):
        out, scratch = _forward_f32_outs(n, out_dim, nbytes, dev)
        rc = _lib.lib().mrirt_inr_forward_f32(C.byref(d), _ptr(w), _ptr(b), _ptr(co), _ptr(fe), int(n), _ptr(out), _ptr(scratch),
                                              nbytes, _stream())
    _lib.check(rc, "mrirt_inr_forward_f32")
    return out, scratch


@inr_forward_f32.register_fake
def _(weights, biases, kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, coords, feats, n):
    nbytes = _train_desc(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, n)[1]
    return _forward_f32_outs(n, out_dim, nbytes, weights.device)


def _loss_operands(logits: torch.Tensor, labels: torch.Tensor, class_weights: Sequence[float], focal_alpha: Sequence[float] = ()):
    """The operand checks of both losses: logits [n, C] and int32 labels [n] on one GPU, 1..16 classes, one class weight each
    (and a focal_alpha that is empty or one value per class); returns (n, C, the device)."""
    z = _dev_flat(logits, torch.float32, "logits")
    lab = _dev_flat(labels, torch.int32, "labels")
    if z.dim() != 2 or z.shape[0] < 1 or lab.numel() != z.shape[0]:
        raise ValueError("logits must be [n, C] with n >= 1 and labels [n]")
    n, nc = int(z.shape[0]), int(z.shape[1])
    if not 1 <= nc <= 16 or len(class_weights) != nc or len(focal_alpha) not in (0, nc):
        raise ValueError("1..16 classes, one class weight each, focal_alpha empty or one value per class")
    return n, nc, _one_device([("logits", z), ("labels", lab)])


def _loss_outs(logits: torch.Tensor, terms: bool, dev, **_):
    """loss [1], aux [2, C], (the extended loss: terms [5],) dlogits like logits."""
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    aux = torch.empty((2, logits.shape[1]), dtype=torch.float32, device=dev)
    if terms:
        return loss, aux, torch.empty(5, dtype=torch.float32, device=dev), torch.empty_like(logits)
    return loss, aux, torch.empty_like(logits)


@torch.library.custom_op("mrirt::inr_loss", mutates_args=())
def inr_loss(logits: torch.Tensor, labels: torch.Tensor, class_weights: Sequence[float],
             dice_weight: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss fp32 [1], aux fp32 [2, C]: CE per class and Dice per class, dlogits fp32 [n, C]) of mrirt_inr_loss
    (inr/inr/model.py:64-88) on logits [n, C] and int32 labels [n]."""
    n, nc, dev = _loss_operands(logits, labels, class_weights)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = int(lib.mrirt_inr_loss_scratch_bytes(n))
        loss, aux, dl = _loss_outs(logits, False, dev)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rc = lib.mrirt_inr_loss(_ptr(logits), _ptr(labels), n, nc, (C.c_float * nc)(*[float(np.float32(v)) for v in class_weights]),
                                float(dice_weight), _ptr(loss), _ptr(aux), _ptr(dl), _ptr(scratch), nbytes, _stream())
    _lib.check(rc, "mrirt_inr_loss")
    return loss, aux, dl


@torch.library.custom_op("mrirt::inr_loss_ext", mutates_args=())
def inr_loss_ext(logits: torch.Tensor, labels: torch.Tensor, class_weights: Sequence[float], focal_alpha: Sequence[float], dice_weight: float,
                 per_class_dice: bool, focal_gamma: float, label_smoothing: float, edema_fp_weight: float, tversky_alpha: float,
                 tversky_beta: float, tversky_weight: float, edema_logit_reg: float,
                 edema_class: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss fp32 [1], aux fp32 [2, C], terms fp32 [5]: CE, Dice loss, edema FP / n, Tversky index, logit-regulariser mean,
    dlogits fp32 [n, C]) of mrirt_inr_loss_ext (scripts/jax_inr_brats.py:205-257) on logits [n, C] and int32 labels [n].
    An empty ``focal_alpha`` leaves the focal factor unweighted."""
    n, nc, dev = _loss_operands(logits, labels, class_weights, focal_alpha)
    x = _lib.InrLossExt()
    for k in range(nc):
        x.classWeights[k] = float(class_weights[k])
        if len(focal_alpha):
            x.focalAlpha[k] = float(focal_alpha[k])
    x.diceWeight, x.focalGamma, x.labelSmoothing = float(dice_weight), float(focal_gamma), float(label_smoothing)
    x.edemaFpWeight, x.tverskyAlpha, x.tverskyBeta = float(edema_fp_weight), float(tversky_alpha), float(tversky_beta)
    x.tverskyWeight, x.edemaLogitReg, x.edemaClass = float(tversky_weight), float(edema_logit_reg), int(edema_class)
    x.flags = (_lib.LOSS_PER_CLASS_DICE if per_class_dice else 0) | (_lib.LOSS_FOCAL_ALPHA if len(focal_alpha) else 0)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = int(lib.mrirt_inr_loss_ext_scratch_bytes(n))
        loss, aux, terms, dl = _loss_outs(logits, True, dev)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rc = lib.mrirt_inr_loss_ext(_ptr(logits), _ptr(labels), n, nc, C.byref(x), _ptr(loss), _ptr(aux), _ptr(terms), _ptr(dl), _ptr(scratch),
                                    nbytes, _stream())
    _lib.check(rc, "mrirt_inr_loss_ext")
    return loss, aux, terms, dl


@torch.library.custom_op("mrirt::inr_backward", mutates_args=())
def inr_backward(weights: torch.Tensor, dlogits: torch.Tensor, scratch: torch.Tensor, kind: int, num_layers: int, in_dim: int,
                 out_dim: int, hidden: int, fourier_freqs: int, num_mods: int, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(grad_w, grad_b) in the flat layouts of the weights / biases through mrirt_inr_backward, from dlogits [n, out_dim] and
    the ``scratch`` that ``inr_forward_f32`` returned for the same network and n."""
    d, nbytes, nw, nb = _train_desc(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, n)
    w = _dev_flat(weights, torch.float32, "weights")
    dl = _dev_flat(dlogits, torch.float32, "dlogits")
    if w.numel() < nw or dl.numel() < n * out_dim:
        raise ValueError("weights / dlogits are smaller than the network / [n, out_dim]")
    if not scratch.is_cuda or scratch.dtype != torch.uint8 or scratch.numel() < nbytes:
        raise TypeError(f"scratch: expected the {nbytes}-byte device buffer of inr_forward_f32")
    dev = _one_device([("weights", w), ("dlogits", dl), ("scratch", scratch)])
    with torch.cuda.device(dev):
        gw, gb = _backward_outs(nw, nb, dev)
        rc = _lib.lib().mrirt_inr_backward(C.byref(d), _ptr(w), int(n), _ptr(dl), _ptr(gw), _ptr(gb), 0, _ptr(scratch),
                                           scratch.numel(), _stream())
    _lib.check(rc, "mrirt_inr_backward")
    return gw, gb


@inr_backward.register_fake
def _(weights, dlogits, scratch, kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, n):
    _, _, nw, nb = _train_desc(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, n)
    return _backward_outs(nw, nb, weights.device)


# --- INR training loop: voxel sampler and clipped AdamW (csrc/inr_optim.hip) ------------------------------------------------
def _u64(v: int) -> int:
    return int(v) & 0xFFFFFFFFFFFFFFFF


def _sampler_cache(mods_table, seg_table, num_mods: int, h: int, w: int, d: int, extra: Sequence = ()):
    """The table checks and the MrirtInrCache of both samplers; ``extra``: further (name, device tensor) operands for the
    one-device check.  Returns (cache, ncases, the device)."""
    st = _dev_flat(seg_table, torch.int64, "seg_table")
    mt = _dev_flat(mods_table, torch.int64, "mods_table")
    if st.numel() < 1 or (num_mods > 0 and (mt is None or mt.numel() != st.numel())):
        raise ValueError("seg_table must hold one address per case, and mods_table as many when num_mods > 0")
    dev = _one_device([("seg_table", st), ("mods_table", mt)] + list(extra))
    c = _lib.InrCache()
    c.mods, c.seg, c.ncases, c.numMods = (mt.data_ptr() if num_mods > 0 else None), st.data_ptr(), st.numel(), num_mods
    c.hwd[0], c.hwd[1], c.hwd[2] = h, w, d
    return c, st.numel(), dev


def _sample_outs(n: int, num_mods: int, dev, **_):
    """coords [n, 3], feats [n, num_mods], labels int32 [n]."""
    return (torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, num_mods), dtype=torch.float32, device=dev),
            torch.empty(n, dtype=torch.int32, device=dev))


@torch.library.custom_op("mrirt::inr_sample_batch", mutates_args=())
def inr_sample_batch(mods_table: Optional[torch.Tensor], seg_table: torch.Tensor, num_mods: int, h: int, w: int, d: int, seed: int,
                     batch_index: int, n: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(coords fp32 [n, 3], feats fp32 [n, num_mods], labels int32 [n]) of mrirt_inr_sample_batch.  ``mods_table`` /
    ``seg_table`` are int64 device tensors of per-case device addresses (fp32 [num_mods, h, w, d] and int16 [h, w, d] volumes,
    which the caller keeps alive); ``seed`` and ``batch_index`` are taken modulo 2^64."""
    c, _, dev = _sampler_cache(mods_table, seg_table, num_mods, h, w, d)
    with torch.cuda.device(dev):
        coords, feats, labels = _sample_outs(n, num_mods, dev)
        rc = _lib.lib().mrirt_inr_sample_batch(C.byref(c), _u64(seed), _u64(batch_index), int(n), _ptr(coords),
                                               _ptr(feats) if num_mods > 0 else None, _ptr(labels), _stream())
    _lib.check(rc, "mrirt_inr_sample_batch")
    return coords, feats, labels


@torch.library.custom_op("mrirt::inr_sample_batch_mix", mutates_args=())
def inr_sample_batch_mix(mods_table: Optional[torch.Tensor], seg_table: torch.Tensor, tumour_index: Optional[torch.Tensor],
                         tumour_offsets: Optional[torch.Tensor], num_mods: int, h: int, w: int, d: int, seed: int, batch_index: int, n: int,
                         n_tumour: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``inr_sample_batch`` with the first ``n_tumour`` points drawn from the tumour voxels (mrirt_inr_sample_batch_mix):
    ``tumour_index`` holds the uint32 voxel offsets in an int32 device tensor, ``tumour_offsets`` is int64 [ncases + 1]
    (``VoxelCache.tumour_voxels`` / ``tumour_offsets``); both may be None when ``n_tumour`` is 0."""
    ti = _dev_flat(tumour_index, torch.int32, "tumour_index")
    to = _dev_flat(tumour_offsets, torch.int64, "tumour_offsets")
    c, ncases, dev = _sampler_cache(mods_table, seg_table, num_mods, h, w, d, extra=[("tumour_index", ti), ("tumour_offsets", to)])
    if n_tumour != 0 and (ti is None or to is None or to.numel() != ncases + 1):
        raise ValueError("n_tumour > 0 needs tumour_index and tumour_offsets [ncases + 1]")
    t = _lib.InrTumourIndex(ti.data_ptr(), to.data_ptr()) if n_tumour != 0 else None
    with torch.cuda.device(dev):
        coords, feats, labels = _sample_outs(n, num_mods, dev)
        rc = _lib.lib().mrirt_inr_sample_batch_mix(C.byref(c), C.byref(t) if t is not None else None, _u64(seed), _u64(batch_index), int(n),
                                                   int(n_tumour), _ptr(coords), _ptr(feats) if num_mods > 0 else None, _ptr(labels), _stream())
    _lib.check(rc, "mrirt_inr_sample_batch_mix")
    return coords, feats, labels


def _adamw_outs(w, b, mu_w, mu_b, nu_w, nu_b, dev, **_):
    """Copies of the parameters and moments for the update to run on, and gnorm fp64 [2]."""
    return [x.clone() for x in (w, b, mu_w, mu_b, nu_w, nu_b)] + [torch.empty(2, dtype=torch.float64, device=dev)]


@torch.library.custom_op("mrirt::inr_adamw_step", mutates_args=())
def inr_adamw_step(w: torch.Tensor, b: torch.Tensor, gw: torch.Tensor, gb: torch.Tensor, mu_w: torch.Tensor, mu_b: torch.Tensor,
                   nu_w: torch.Tensor, nu_b: torch.Tensor, lr: float, b1: float, b2: float, eps: float, weight_decay: float,
                   clip_norm: float, t: int, gscale: float) -> List[torch.Tensor]:
    """[w, b, mu_w, mu_b, nu_w, nu_b, gnorm] after update number t + 1 of mrirt_inr_adamw_step on copies of the flat fp32
    parameters and moments (the arguments are not changed); gnorm fp64 [2] = the global gradient norm and the clip factor."""
    ten = [_dev_flat(x, torch.float32, k) for k, x in (("w", w), ("b", b), ("gw", gw), ("gb", gb), ("mu_w", mu_w), ("mu_b", mu_b),
                                                        ("nu_w", nu_w), ("nu_b", nu_b))]
    nw, nb = ten[0].numel(), ten[1].numel()
    if any(x.numel() != nw for x in ten[2::2]) or any(x.numel() != nb for x in ten[3::2]):
        raise ValueError("gradients and moments must have the sizes of w and b")
    dev = _one_device([("w", ten[0])] + [("arg", x) for x in ten[1:]])
    lib = _lib.lib()
    hp = _lib.AdamW(lr, b1, b2, eps, weight_decay, clip_norm)
    with torch.cuda.device(dev):
        ow, ob, omw, omb, onw, onb, gnorm = _adamw_outs(w, b, mu_w, mu_b, nu_w, nu_b, dev)
        nbytes = int(lib.mrirt_inr_adamw_scratch_bytes(nw + nb))
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        rc = lib.mrirt_inr_adamw_step(_ptr(ow), _ptr(ob), _ptr(ten[2]), _ptr(ten[3]), _ptr(omw), _ptr(omb), _ptr(onw), _ptr(onb), nw, nb,
                                      C.byref(hp), _u64(t), float(gscale), _ptr(gnorm), _ptr(scratch), nbytes, _stream())
    _lib.check(rc, "mrirt_inr_adamw_step")
    return [ow, ob, omw, omb, onw, onb, gnorm]


# --- the fake kernels: every operator's own outs function, on the device of the named operand ------------------------------
_K1_BLOCKS = {"params": _lib.BratsParams, "ext": _lib.RenderExt}
render_mesh_fake = _shapes(render_mesh, _frame_outs, ["nodes"], {"params": _lib.MeshParams, "ext": _lib.RenderExt})
_shapes(render_brats, _frame_outs, ["vol0", "vol1", "vol2", "vol3"], _K1_BLOCKS)
_shapes(render_brats_backward, _brats_backward_outs, ["grad_out"], _K1_BLOCKS)
_shapes(render_brats_soft, _soft_outs, ["logits"], _K1_BLOCKS)
_shapes(render_brats_soft_backward, _soft_backward_outs, ["logits"])
_shapes(render_volume, _frame_outs, ["volume"], {"params": _lib.VolumeParams, "ext": _lib.RenderExt})
_shapes(render_sdf, _sdf_outs, ["like"])
_shapes(inr_forward, _logits_outs, ["weights"])
_shapes(edt_squared, _edt_outs, ["labels"])
_shapes(hausdorff, _hausdorff_outs, ["pred"])
_shapes(surface_count, _surface_count_outs, ["labels"])
_shapes(surface_extract, _surface_extract_outs, ["labels"])
_shapes(inr_loss, functools.partial(_loss_outs, terms=False), ["logits"])
_shapes(inr_loss_ext, functools.partial(_loss_outs, terms=True), ["logits"])
_shapes(inr_sample_batch, _sample_outs, ["seg_table"])
_shapes(inr_sample_batch_mix, _sample_outs, ["seg_table"])
_shapes(inr_adamw_step, _adamw_outs, ["w"])
