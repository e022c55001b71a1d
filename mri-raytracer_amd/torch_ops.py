"""``torch.ops.mrirt.*`` — the C ABI of libmrirt.so registered as PyTorch custom operators.

Device tensors in, a device tensor out, launched on the current HIP stream, no implicit
synchronisation.  The operators are thin: parameter blocks travel as
CPU ``uint8`` tensors holding the C structs of include/mrirt.h byte for byte (``pack_brats_params``
& co. build them from the reference's ``gParams`` dicts), every size check the C side cannot make
(it only sees pointers) is made here, and the launch itself is the same ``mrirt_*`` entry point the
rest of the package calls.  There is no CPU implementation: the only other registration is the
shape function ("fake" kernel) that ``torch.compile`` / meta tensors need.  The render operators also exist as a
C++ extension (``load_native()`` -> ``torch.ops.mrirt_native.*``, csrc/torch_binding.cpp).

    blob = mrirt.torch_ops.pack_brats_params(gparams)
    ext  = mrirt.torch_ops.pack_render_ext({"layout": "vg", **mrirt.synth.SHADE_EXT})
    img  = torch.ops.mrirt.render_brats(blob, ext, grid.data, None, None, None, None, None)
"""
from __future__ import annotations

import ctypes as C
from typing import Any, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .params import brats_params, mesh_params, render_ext, sdf_params, volume_params


def load_native():
    """``torch.ops.mrirt_native`` — the same render operators registered from C++ (csrc/torch_binding.cpp, a
    PyTorch-ROCm C++ extension linked to libmrirt.so; schemas as ``torch.ops.mrirt.render_*`` below).  Raises if
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


def _out_shape(width: int, height: int, E: _lib.RenderExt):
    if E.tileSize > 0:
        tiles_x = (width + E.tileSize - 1) // E.tileSize
        tiles_y = (height + E.tileSize - 1) // E.tileSize
        total = tiles_x * tiles_y
        local = (total - E.tileRank + E.tileWorld - 1) // E.tileWorld if E.tileRank < total else 0
        return (local, int(E.tileSize), int(E.tileSize), 4)
    return (height, width, 4)


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


# --- K1 -----------------------------------------------------------------------------------------
@torch.library.custom_op("mrirt::render_brats", mutates_args=())
def render_brats(params: torch.Tensor, ext: torch.Tensor, vol0: Optional[torch.Tensor], vol1: Optional[torch.Tensor],
                 vol2: Optional[torch.Tensor], vol3: Optional[torch.Tensor], labels: Optional[torch.Tensor],
                 preds: Optional[torch.Tensor]) -> torch.Tensor:
    """brats_main (inr/viewer/brats_rt.slang:85-168) through mrirt_render_brats_ex."""
    P, E = _unblob(params, _lib.BratsParams), _unblob(ext, _lib.RenderExt)
    dims = [int(v) for v in P.dims]
    vols = [_dev_flat(v, torch.float32, f"gIntensity{m}") for m, v in enumerate((vol0, vol1, vol2, vol3))]
    lab = _dev_flat(labels, torch.int32, "gLabels")
    prd = _dev_flat(preds, torch.int32, "gPreds")
    need, lneed = _grid_need(dims, E.layout), _grid_need(dims, E.labelLayout)
    mod4 = E.layout == _lib.LAYOUT_MOD4                  # vol0 = the float4 grid of all four modalities (vol1..3 are ignored)
    for m, v in enumerate(vols):
        if (m == 0 if mod4 else P.volEnabled[m] != 0) and (v is None or v.numel() < need):
            raise ValueError(f"gIntensity{m} is {'the MOD4 grid' if mod4 else 'enabled'} but holds {0 if v is None else v.numel()} < {need} elements")
    if P.showSeg != 0 and (lab is None or lab.numel() < lneed):
        raise ValueError("showSeg is set but gLabels is missing or too small")
    cells = E.labelLayout == _lib.LAYOUT_LABCELL     # gLabels carries both grids, gPreds is ignored
    if P.showPred != 0 and ((lab if cells else prd) is None or (lab if cells else prd).numel() < lneed):
        raise ValueError("showPred is set but gPreds (or the label-cell grid) is missing or too small")
    dev = _one_device([(f"gIntensity{m}", v) for m, v in enumerate(vols)] + [("gLabels", lab), ("gPreds", prd)])
    dt = torch.float16 if E.outFormat == _lib.OUT_RGBA16F else torch.float32
    vp = (C.c_void_p * 4)(*[C.c_void_p(v.data_ptr()) if v is not None else None for v in vols])
    with torch.cuda.device(dev):
        out = torch.empty(_out_shape(int(P.imageSize[0]), int(P.imageSize[1]), E), dtype=dt, device=dev)
        rc = _lib.lib().mrirt_render_brats_ex(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(prd), _ptr(out),
                                              int(P.imageSize[0]), None, _stream())
    _lib.check(rc, "mrirt_render_brats_ex")
    return out


@render_brats.register_fake
def _(params, ext, vol0, vol1, vol2, vol3, labels, preds):
    P, E = _unblob(params, _lib.BratsParams), _unblob(ext, _lib.RenderExt)
    dev = next(v.device for v in (vol0, vol1, vol2, vol3) if v is not None)
    dt = torch.float16 if E.outFormat == _lib.OUT_RGBA16F else torch.float32
    return torch.empty(_out_shape(int(P.imageSize[0]), int(P.imageSize[1]), E), dtype=dt, device=dev)


# --- K1 backward --------------------------------------------------------------------------------
def _present(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None or t.numel() == 0 else t


@torch.library.custom_op("mrirt::render_brats_backward", mutates_args=())
def render_brats_backward(params: torch.Tensor, ext: torch.Tensor, grad_out: torch.Tensor, vol0: Optional[torch.Tensor],
                          vol1: Optional[torch.Tensor], vol2: Optional[torch.Tensor], vol3: Optional[torch.Tensor],
                          labels: Optional[torch.Tensor], preds: Optional[torch.Tensor]
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Gradients of one K1 frame on LINEAR fp32 grids through mrirt_render_brats_backward: ``grad_out`` is dL/dframe, fp32
    [H, W, 4] (alpha ignored).  Returns dL/dvol0..3 (fp32 [X*Y*Z]; an empty tensor for a modality that is disabled or not
    bound — an empty tensor also stands for an absent modality on the way in) and dL/d(ww, wl, intensityAlpha, gamma) as
    float64 [4].  Freshly zeroed outputs: summing over views is the caller's ``+=``."""
    P, E = _unblob(params, _lib.BratsParams), _unblob(ext, _lib.RenderExt)
    dims = [int(v) for v in P.dims]
    nvox = dims[0] * dims[1] * dims[2]
    W, H = int(P.imageSize[0]), int(P.imageSize[1])
    vols = [_dev_flat(_present(v), torch.float32, f"gIntensity{m}") for m, v in enumerate((vol0, vol1, vol2, vol3))]
    lab = _dev_flat(_present(labels), torch.int32, "gLabels")
    prd = _dev_flat(_present(preds), torch.int32, "gPreds")
    g = _dev_flat(grad_out, torch.float32, "grad_out")
    if tuple(g.shape) != (H, W, 4):
        raise ValueError(f"grad_out: expected ({H}, {W}, 4), got {tuple(g.shape)}")
    for m, v in enumerate(vols):
        if P.volEnabled[m] != 0 and (v is None or v.numel() < nvox):
            raise ValueError(f"gIntensity{m} is enabled but holds {0 if v is None else v.numel()} < {nvox} elements")
    if P.showSeg != 0 and (lab is None or lab.numel() < nvox):
        raise ValueError("showSeg is set but gLabels is missing or too small")
    if P.showPred != 0 and (prd is None or prd.numel() < nvox):
        raise ValueError("showPred is set but gPreds is missing or too small")
    dev = _one_device([("grad_out", g)] + [(f"gIntensity{m}", v) for m, v in enumerate(vols)] + [("gLabels", lab), ("gPreds", prd)])
    vp = (C.c_void_p * 4)(*[C.c_void_p(v.data_ptr()) if v is not None else None for v in vols])
    with torch.cuda.device(dev):
        gv = [torch.zeros(nvox if (P.volEnabled[m] != 0 and vols[m] is not None) else 0, dtype=torch.float32, device=dev)
              for m in range(4)]
        gtf = torch.zeros(4, dtype=torch.float64, device=dev)
        gp = (C.c_void_p * 4)(*[C.c_void_p(t.data_ptr()) if t.numel() else None for t in gv])
        rc = _lib.lib().mrirt_render_brats_backward(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(prd), _ptr(g), W, gp, _ptr(gtf),
                                                    _stream())
    _lib.check(rc, "mrirt_render_brats_backward")
    return gv[0], gv[1], gv[2], gv[3], gtf


@render_brats_backward.register_fake
def _(params, ext, grad_out, vol0, vol1, vol2, vol3, labels, preds):
    P = _unblob(params, _lib.BratsParams)
    nvox = int(P.dims[0]) * int(P.dims[1]) * int(P.dims[2])
    gv = [torch.empty(nvox if (P.volEnabled[m] != 0 and v is not None and v.numel() != 0) else 0, dtype=torch.float32,
                      device=grad_out.device) for m, v in enumerate((vol0, vol1, vol2, vol3))]
    return gv[0], gv[1], gv[2], gv[3], torch.empty(4, dtype=torch.float64, device=grad_out.device)


# --- K1 soft prediction overlay -------------------------------------------------------------------
def _bind_soft(params, ext, logits, offsets, vols, labels, frame_like=None):
    """The checks the two soft-overlay operators share; returns (P, E, vol pointers, labels, device)."""
    P, E = _unblob(params, _lib.BratsParams), _unblob(ext, _lib.RenderExt)
    dims = [int(v) for v in P.dims]
    nvox = dims[0] * dims[1] * dims[2]
    W, H = int(P.imageSize[0]), int(P.imageSize[1])
    vols = [_dev_flat(_present(v), torch.float32, f"gIntensity{m}") for m, v in enumerate(vols)]
    lab = _dev_flat(_present(labels), torch.int32, "gLabels")
    z = _dev_flat(logits, torch.float32, "logits")
    off = _dev_flat(offsets, torch.int64, "offsets")
    if z.dim() != 2 or not 1 <= int(z.shape[1]) <= 16:
        raise ValueError(f"logits: expected (rows, 1..16 classes), got {tuple(z.shape)}")
    if off.numel() != W * H:
        raise ValueError(f"offsets: expected {W * H} elements (one per pixel), got {off.numel()}")
    for m, v in enumerate(vols):
        if P.volEnabled[m] != 0 and (v is None or v.numel() < nvox):
            raise ValueError(f"gIntensity{m} is enabled but holds {0 if v is None else v.numel()} < {nvox} elements")
    if P.showSeg != 0 and (lab is None or lab.numel() < nvox):
        raise ValueError("showSeg is set but gLabels is missing or too small")
    if frame_like is not None and tuple(frame_like.shape) != (H, W, 4):
        raise ValueError(f"grad_out: expected ({H}, {W}, 4), got {tuple(frame_like.shape)}")
    dev = _one_device([("logits", z), ("offsets", off), ("grad_out", frame_like)] + [(f"gIntensity{m}", v) for m, v in enumerate(vols)]
                      + [("gLabels", lab)])
    vp = (C.c_void_p * 4)(*[C.c_void_p(v.data_ptr()) if v is not None else None for v in vols])
    return P, E, vp, lab, dev


@torch.library.custom_op("mrirt::render_brats_soft", mutates_args=())
def render_brats_soft(params: torch.Tensor, ext: torch.Tensor, logits: torch.Tensor, offsets: torch.Tensor,
                      vol0: Optional[torch.Tensor], vol1: Optional[torch.Tensor], vol2: Optional[torch.Tensor],
                      vol3: Optional[torch.Tensor], labels: Optional[torch.Tensor]) -> torch.Tensor:
    """The soft-overlay K1 frame through mrirt_render_brats_soft: ``logits`` fp32 [rows, C], ``offsets`` int64 [H * W] (row of
    the first sample of every pixel); LINEAR fp32 grids.  Returns fp32 [H, W, 4]."""
    P, E, vp, lab, dev = _bind_soft(params, ext, logits, offsets, (vol0, vol1, vol2, vol3), labels)
    W, H = int(P.imageSize[0]), int(P.imageSize[1])
    with torch.cuda.device(dev):
        out = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        rc = _lib.lib().mrirt_render_brats_soft(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(logits), int(logits.shape[1]), _ptr(offsets),
                                                _ptr(out), W, None, _stream())
    _lib.check(rc, "mrirt_render_brats_soft")
    return out


@render_brats_soft.register_fake
def _(params, ext, logits, offsets, vol0, vol1, vol2, vol3, labels):
    P = _unblob(params, _lib.BratsParams)
    return torch.empty((int(P.imageSize[1]), int(P.imageSize[0]), 4), dtype=torch.float32, device=logits.device)


@torch.library.custom_op("mrirt::render_brats_soft_backward", mutates_args=())
def render_brats_soft_backward(params: torch.Tensor, ext: torch.Tensor, grad_out: torch.Tensor, logits: torch.Tensor,
                               offsets: torch.Tensor, vol0: Optional[torch.Tensor], vol1: Optional[torch.Tensor],
                               vol2: Optional[torch.Tensor], vol3: Optional[torch.Tensor], labels: Optional[torch.Tensor]
                               ) -> torch.Tensor:
    """dL/dlogits of the soft-overlay frame through mrirt_render_brats_soft_backward: ``grad_out`` is dL/dframe, fp32
    [H, W, 4] (alpha ignored).  Returns fp32 shaped like ``logits``, allocated zeroed (rows no ray owns stay zero)."""
    g = _dev_flat(grad_out, torch.float32, "grad_out")
    P, E, vp, lab, dev = _bind_soft(params, ext, logits, offsets, (vol0, vol1, vol2, vol3), labels, frame_like=g)
    with torch.cuda.device(dev):
        dl = torch.zeros_like(logits)
        rc = _lib.lib().mrirt_render_brats_soft_backward(C.byref(P), C.byref(E), vp, _ptr(lab), _ptr(logits), int(logits.shape[1]),
                                                         _ptr(offsets), _ptr(g), int(P.imageSize[0]), _ptr(dl), _stream())
    _lib.check(rc, "mrirt_render_brats_soft_backward")
    return dl


@render_brats_soft_backward.register_fake
def _(params, ext, grad_out, logits, offsets, vol0, vol1, vol2, vol3, labels):
    return torch.empty_like(logits)


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
    dt = torch.float16 if E.outFormat == _lib.OUT_RGBA16F else torch.float32
    with torch.cuda.device(vol.device):
        out = torch.empty(_out_shape(int(P.imageSize[0]), int(P.imageSize[1]), E), dtype=dt, device=vol.device)
        rc = _lib.lib().mrirt_render_volume(C.byref(P), C.byref(E), _ptr(vol), int(mode), _ptr(out), int(P.imageSize[0]),
                                            None, _stream())
    _lib.check(rc, "mrirt_render_volume")
    return out


@render_volume.register_fake
def _(params, ext, volume, mode):
    P, E = _unblob(params, _lib.VolumeParams), _unblob(ext, _lib.RenderExt)
    dt = torch.float16 if E.outFormat == _lib.OUT_RGBA16F else torch.float32
    return torch.empty(_out_shape(int(P.imageSize[0]), int(P.imageSize[1]), E), dtype=dt, device=volume.device)


# --- K3 -----------------------------------------------------------------------------------------
@torch.library.custom_op("mrirt::render_sdf", mutates_args=())
def render_sdf(params: torch.Tensor, width: int, height: int, like: torch.Tensor) -> torch.Tensor:
    """raymarch_cs (scripts/raymarch/raymarch.slang:60-99); ``like`` only names the device."""
    P = _unblob(params, _lib.SdfParams)
    if not like.is_cuda:
        raise TypeError("like: expected a device tensor")
    with torch.cuda.device(like.device):
        out = torch.empty((height, width, 4), dtype=torch.float32, device=like.device)
        rc = _lib.lib().mrirt_render_sdf(C.byref(P), int(width), int(height), _ptr(out), int(width), _stream())
    _lib.check(rc, "mrirt_render_sdf")
    return out


@render_sdf.register_fake
def _(params, width, height, like):
    return torch.empty((height, width, 4), dtype=torch.float32, device=like.device)


# --- K4 -----------------------------------------------------------------------------------------
@torch.library.custom_op("mrirt::render_mesh", mutates_args=())
def render_mesh(params: torch.Tensor, ext: torch.Tensor, nodes: torch.Tensor, tris: torch.Tensor, verts: torch.Tensor,
                max_depth: int) -> torch.Tensor:
    """compute_main (scripts/mesh_rt/mesh_rt.slang:138-164) through mrirt_render_mesh.  nodes: float32 [2N x 4], tris: int32
    [M x 4], verts: float32 [V x 4] (mrirt.upload_mesh's buffers; the counts are taken from their sizes); max_depth: the
    tree's depth (``Mesh.depth``).  The kernel stops, and paints, any ray that meets a malformed buffer; it never reads
    outside these three tensors."""
    P, E = _unblob(params, _lib.MeshParams), _unblob(ext, _lib.RenderExt)
    n = _dev_flat(nodes, torch.float32, "gBVHNodes")
    t = _dev_flat(tris, torch.int32, "gTris")
    v = _dev_flat(verts, torch.float32, "gVerts")
    dev = _one_device([("gBVHNodes", n), ("gTris", t), ("gVerts", v)])
    dt = torch.float16 if E.outFormat == _lib.OUT_RGBA16F else torch.float32
    with torch.cuda.device(dev):
        out = torch.empty((int(P.imageSize[1]), int(P.imageSize[0]), 4), dtype=dt, device=dev)
        rc = _lib.lib().mrirt_render_mesh(C.byref(P), C.byref(E), _ptr(n), n.numel() // 8, _ptr(t), t.numel() // 4, _ptr(v),
                                          v.numel() // 4, int(max_depth), _ptr(out), int(P.imageSize[0]), None, None, _stream())
    _lib.check(rc, "mrirt_render_mesh")
    return out


@render_mesh.register_fake
def render_mesh_fake(params, ext, nodes, tris, verts, max_depth):
    P, E = _unblob(params, _lib.MeshParams), _unblob(ext, _lib.RenderExt)
    dt = torch.float16 if E.outFormat == _lib.OUT_RGBA16F else torch.float32
    return torch.empty((int(P.imageSize[1]), int(P.imageSize[0]), 4), dtype=dt, device=nodes.device)


# --- INR ----------------------------------------------------------------------------------------
@torch.library.custom_op("mrirt::inr_forward", mutates_args=())
def inr_forward(weights: torch.Tensor, biases: torch.Tensor, kind: int, num_layers: int, in_dim: int, out_dim: int,
                hidden: int, fourier_freqs: int, num_mods: int, w0: float, coords: Optional[torch.Tensor],
                feats: Optional[torch.Tensor], n: int) -> torch.Tensor:
    """Logits [n, out_dim] of the packed MLP (``mrirt.inr.pack_mlp(...).weights / .biases``) for n points:
    inr/inr/model.py:21-50 (kind 0), notebooks/neumors_inr.ipynb:1165-1178 (kind 1), or the raw-input
    forms (kinds 2/3: ``feats`` is the [n, in_dim] input matrix)."""
    d = _lib.InrDesc()
    d.kind, d.numLayers, d.inDim, d.outDim, d.hidden = kind, num_layers, in_dim, out_dim, hidden
    d.fourierFreqs, d.numMods, d.w0 = fourier_freqs, num_mods, w0
    need = int(_lib.lib().mrirt_inr_pack_bytes(C.byref(d)))
    if need <= 0:
        raise ValueError("unsupported network shape")
    if not weights.is_cuda or weights.dtype != torch.uint8 or weights.numel() < need:
        raise TypeError(f"weights: expected the {need}-byte packed image of mrirt_inr_pack_weights on the device")
    nb = (num_layers - 1) * hidden + ((out_dim + 31) // 32) * 32
    bz = _dev_flat(biases, torch.float32, "biases")
    if bz.numel() < nb:
        raise ValueError(f"biases holds {bz.numel()} < {nb} floats (each layer padded to a multiple of 32)")
    co = _dev_flat(coords, torch.float32, "coords")
    fe = _dev_flat(feats, torch.float32, "feats")
    if kind < 2 and (co is None or co.numel() < 3 * n):
        raise ValueError("coords must hold [n, 3] floats")
    width = in_dim if kind >= 2 else num_mods
    if width > 0 and (fe is None or fe.numel() < width * n):
        raise ValueError(f"feats must hold [n, {width}] floats")
    d.weights, d.biases = weights.data_ptr(), bz.data_ptr()
    dev = _one_device([("weights", weights), ("biases", bz), ("coords", co), ("feats", fe)])
    with torch.cuda.device(dev):
        out = torch.empty((n, out_dim), dtype=torch.float32, device=dev)
        rc = _lib.lib().mrirt_inr_forward(C.byref(d), _ptr(co), _ptr(fe), int(n), _ptr(out), None, _stream())
    _lib.check(rc, "mrirt_inr_forward")
    return out


@inr_forward.register_fake
def _(weights, biases, kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, w0, coords, feats, n):
    return torch.empty((n, out_dim), dtype=torch.float32, device=weights.device)


# --- exact distance transform / Hausdorff -------------------------------------------------------
def _edt_args(labels: Sequence, spacing: Sequence[float]):
    vols = [_dev_flat(v, torch.int16, what) for what, v in labels]
    if any(v.dim() != 3 or v.shape != vols[0].shape for v in vols):
        raise ValueError("label volumes must be (H, W, D) int16 tensors of one shape")
    if len(spacing) != 3:
        raise ValueError("spacing: expected three values")
    return vols, (C.c_uint32 * 3)(*vols[0].shape), (C.c_float * 3)(*[float(np.float32(s)) for s in spacing])


@torch.library.custom_op("mrirt::edt_squared", mutates_args=())
def edt_squared(labels: torch.Tensor, cls: int, spacing: Sequence[float]) -> torch.Tensor:
    """fp64 (H, W, D): squared distance of every voxel to the nearest voxel with ``labels == cls`` (+inf when there is
    none), coordinates ``float32(index) * float32(spacing)`` — mrirt_edt_squared, exact."""
    (lab,), hwd, sp = _edt_args([("labels", labels)], spacing)
    lib = _lib.lib()
    with torch.cuda.device(lab.device):
        nbytes = int(lib.mrirt_edt_scratch_bytes(hwd, 0))
        out = torch.empty(tuple(lab.shape), dtype=torch.float64, device=lab.device)
        scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=lab.device)
        rc = lib.mrirt_edt_squared(_ptr(lab), hwd, int(cls), sp, _ptr(out), _ptr(scratch), nbytes, _stream())
    _lib.check(rc, "mrirt_edt_squared")
    return out


@edt_squared.register_fake
def _(labels, cls, spacing):
    return torch.empty(tuple(labels.shape), dtype=torch.float64, device=labels.device)


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
        out = torch.empty((max(int(num_classes), 0), 2), dtype=torch.float64, device=dev)
        scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=dev)
        rc = lib.mrirt_hausdorff(_ptr(p), _ptr(t), hwd, sp, int(num_classes), _ptr(out), _ptr(scratch), nbytes, _stream())
    _lib.check(rc, "mrirt_hausdorff")
    return out


@hausdorff.register_fake
def _(pred, truth, spacing, num_classes):
    return torch.empty((num_classes, 2), dtype=torch.float64, device=pred.device)


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


@torch.library.custom_op("mrirt::surface_count", mutates_args=())
def surface_count(labels: torch.Tensor, class_mask: int) -> torch.Tensor:
    """int64 [2] on the device: vertices and triangles of the surface of the voxels whose label's bit is set in
    ``class_mask`` (mrirt_surface_count).  No host synchronisation."""
    lab, hwd, nbytes = _surface_args(labels, class_mask)
    with torch.cuda.device(lab.device):
        counts = torch.empty(2, dtype=torch.int64, device=lab.device)
        scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=lab.device)
        rc = _lib.lib().mrirt_surface_count(_ptr(lab), hwd, int(class_mask), _ptr(scratch), nbytes, _ptr(counts), _stream())
    _lib.check(rc, "mrirt_surface_count")
    return counts


@surface_count.register_fake
def _(labels, class_mask):
    return torch.empty(2, dtype=torch.int64, device=labels.device)


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
        verts = torch.zeros((int(num_verts), 3), dtype=torch.float32, device=lab.device)
        tris = torch.zeros((int(num_tris), 3), dtype=torch.int32, device=lab.device)
        counts = torch.empty(2, dtype=torch.int64, device=lab.device)
        scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=lab.device)
        rc = _lib.lib().mrirt_surface_extract(_ptr(lab), hwd, int(class_mask), sp, org, _ptr(verts) if num_verts else None,
                                              int(num_verts), _ptr(tris) if num_tris else None, int(num_tris), _ptr(scratch),
                                              nbytes, _ptr(counts), _stream())
    _lib.check(rc, "mrirt_surface_extract")
    return verts, tris


@surface_extract.register_fake
def _(labels, class_mask, spacing, origin, num_verts, num_tris):
    return (torch.empty((num_verts, 3), dtype=torch.float32, device=labels.device),
            torch.empty((num_tris, 3), dtype=torch.int32, device=labels.device))


# --- INR training step (fp32; csrc/inr_train.hip) -----------------------------------------------
def _train_desc(kind: int, num_layers: int, in_dim: int, out_dim: int, hidden: int, fourier_freqs: int, num_mods: int, n: int):
    d = _lib.InrDesc()
    d.kind, d.numLayers, d.inDim, d.outDim, d.hidden = kind, num_layers, in_dim, out_dim, hidden
    d.fourierFreqs, d.numMods = fourier_freqs, num_mods
    nbytes = int(_lib.lib().mrirt_inr_train_scratch_bytes(C.byref(d), int(n)))
    if nbytes <= 0:
        raise ValueError("unsupported network kind / shape / n for the training step (ReLU kinds only)")
    nw = in_dim * hidden + (num_layers - 2) * hidden * hidden + hidden * out_dim
    nb = (num_layers - 1) * hidden + out_dim
    return d, nbytes, nw, nb


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
    co = _dev_flat(coords, torch.float32, "coords")
    fe = _dev_flat(feats, torch.float32, "feats")
    if kind < 2 and (co is None or co.numel() < 3 * n):
        raise ValueError("coords must hold [n, 3] floats")
    width = in_dim if kind >= 2 else num_mods
    if width > 0 and (fe is None or fe.numel() < width * n):
        raise ValueError(f"feats must hold [n, {width}] floats")
    dev = _one_device([("weights", w), ("biases", b), ("coords", co), ("feats", fe)])
    with torch.cuda.device(dev):
        out = torch.empty((n, out_dim), dtype=torch.float32, device=dev)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rc = _lib.lib().mrirt_inr_forward_f32(C.byref(d), _ptr(w), _ptr(b), _ptr(co), _ptr(fe), int(n), _ptr(out), _ptr(scratch),
                                              nbytes, _stream())
    _lib.check(rc, "mrirt_inr_forward_f32")
    return out, scratch


@inr_forward_f32.register_fake
def _(weights, biases, kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, coords, feats, n):
    return (torch.empty((n, out_dim), dtype=torch.float32, device=weights.device),
            torch.empty(_train_desc(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, n)[1], dtype=torch.uint8,
                        device=weights.device))


@torch.library.custom_op("mrirt::inr_loss", mutates_args=())
def inr_loss(logits: torch.Tensor, labels: torch.Tensor, class_weights: Sequence[float],
             dice_weight: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss fp32 [1], aux fp32 [2, C]: CE per class and Dice per class, dlogits fp32 [n, C]) of mrirt_inr_loss
    (inr/inr/model.py:64-88) on logits [n, C] and int32 labels [n]."""
    z = _dev_flat(logits, torch.float32, "logits")
    lab = _dev_flat(labels, torch.int32, "labels")
    if z.dim() != 2 or z.shape[0] < 1 or lab.numel() != z.shape[0]:
        raise ValueError("logits must be [n, C] with n >= 1 and labels [n]")
    n, nc = int(z.shape[0]), int(z.shape[1])
    if not 1 <= nc <= 16 or len(class_weights) != nc:
        raise ValueError("1..16 classes, one class weight each")
    dev = _one_device([("logits", z), ("labels", lab)])
    lib = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = int(lib.mrirt_inr_loss_scratch_bytes(n))
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        aux = torch.empty((2, nc), dtype=torch.float32, device=dev)
        dl = torch.empty_like(z)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rc = lib.mrirt_inr_loss(_ptr(z), _ptr(lab), n, nc, (C.c_float * nc)(*[float(np.float32(v)) for v in class_weights]),
                                float(dice_weight), _ptr(loss), _ptr(aux), _ptr(dl), _ptr(scratch), nbytes, _stream())
    _lib.check(rc, "mrirt_inr_loss")
    return loss, aux, dl


@inr_loss.register_fake
def _(logits, labels, class_weights, dice_weight):
    return (torch.empty(1, dtype=torch.float32, device=logits.device),
            torch.empty((2, logits.shape[1]), dtype=torch.float32, device=logits.device), torch.empty_like(logits))


@torch.library.custom_op("mrirt::inr_loss_ext", mutates_args=())
def inr_loss_ext(logits: torch.Tensor, labels: torch.Tensor, class_weights: Sequence[float], focal_alpha: Sequence[float], dice_weight: float,
                 per_class_dice: bool, focal_gamma: float, label_smoothing: float, edema_fp_weight: float, tversky_alpha: float,
                 tversky_beta: float, tversky_weight: float, edema_logit_reg: float,
                 edema_class: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss fp32 [1], aux fp32 [2, C], terms fp32 [5]: CE, Dice loss, edema FP / n, Tversky index, logit-regulariser mean,
    dlogits fp32 [n, C]) of mrirt_inr_loss_ext (scripts/jax_inr_brats.py:205-257) on logits [n, C] and int32 labels [n].
    An empty ``focal_alpha`` leaves the focal factor unweighted."""
    z = _dev_flat(logits, torch.float32, "logits")
    lab = _dev_flat(labels, torch.int32, "labels")
    if z.dim() != 2 or z.shape[0] < 1 or lab.numel() != z.shape[0]:
        raise ValueError("logits must be [n, C] with n >= 1 and labels [n]")
    n, nc = int(z.shape[0]), int(z.shape[1])
    if not 1 <= nc <= 16 or len(class_weights) != nc or len(focal_alpha) not in (0, nc):
        raise ValueError("1..16 classes, one class weight each, focal_alpha empty or one value per class")
    x = _lib.InrLossExt()
    for k in range(nc):
        x.classWeights[k] = float(class_weights[k])
        if len(focal_alpha):
            x.focalAlpha[k] = float(focal_alpha[k])
    x.diceWeight, x.focalGamma, x.labelSmoothing = float(dice_weight), float(focal_gamma), float(label_smoothing)
    x.edemaFpWeight, x.tverskyAlpha, x.tverskyBeta = float(edema_fp_weight), float(tversky_alpha), float(tversky_beta)
    x.tverskyWeight, x.edemaLogitReg, x.edemaClass = float(tversky_weight), float(edema_logit_reg), int(edema_class)
    x.flags = (_lib.LOSS_PER_CLASS_DICE if per_class_dice else 0) | (_lib.LOSS_FOCAL_ALPHA if len(focal_alpha) else 0)
    dev = _one_device([("logits", z), ("labels", lab)])
    lib = _lib.lib()
    with torch.cuda.device(dev):
        nbytes = int(lib.mrirt_inr_loss_ext_scratch_bytes(n))
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        aux = torch.empty((2, nc), dtype=torch.float32, device=dev)
        terms = torch.empty(5, dtype=torch.float32, device=dev)
        dl = torch.empty_like(z)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rc = lib.mrirt_inr_loss_ext(_ptr(z), _ptr(lab), n, nc, C.byref(x), _ptr(loss), _ptr(aux), _ptr(terms), _ptr(dl), _ptr(scratch), nbytes,
                                    _stream())
    _lib.check(rc, "mrirt_inr_loss_ext")
    return loss, aux, terms, dl


@inr_loss_ext.register_fake
def _(logits, labels, class_weights, focal_alpha, dice_weight, per_class_dice, focal_gamma, label_smoothing, edema_fp_weight, tversky_alpha,
      tversky_beta, tversky_weight, edema_logit_reg, edema_class):
    return (torch.empty(1, dtype=torch.float32, device=logits.device), torch.empty((2, logits.shape[1]), dtype=torch.float32, device=logits.device),
            torch.empty(5, dtype=torch.float32, device=logits.device), torch.empty_like(logits))


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
        gw = torch.empty(nw, dtype=torch.float32, device=dev)
        gb = torch.empty(nb, dtype=torch.float32, device=dev)
        rc = _lib.lib().mrirt_inr_backward(C.byref(d), _ptr(w), int(n), _ptr(dl), _ptr(gw), _ptr(gb), 0, _ptr(scratch),
                                           scratch.numel(), _stream())
    _lib.check(rc, "mrirt_inr_backward")
    return gw, gb


@inr_backward.register_fake
def _(weights, dlogits, scratch, kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, n):
    _, _, nw, nb = _train_desc(kind, num_layers, in_dim, out_dim, hidden, fourier_freqs, num_mods, n)
    return (torch.empty(nw, dtype=torch.float32, device=weights.device), torch.empty(nb, dtype=torch.float32, device=weights.device))


# --- INR training loop: voxel sampler and clipped AdamW (csrc/inr_optim.hip) ------------------------------------------------
def _u64(v: int) -> int:
    return int(v) & 0xFFFFFFFFFFFFFFFF


@torch.library.custom_op("mrirt::inr_sample_batch", mutates_args=())
def inr_sample_batch(mods_table: Optional[torch.Tensor], seg_table: torch.Tensor, num_mods: int, h: int, w: int, d: int, seed: int,
                     batch_index: int, n: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(coords fp32 [n, 3], feats fp32 [n, num_mods], labels int32 [n]) of mrirt_inr_sample_batch.  ``mods_table`` /
    ``seg_table`` are int64 device tensors of per-case device addresses (fp32 [num_mods, h, w, d] and int16 [h, w, d] volumes,
    which the caller keeps alive); ``seed`` and ``batch_index`` are taken modulo 2^64."""
    st = _dev_flat(seg_table, torch.int64, "seg_table")
    mt = _dev_flat(mods_table, torch.int64, "mods_table")
    if st.numel() < 1 or (num_mods > 0 and (mt is None or mt.numel() != st.numel())):
        raise ValueError("seg_table must hold one address per case, and mods_table as many when num_mods > 0")
    dev = _one_device([("seg_table", st), ("mods_table", mt)])
    c = _lib.InrCache()
    c.mods, c.seg, c.ncases, c.numMods = (mt.data_ptr() if num_mods > 0 else None), st.data_ptr(), st.numel(), num_mods
    c.hwd[0], c.hwd[1], c.hwd[2] = h, w, d
    with torch.cuda.device(dev):
        coords = torch.empty((n, 3), dtype=torch.float32, device=dev)
        feats = torch.empty((n, num_mods), dtype=torch.float32, device=dev)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        rc = _lib.lib().mrirt_inr_sample_batch(C.byref(c), _u64(seed), _u64(batch_index), int(n), _ptr(coords),
                                               _ptr(feats) if num_mods > 0 else None, _ptr(labels), _stream())
    _lib.check(rc, "mrirt_inr_sample_batch")
    return coords, feats, labels


@inr_sample_batch.register_fake
def _(mods_table, seg_table, num_mods, h, w, d, seed, batch_index, n):
    dev = seg_table.device
    return (torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, num_mods), dtype=torch.float32, device=dev),
            torch.empty(n, dtype=torch.int32, device=dev))


@torch.library.custom_op("mrirt::inr_sample_batch_mix", mutates_args=())
def inr_sample_batch_mix(mods_table: Optional[torch.Tensor], seg_table: torch.Tensor, tumour_index: Optional[torch.Tensor],
                         tumour_offsets: Optional[torch.Tensor], num_mods: int, h: int, w: int, d: int, seed: int, batch_index: int, n: int,
                         n_tumour: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``inr_sample_batch`` with the first ``n_tumour`` points drawn from the tumour voxels (mrirt_inr_sample_batch_mix):
    ``tumour_index`` holds the uint32 voxel offsets in an int32 device tensor, ``tumour_offsets`` is int64 [ncases + 1]
    (``VoxelCache.tumour_voxels`` / ``tumour_offsets``); both may be None when ``n_tumour`` is 0."""
    st = _dev_flat(seg_table, torch.int64, "seg_table")
    mt = _dev_flat(mods_table, torch.int64, "mods_table")
    ti = _dev_flat(tumour_index, torch.int32, "tumour_index")
    to = _dev_flat(tumour_offsets, torch.int64, "tumour_offsets")
    if st.numel() < 1 or (num_mods > 0 and (mt is None or mt.numel() != st.numel())):
        raise ValueError("seg_table must hold one address per case, and mods_table as many when num_mods > 0")
    if n_tumour != 0 and (ti is None or to is None or to.numel() != st.numel() + 1):
        raise ValueError("n_tumour > 0 needs tumour_index and tumour_offsets [ncases + 1]")
    dev = _one_device([("seg_table", st), ("mods_table", mt), ("tumour_index", ti), ("tumour_offsets", to)])
    c = _lib.InrCache()
    c.mods, c.seg, c.ncases, c.numMods = (mt.data_ptr() if num_mods > 0 else None), st.data_ptr(), st.numel(), num_mods
    c.hwd[0], c.hwd[1], c.hwd[2] = h, w, d
    t = _lib.InrTumourIndex(ti.data_ptr(), to.data_ptr()) if n_tumour != 0 else None
    with torch.cuda.device(dev):
        coords = torch.empty((n, 3), dtype=torch.float32, device=dev)
        feats = torch.empty((n, num_mods), dtype=torch.float32, device=dev)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        rc = _lib.lib().mrirt_inr_sample_batch_mix(C.byref(c), C.byref(t) if t is not None else None, _u64(seed), _u64(batch_index), int(n),
                                                   int(n_tumour), _ptr(coords), _ptr(feats) if num_mods > 0 else None, _ptr(labels), _stream())
    _lib.check(rc, "mrirt_inr_sample_batch_mix")
    return coords, feats, labels


@inr_sample_batch_mix.register_fake
def _(mods_table, seg_table, tumour_index, tumour_offsets, num_mods, h, w, d, seed, batch_index, n, n_tumour):
    dev = seg_table.device
    return (torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, num_mods), dtype=torch.float32, device=dev),
            torch.empty(n, dtype=torch.int32, device=dev))


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
        ow, ob, omw, omb, onw, onb = (ten[i].clone() for i in (0, 1, 4, 5, 6, 7))
        nbytes = int(lib.mrirt_inr_adamw_scratch_bytes(nw + nb))
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        gnorm = torch.empty(2, dtype=torch.float64, device=dev)
        rc = lib.mrirt_inr_adamw_step(_ptr(ow), _ptr(ob), _ptr(ten[2]), _ptr(ten[3]), _ptr(omw), _ptr(omb), _ptr(onw), _ptr(onb), nw, nb,
                                      C.byref(hp), _u64(t), float(gscale), _ptr(gnorm), _ptr(scratch), nbytes, _stream())
    _lib.check(rc, "mrirt_inr_adamw_step")
    return [ow, ob, omw, omb, onw, onb, gnorm]


@inr_adamw_step.register_fake
def _(w, b, gw, gb, mu_w, mu_b, nu_w, nu_b, lr, b1, b2, eps, weight_decay, clip_norm, t, gscale):
    return [torch.empty_like(w), torch.empty_like(b), torch.empty_like(mu_w), torch.empty_like(mu_b), torch.empty_like(nu_w),
            torch.empty_like(nu_b), torch.empty(2, dtype=torch.float64, device=w.device)]
