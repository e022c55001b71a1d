"""Load-time volume preparation: the NumPy host code either side of the kernels.

Mirrors (array-in/array-out, no NIfTI dependency):
  * ``load_nifti_float`` / ``load_seg_uint`` / world scaling / ``frame_volume`` —
    inr/viewer/brats_viewer.py:46-74,204-210,320-324
  * u8 packing, NIfTI-mask mapping and the BC4 block decode —
    scripts/volumeRendering/app.py:145-250
These run once per case on the host (as in the reference); per-frame work is all on the GPU.
The ``*_device`` functions at the end are the same preparation on the GPU (csrc/prep.hip): the percentile window
and normalisation, the z-score and scipy.ndimage's Gaussian filter, bit for bit what the host definitions give.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


def normalize_intensity(data: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(X,Y,Z) raw intensities -> (linear fp32 x-fastest buffer, normalised (X,Y,Z) array, dims).
    Percentile-1/99.5 window mapped to [0,1] (brats_viewer.py:50-65)."""
    vol = np.asarray(data, dtype=np.float32)
    lo, hi = float(np.percentile(vol, 1.0)), float(np.percentile(vol, 99.5))
    if hi <= lo:
        lo, hi = float(vol.min()), float(vol.max())
    span = max(1e-6, hi - lo)
    norm = np.clip((vol - lo) / span, 0.0, 1.0).astype(np.float32)
    return flatten_xyz(norm), norm, np.asarray(norm.shape, dtype=np.uint32)


def flatten_xyz(vol_xyz: np.ndarray) -> np.ndarray:
    """(X,Y,Z) -> 1-D with x fastest, i.e. index x + y*X + z*X*Y (brats_viewer.py:64,73)."""
    return np.ascontiguousarray(np.transpose(vol_xyz, (2, 1, 0)).reshape(-1))


def labels_to_uint(data: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Segmentation (X,Y,Z) float -> (linear uint32 buffer, dims) (brats_viewer.py:68-74)."""
    lab = np.rint(np.asarray(data, dtype=np.float32)).astype(np.uint32)
    return flatten_xyz(lab), np.asarray(lab.shape, dtype=np.uint32)


def world_frame(dims, zooms):
    """Voxel size, box origin, camera target and radius for a volume (brats_viewer.py:206-210,322-324):
    the longest axis spans 1.8 world units, centred on the origin."""
    d = np.asarray(dims).astype(np.uint32)
    k = np.float32(1.8 / float(max(d)))
    voxel_size = (np.asarray(zooms, dtype=np.float32) * k).astype(np.float32)
    extent = voxel_size * d.astype(np.float32)
    vol_min = (-0.5 * extent).astype(np.float32)
    target = (vol_min + 0.5 * extent).astype(np.float32)
    radius = float(np.linalg.norm(extent) * 0.8)
    return voxel_size, vol_min, target, radius


def pack_u8_as_u32x4(voxels_u8: np.ndarray) -> np.ndarray:
    """The reference's ``gVolumeU8`` upload: pad to a multiple of 4, widen every byte to uint32,
    view as rows of 4 (app.py:149-153).  Kept for drop-in parity; ``mode='u8'`` avoids the 4x."""
    flat = np.asarray(voxels_u8, dtype=np.uint8).reshape(-1)
    if flat.size % 4:
        flat = np.concatenate([flat, np.zeros(4 - flat.size % 4, dtype=np.uint8)])
    return flat.astype(np.uint32).reshape(-1, 4)


def mask_to_u8(data: np.ndarray, mode: str = "occupancy") -> np.ndarray:
    """NIfTI mask (X,Y,Z) -> flattened (Z,Y,X) u8 (app.py:180-197)."""
    vol = np.asarray(data, dtype=np.float32)
    if mode == "occupancy":
        u8 = np.where(vol > 0.5, 255, 0).astype(np.uint8)
    elif mode == "labels":
        u8 = np.zeros(vol.shape, dtype=np.uint8)
        for value, code in ((1.0, 85), (2.0, 170), (4.0, 255)):
            u8[np.isclose(vol, value)] = code
    else:
        raise ValueError(f"mask_mode must be 'occupancy' or 'labels', got {mode!r}")
    return flatten_xyz(u8)


def bc4_decode(bc: bytes, width: int, height: int, depth: int) -> np.ndarray:
    """BC4 (RGTC1 unorm) slices -> flattened u8 voxels (app.py:200-248).  8-byte blocks:
    two endpoints + 16 three-bit codes; r0 > r1 -> 6 interpolants, else 4 plus 0 and 255."""
    bw, bh = (width + 3) // 4, (height + 3) // 4
    want = depth * bw * bh * 8
    if len(bc) != want:
        raise RuntimeError(f"a {depth}x{height}x{width} BC4 volume is {want} bytes of 8-byte blocks, got {len(bc)}")
    blk = np.frombuffer(bc, dtype=np.uint8).reshape(depth, bh, bw, 8)
    r0 = blk[..., 0].astype(np.int32)
    r1 = blk[..., 1].astype(np.int32)
    bits = np.zeros(blk.shape[:-1], dtype=np.uint64)
    for k in range(6):
        bits |= blk[..., 2 + k].astype(np.uint64) << np.uint64(8 * k)
    six = r0 > r1
    pal = np.empty(blk.shape[:-1] + (8,), dtype=np.int32)
    pal[..., 0], pal[..., 1] = r0, r1
    for i in range(1, 7):
        a = ((7 - i) * r0 + i * r1 + 3) // 7
        if i <= 4:
            b = ((5 - i) * r0 + i * r1 + 2) // 5
        else:
            b = np.full_like(r0, 0 if i == 5 else 255)
        pal[..., i + 1] = np.where(six, a, b)
    codes = (bits[..., None] >> (np.arange(16, dtype=np.uint64) * np.uint64(3))) & np.uint64(7)
    texels = np.take_along_axis(pal, codes.astype(np.int64), axis=-1).astype(np.uint8)   # (D,bh,bw,16)
    img = texels.reshape(depth, bh, bw, 4, 4).transpose(0, 1, 3, 2, 4).reshape(depth, bh * 4, bw * 4)
    return np.ascontiguousarray(img[:, :height, :width]).reshape(-1)


def bc4_decode_device(bc, width: int, height: int, depth: int, stream=None):
    """The same decode on the GPU (csrc/grid_ops.hip): ``bc`` is the block stream as bytes, a NumPy uint8
    array or a device uint8 tensor; returns the flattened (D*H*W,) device uint8 tensor, ready to be bound as
    ``gVolumeU8`` with ``mode='u8'``."""
    import ctypes as C
    import torch
    from . import _lib
    if not torch.cuda.is_available():
        raise RuntimeError("bc4_decode_device needs an MI355X; volume.bc4_decode is the host decode")
    bw, bh = (width + 3) // 4, (height + 3) // 4
    want = depth * bw * bh * 8
    if isinstance(bc, (bytes, bytearray, memoryview)):
        bc = np.frombuffer(bytes(bc), dtype=np.uint8).copy()
    t = torch.as_tensor(bc)
    if t.dtype != torch.uint8 or t.numel() != want:
        raise RuntimeError(f"a {depth}x{height}x{width} BC4 volume is {want} bytes of 8-byte blocks, got {t.numel()}")
    t = t.reshape(-1).cuda().contiguous()
    out = torch.empty(depth * height * width, dtype=torch.uint8, device=t.device)
    s = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    _lib.check(_lib.lib().mrirt_bc4_decode(C.c_void_p(t.data_ptr()), width, height, depth, C.c_void_p(out.data_ptr()), s),
               "mrirt_bc4_decode")
    return out


def zscore_nonzero(arr: np.ndarray) -> np.ndarray:
    """Per-modality z-score over non-zero voxels, sigma + 1e-6 (brats_viewer.py:281-287)."""
    a = np.asarray(arr, dtype=np.float32)
    nz = a != 0
    if nz.any():
        a = (a - a[nz].mean()) / (a[nz].std() + 1e-6)
    return a


# --- the same preparation on the GPU (csrc/prep.hip) ----------------------------------------------------------------------
GAUSS_MAX_RADIUS = 16


def _device_f32(x):
    """NumPy array or tensor -> contiguous fp32 tensor on the GPU (a device fp32 tensor is used as it is)."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("the *_device preparation needs an MI355X; the functions without the suffix are the host code")
    if not isinstance(x, torch.Tensor):
        a = np.ascontiguousarray(x, dtype=np.float32)
        x = torch.from_numpy(a if a.flags.writeable else a.copy())
    t = x
    return t.to(device="cuda", dtype=torch.float32).contiguous()


def _stream(stream):
    import ctypes as C
    import torch
    return C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def _ptr(t):
    import ctypes as C
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dims3(shape):
    import ctypes as C
    return (C.c_uint32 * 3)(*[int(v) for v in shape])


def prep_window_device(vol, percentiles=(1.0, 99.5), stream=None):
    """The window record of a volume, on the device: 8 floats { lo, hi, span, min, max, p_lo, p_hi, 0 } with p = np.percentile
    (fp32, ``linear``) and the min / max fallback of :func:`normalize_intensity`.  Nothing is read back."""
    import torch
    from . import _lib
    t = _device_f32(vol)
    n = t.numel()
    l = _lib.lib()
    need = l.mrirt_prep_scratch_bytes(n)
    if need == 0:
        raise ValueError(f"a volume of {n} values is outside 1 .. 2^31 - 1")
    scratch = torch.empty(need, dtype=torch.uint8, device=t.device)
    record = torch.empty(8, dtype=torch.float32, device=t.device)
    _lib.check(l.mrirt_prep_window(_ptr(t), n, float(percentiles[0]), float(percentiles[1]), _ptr(record), _ptr(scratch), need,
                                   _stream(stream)), "mrirt_prep_window")
    return record


def normalize_intensity_device(data, percentiles=(1.0, 99.5), stream=None):
    """:func:`normalize_intensity` on the GPU: (X,Y,Z) raw intensities (NumPy or device tensor) -> (linear, norm, dims,
    window); ``linear`` (x fastest) and ``norm`` (X,Y,Z) are device fp32 tensors equal to the host function's arrays,
    ``dims`` the same uint32 array, ``window`` the device record of :func:`prep_window_device`."""
    import torch
    from . import _lib
    t = _device_f32(data)
    if t.dim() != 3:
        raise ValueError(f"expected an (X,Y,Z) volume, got shape {tuple(t.shape)}")
    window = prep_window_device(t, percentiles, stream)
    norm = torch.empty_like(t)
    linear = torch.empty(t.numel(), dtype=torch.float32, device=t.device)
    _lib.check(_lib.lib().mrirt_prep_normalize(_ptr(t), _dims3(t.shape), _ptr(window), _ptr(norm), _ptr(linear), _stream(stream)),
               "mrirt_prep_normalize")
    return linear, norm, np.asarray(t.shape, dtype=np.uint32), window


def zscore_nonzero_device(mods, out=None, stream=None):
    """:func:`zscore_nonzero` of every modality on the GPU.  ``mods``: (M, ...) — each ``mods[m]`` is z-scored on its own —
    or one 3-D volume.  Returns (z, stats): ``z`` a device fp32 tensor of the input's shape (``out=mods`` works in place),
    ``stats`` a device fp32 (4, M) tensor { mu, sigma, sigma + 1e-6, count (its uint32 bits) }: rows 0 and 2 are the
    ``zmu`` / ``zsigma`` that render_brats_inr and render_brats_inr_autograd take (they divide by zsigma as given, so it is
    the row WITH the 1e-6).  mu and sigma come from fp64 sums in a fixed order."""
    import torch
    from . import _lib
    t = _device_f32(mods)
    single = t.dim() == 3
    M = 1 if single else int(t.shape[0])
    if t.dim() < 2 or M < 1:
        raise ValueError(f"expected (M, ...) modalities or one volume, got shape {tuple(t.shape)}")
    n = t.numel() // M
    l = _lib.lib()
    need = l.mrirt_prep_zscore_scratch_bytes(n, M)
    if need == 0:
        raise ValueError(f"{M} modalities of {n} values are outside the limits (1..64 modalities of 1 .. 2^31 - 1 values)")
    scratch = torch.empty(need, dtype=torch.uint8, device=t.device)
    stats = torch.empty((4, M), dtype=torch.float32, device=t.device)
    z = torch.empty_like(t) if out is None else out
    if z.shape != t.shape or z.dtype != torch.float32 or not z.is_cuda or not z.is_contiguous():
        raise ValueError("out must be a contiguous device fp32 tensor of the input's shape")
    s = _stream(stream)
    _lib.check(l.mrirt_prep_zscore_stats(_ptr(t), n, M, _ptr(stats), _ptr(scratch), need, s), "mrirt_prep_zscore_stats")
    _lib.check(l.mrirt_prep_zscore_apply(_ptr(t), n, M, _ptr(stats), _ptr(z), s), "mrirt_prep_zscore_apply")
    return z, stats


def zscore_constants(stats):
    """Host copies of a stats record: (zmu, zsigma, count) with zsigma = sigma + 1e-6, the divisor the INR renders expect."""
    h = stats.detach().cpu().numpy()
    return h[0].copy(), h[2].copy(), h[3].view(np.uint32).copy()


def gaussian_weights(sigma: float) -> np.ndarray:
    """SciPy's Gaussian kernel for ``sigma``: radius int(4 sigma + 0.5), exp(-0.5 / sigma^2 x^2) over its sum, NumPy fp64."""
    sigma = float(sigma)
    if not (sigma > 0.0 and np.isfinite(sigma)):
        raise ValueError(f"sigma must be positive and finite, got {sigma}")
    r = int(4.0 * sigma + 0.5)
    if r > GAUSS_MAX_RADIUS:
        raise ValueError(f"sigma {sigma} needs radius {r} > {GAUSS_MAX_RADIUS}")
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


def gaussian_filter_device(vol, sigma, out=None, stream=None):
    """scipy.ndimage.gaussian_filter(vol, sigma) (fp32, mode ``reflect``) of a 3-D volume on the GPU, bit for bit.
    ``out`` may be ``vol`` itself (a device tensor) for an in-place filter."""
    import ctypes as C
    import torch
    from . import _lib
    t = _device_f32(vol)
    if t.dim() != 3:
        raise ValueError(f"expected a 3-D volume, got shape {tuple(t.shape)}")
    w = gaussian_weights(sigma)
    r = (len(w) - 1) // 2
    res = torch.empty_like(t) if out is None else out
    if res.shape != t.shape or res.dtype != torch.float32 or not res.is_cuda or not res.is_contiguous():
        raise ValueError("out must be a contiguous device fp32 tensor of the input's shape")
    scratch = torch.empty_like(t)
    wc = (C.c_double * len(w))(*w.tolist())
    _lib.check(_lib.lib().mrirt_prep_gaussian3d(_ptr(t), _dims3(t.shape), wc, r, _ptr(res), _ptr(scratch), _stream(stream)),
               "mrirt_prep_gaussian3d")
    return res
