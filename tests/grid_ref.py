"""NumPy restatements of the load-time grid layouts and of the skip-map inputs, from their documented definitions
(include/mrirt.h, the comments of csrc/mrirt_device.h and csrc/mrirt_host.h).  TEST INFRASTRUCTURE ONLY.

Every builder takes a linear grid as a ``[Z][Y][X]`` array (x fastest) and returns the WHOLE destination buffer, pad
elements included, so a test can demand ``==`` on every byte the device wrote.  Nothing here imports the package.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

F = np.float32


def _zyx(lin, dims, dtype=None) -> np.ndarray:
    X, Y, Z = (int(v) for v in dims)
    a = np.asarray(lin) if dtype is None else np.asarray(lin, dtype=dtype)
    return a.reshape(Z, Y, X)


def _coords(dims):
    X, Y, Z = (int(v) for v in dims)
    return np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")      # z, y, x


# ----------------------------------------------------------------------------------------------------------------------
# VG / QUAD / MOD4: float4 per voxel in 2x2x2 bricks, bricks x-fastest
# ----------------------------------------------------------------------------------------------------------------------
def vec4_elem(dims) -> Tuple[np.ndarray, int]:
    """(element index of every voxel as a [Z][Y][X] array, number of elements of the padded grid)."""
    X, Y, Z = (int(v) for v in dims)
    nbx, nby, nbz = (X + 1) // 2, (Y + 1) // 2, (Z + 1) // 2
    z, y, x = _coords(dims)
    e = 8 * ((x >> 1) + nbx * ((y >> 1) + nby * (z >> 1))) + (x & 1) + 2 * (y & 1) + 4 * (z & 1)
    return e, 8 * nbx * nby * nbz


def _vg_voxels(v: np.ndarray) -> np.ndarray:
    """(Z,Y,X) fp32 -> (Z,Y,X,4): the value and its three lattice differences, neighbours clamped, fp32 subtraction."""
    Z, Y, X = v.shape
    z, y, x = _coords((X, Y, Z))
    xp, yp, zp = np.minimum(x + 1, X - 1), np.minimum(y + 1, Y - 1), np.minimum(z + 1, Z - 1)
    xm, ym, zm = np.maximum(x - 1, 0), np.maximum(y - 1, 0), np.maximum(z - 1, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([v, v[z, y, xp] - v[z, y, xm], v[z, yp, x] - v[z, ym, x], v[zp, y, x] - v[zm, y, x]], axis=-1).astype(F)


def vec4_ref(lin, dims, kind: str) -> np.ndarray:
    """The whole "vg" / "quad" / "mod4" grid as (elements, 4) fp32.  ``lin``: one linear grid, or for "mod4" the four
    modalities (a missing one given as None is stored as zeros)."""
    X, Y, Z = (int(v) for v in dims)
    e, total = vec4_elem(dims)
    z, y, x = _coords(dims)
    if kind == "mod4":
        mods = [np.zeros((Z, Y, X), F) if m is None else _zyx(m, dims, F) for m in lin]
        assert len(mods) == 4
        vox = np.stack(mods, axis=-1)
    else:
        v = _zyx(lin, dims, F)
        if kind == "vg":
            vox = _vg_voxels(v)
        elif kind == "quad":
            xp, yp = np.minimum(x + 1, X - 1), np.minimum(y + 1, Y - 1)
            vox = np.stack([v, v[z, yp, x], v[z, y, xp], v[z, yp, xp]], axis=-1)
        else:
            raise ValueError(kind)
    out = np.zeros((total, 4), F)                      # every pad element: four +0.0
    out[e.reshape(-1)] = vox.reshape(-1, 4)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# VGA: the VG voxels three times, in bricks one voxel thick along x, y, z
# ----------------------------------------------------------------------------------------------------------------------
VGA_SET_LINES, VGA_ROW_PHASE, VGA_SLICE_PHASE = 64, 8, 36


def _pad_to_phase(lines: int, phase: int) -> int:
    """Pitches of 64 lines or more are moved up to the next value that is ``phase`` modulo 64."""
    if lines < VGA_SET_LINES:
        return lines
    return lines + (phase + VGA_SET_LINES - lines % VGA_SET_LINES) % VGA_SET_LINES


def vga_geometry_ref(dims) -> List[Dict]:
    """Per copy a = 0, 1, 2: bricks per axis ``nb``, ``rowLines``, ``sliceLines``, ``elems`` (float4), ``base`` (float4
    elements before this copy), and the separable address terms ``sh`` / ``mask`` / ``inner`` / ``mul``."""
    out, base = [], 0
    for a in range(3):
        nb, sh, mask, inner = [0] * 3, [0] * 3, [0] * 3, [0] * 3
        first, stride = True, 1
        for k in range(3):
            if k == a:
                nb[k] = int(dims[k])
            elif first:                                   # the first non-flat axis gets 4 voxels of the brick
                nb[k], sh[k], mask[k], inner[k] = (int(dims[k]) + 3) // 4, 2, 3, stride
                stride, first = stride * 4, False
            else:                                         # the second gets 2
                nb[k], sh[k], mask[k], inner[k] = (int(dims[k]) + 1) // 2, 1, 1, stride
                stride *= 2
        row = _pad_to_phase(nb[0], VGA_ROW_PHASE)
        sl = _pad_to_phase(row * nb[1], VGA_SLICE_PHASE)
        elems = sl * nb[2] * 8
        out.append(dict(nb=nb, rowLines=row, sliceLines=sl, elems=elems, base=base, sh=sh, mask=mask, inner=inner,
                        mul=[8, row * 8, sl * 8]))
        base += elems
    return out


def vga_elem(dims, a: int) -> np.ndarray:
    """Element index (inside copy a) of every voxel, as a [Z][Y][X] array."""
    g = vga_geometry_ref(dims)[a]
    z, y, x = _coords(dims)
    e = 0
    for k, i in enumerate((x, y, z)):
        e = e + (i >> g["sh"][k]) * g["mul"][k] + (i & g["mask"][k]) * g["inner"][k]
    return e


def vga_ref(lin, dims) -> np.ndarray:
    """The whole "vga" grid (three copies, cumulative bases, pads zero) as (elements, 4) fp32."""
    geo = vga_geometry_ref(dims)
    vox = _vg_voxels(_zyx(lin, dims, F)).reshape(-1, 4)
    out = np.zeros((geo[2]["base"] + geo[2]["elems"], 4), F)
    for a in range(3):
        out[geo[a]["base"] + vga_elem(dims, a).reshape(-1)] = vox
    return out


# ----------------------------------------------------------------------------------------------------------------------
# CELL8: per voxel the eight bytes of its trilinear cell
# ----------------------------------------------------------------------------------------------------------------------
def cell8_ref(u8, dims) -> np.ndarray:
    """(voxels, 8) uint8 in memory order: the K2 march unpacks c000, c100, c010, c110 from the low word (lowest byte first)
    and c001, c101, c011, c111 from the high word; p1 = min(p0 + 1, d - 1)."""
    X, Y, Z = (int(v) for v in dims)
    v = _zyx(u8, dims).astype(np.uint8)
    z, y, x = _coords(dims)
    xp, yp, zp = np.minimum(x + 1, X - 1), np.minimum(y + 1, Y - 1), np.minimum(z + 1, Z - 1)
    c = [v[zz, yy, xx] for zz in (z, zp) for yy in (y, yp) for xx in (x, xp)]       # x fastest, then y, then z
    return np.stack(c, axis=-1).reshape(-1, 8)


# ----------------------------------------------------------------------------------------------------------------------
# macro cells: cell m of an axis covers voxels [8m, min(8m + 8, D - 1)] inclusive
# ----------------------------------------------------------------------------------------------------------------------
def macro_dims(dims) -> Tuple[int, int, int]:
    return tuple((int(v) + 7) // 8 for v in dims)


def axis_cells(coord: int, D: int) -> List[int]:
    """The macro cells of one axis whose inclusive voxel range holds ``coord``."""
    return [m for m in range((D + 7) // 8) if 8 * m <= coord <= min(8 * m + 8, D - 1)]


def _cell_reduce(a: np.ndarray, op, neutral) -> np.ndarray:
    """op-reduce a [Z][Y][X] array over the inclusive range of every macro cell; cells x fastest.  The ranges are boxes, so
    one axis at a time: the eight voxels [8m, 8m + 7], then the overlap plane 8m + 8 (padded with ``neutral`` past D - 1)."""
    for axis in range(3):
        D = a.shape[axis]
        m = (D + 7) // 8
        pad = [(0, 0)] * 3
        pad[axis] = (0, 8 * m + 1 - D)
        p = np.moveaxis(np.pad(a, pad, constant_values=neutral), axis, -1)
        body = op.reduce(p[..., :8 * m].reshape(p.shape[:-1] + (m, 8)), axis=-1)
        a = np.moveaxis(op(body, p[..., 8::8][..., :m]), -1, axis)
    return a.reshape(-1)


HALF_FLT_MAX = F(0.5) * np.finfo(F).max


def macro_max_ref(lin, dims) -> np.ndarray:
    """fp32 upper bound of the trilinear fetch per macro cell: ub = fl(vmax + fl(2e-6f * max|v|)); +inf when the cell
    holds a NaN, or when its value range fl(vmax - vmin) is not below FLT_MAX / 2: from FLT_MAX on, lerp's b - a overflows
    and the fetch itself can be +inf between two finite voxels, and the factor two is the headroom for the ulps by which
    the inner lerps may leave [vmin, vmax] before the outer ones subtract them."""
    v = _zyx(lin, dims, F)
    nan = np.isnan(v)
    v0 = np.where(nan, F(0), v)
    with np.errstate(invalid="ignore", over="ignore"):
        vmax, vmin = _cell_reduce(v0, np.maximum, F(-np.inf)), _cell_reduce(v0, np.minimum, F(np.inf))
        amax = _cell_reduce(np.abs(v0), np.maximum, F(0))
        wide = ~((vmax - vmin) < HALF_FLT_MAX)
        ub = vmax + F(2e-6) * amax
    assert ub.dtype == F
    return np.where(_cell_reduce(nan, np.logical_or, False) | wide, F(np.inf), ub).astype(F)


def macro_labels_ref(lab, dims) -> np.ndarray:
    """The OR of the labels of every macro cell, uint32."""
    return _cell_reduce(_zyx(lab, dims).astype(np.uint32), np.bitwise_or, np.uint32(0))


def cell_any(flags, dims) -> np.ndarray:
    """Per macro cell: is any voxel of its inclusive range flagged?  ``flags``: boolean [Z][Y][X]."""
    return _cell_reduce(_zyx(flags, dims).astype(bool), np.logical_or, False)


# ----------------------------------------------------------------------------------------------------------------------
# the per-launch "contributes nothing" mask
# ----------------------------------------------------------------------------------------------------------------------
def window_floor(wl, ww) -> np.float32:
    """tf_lo = fl(wl - fl(ww * 0.5))."""
    return F(F(wl) - F(F(ww) * F(0.5)))


def weight_sum(enabled: Sequence[int], weights: Sequence[float]) -> np.float32:
    """wSum: the enabled modalities' weights, added in slot order in fp32."""
    s = F(0.0)
    for m in range(4):
        if enabled[m]:
            s = F(s + F(weights[m]))
    return s


def skip_value_ref(ubs: Sequence[np.ndarray], weights: Sequence[float], wsum) -> np.ndarray:
    """The mask kernel's per-cell value in STRICT arithmetic: v = 0, v = fl(fl(ub * w) + v) per enabled channel in channel
    order, then v = fl(v / wsum) when wsum > 0."""
    v = np.zeros(np.asarray(ubs[0]).shape, F)
    with np.errstate(invalid="ignore", over="ignore"):
        for ub, w in zip(ubs, weights):
            v = (np.asarray(ub, F) * F(w)).astype(F) + v
        if F(wsum) > 0:
            v = (v / F(wsum)).astype(F)
    return v


def skip_mask_ref(ubs, weights, wsum, tf_lo, seg_any: Optional[np.ndarray], pred_any: Optional[np.ndarray]) -> np.ndarray:
    """True = the cell contributes nothing: v <= tf_lo (a NaN is never empty) and no shown label summary is non-zero.
    ``ubs`` / ``weights``: the enabled channels only; ``seg_any`` / ``pred_any``: None when that overlay is not shown."""
    with np.errstate(invalid="ignore"):
        empty = skip_value_ref(ubs, weights, wsum) <= F(tf_lo)
    for any_ in (seg_any, pred_any):
        if any_ is not None:
            empty &= np.asarray(any_) == 0
    return empty


def needed_ref(vols: Sequence[np.ndarray], weights: Sequence[float], dims, tf_lo,
               seg: Optional[np.ndarray] = None, pred: Optional[np.ndarray] = None) -> np.ndarray:
    """fp64 brute force that never forms a bound: a cell is needed when some voxel of its inclusive range has a weighted
    value sum(w v) / wsum above the window floor (a value that does not compare, i.e. NaN, counts as above), or when a
    shown label grid (``seg`` / ``pred`` not None) holds a non-zero label there.  ``vols`` / ``weights``: enabled channels."""
    acc = np.zeros(_zyx(vols[0], dims).shape, np.float64)
    wsum = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for v, w in zip(vols, weights):
            acc = acc + np.float64(F(w)) * _zyx(v, dims).astype(np.float64)
            wsum += float(F(w))
        if wsum > 0:
            acc = acc / wsum
        hot = ~(acc <= np.float64(F(tf_lo)))
    for lab in (seg, pred):
        if lab is not None:
            hot |= _zyx(lab, dims) != 0
    return cell_any(hot, dims)


def unpack_mask(words: np.ndarray, cells: int) -> np.ndarray:
    """The first ``cells`` bits of the skip scratch (whole 64-lane ballots, little endian) as booleans: True = empty."""
    w = np.ascontiguousarray(words).view(np.uint32)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:cells].astype(bool)
