"""Connected components of label volumes on the GPU (csrc/components.hip): the numbering of
``scipy.ndimage.label`` for a class set of a prediction that is already on the device, the components' sizes, the removal of
small components, and the per-slice counts of the notebooks' slice-consistency score."""
from __future__ import annotations

import ctypes as C

from . import _lib
from .mesh import class_mask

ALL_TUMOUR = tuple(range(1, 32))          # classes=None: every label 1..31, i.e. labels > 0 among the labels a mask can name


def _mask(classes) -> int:
    return class_mask(ALL_TUMOUR if classes is None else classes)


def _connectivity(connectivity) -> int:
    c = int(connectivity)
    if c not in (1, 2, 3):
        raise ValueError(f"connectivity: expected 1, 2 or 3 (6, 18 or 26 neighbours), got {connectivity!r}")
    return c


def _device_of(x):
    import torch
    from .render import _require_gpu
    return x.device if isinstance(x, torch.Tensor) and x.is_cuda else _require_gpu()


def _hwd(t):
    return (C.c_uint32 * 3)(*t.shape)


def _label(lab, mask: int, connectivity: int, stream):
    """(components int32 device tensor, N) of the int16 device volume ``lab``; the one host read is N."""
    import torch
    from .render import _ptr, _stream_ptr
    lib = _lib.lib()
    hwd = _hwd(lab)
    nbytes = int(lib.mrirt_cc_scratch_bytes(hwd))
    if nbytes <= 0:
        raise ValueError(f"label_components: a volume of shape {tuple(lab.shape)} is outside the supported sizes")
    comp = torch.empty(tuple(lab.shape), dtype=torch.int32, device=lab.device)
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=lab.device)
    count = torch.empty(1, dtype=torch.int64, device=lab.device)
    _lib.check(lib.mrirt_cc_label(_ptr(lab), hwd, mask, connectivity, _ptr(comp), _ptr(count), _ptr(scratch), nbytes,
                                  _stream_ptr(stream)), "mrirt_cc_label")
    return comp, int(count.cpu()[0])


def _sizes(comp, n: int, stream):
    import torch
    from .render import _ptr, _stream_ptr
    sizes = torch.empty(n, dtype=torch.int32, device=comp.device)
    _lib.check(_lib.lib().mrirt_cc_sizes(_ptr(comp), _hwd(comp), n, _ptr(sizes) if n else None, _stream_ptr(stream)), "mrirt_cc_sizes")
    return sizes


def count_components_host(mask, connectivity=1) -> int:
    """The number of connected components of a boolean NumPy volume, on the host (what :func:`mrirt.inr.compute_multi_metrics`
    uses for NumPy inputs, which must not need a GPU): a union-find over the adjacent pairs in which the larger of two roots
    is linked to the smallest root proposed for it until every pair shares a root."""
    import itertools
    import numpy as np
    conn = _connectivity(connectivity)
    m = np.asarray(mask, dtype=bool)
    if m.ndim != 3:
        raise ValueError(f"count_components_host: expected an (H, W, D) volume, got shape {m.shape}")
    idx = np.arange(m.size, dtype=np.int64).reshape(m.shape)
    a, b = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for d in itertools.product((-1, 0, 1), repeat=3):
        if d <= (0, 0, 0) or sum(1 for x in d if x) > conn:
            continue
        lo = tuple(slice(max(0, -x), m.shape[k] - max(0, x)) for k, x in enumerate(d))
        hi = tuple(slice(max(0, x), m.shape[k] - max(0, -x)) for k, x in enumerate(d))
        both = m[lo] & m[hi]
        a.append(idx[lo][both])
        b.append(idx[hi][both])
    a, b = np.concatenate(a), np.concatenate(b)
    parent = np.arange(m.size, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        differ = ra != rb
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return int(np.count_nonzero(m.reshape(-1) & (parent == np.arange(m.size))))


def label_components(labels, classes=None, connectivity=1, stream=None):
    """The connected components of the voxels whose label is in ``classes`` (``None``: every label 1..31; otherwise what
    :func:`mrirt.mesh.class_mask` accepts) under 6, 18 or 26 neighbours (``connectivity`` 1, 2 or 3, the structures of
    ``scipy.ndimage.generate_binary_structure(3, connectivity)``).  ``labels``: an (H, W, D) integer volume, a NumPy array or a
    device tensor (what ``predict_volume`` returns).  Returns ``(components, n)``: an int32 device tensor with the numbers
    1..n on the class set and 0 elsewhere, numbered as ``scipy.ndimage.label`` numbers them (by first voxel in C order), and
    the Python int n — the call's one host read."""
    import torch
    from .inr import _label_volume
    from .render import _on_stream
    mask, conn = _mask(classes), _connectivity(connectivity)
    dev = _device_of(labels)
    with torch.cuda.device(dev), _on_stream(stream):
        return _label(_label_volume(labels, dev, "labels"), mask, conn, stream)


def component_sizes(components, n):
    """int32 device tensor of ``n`` sizes: element k - 1 is the number of voxels numbered k in ``components`` (the int32 device
    tensor of :func:`label_components`)."""
    import torch
    n = int(n)
    if n < 0:
        raise ValueError("component_sizes: n must not be negative")
    if not (isinstance(components, torch.Tensor) and components.is_cuda and components.dtype == torch.int32 and components.dim() == 3):
        raise TypeError("component_sizes: expected the int32 (H, W, D) device tensor label_components returns")
    with torch.cuda.device(components.device):
        return _sizes(components.contiguous(), n, None)


def remove_small_components(labels, classes=None, min_voxels=0, connectivity=1, keep_largest=False, fill=0):
    """``labels`` as an int16 device tensor in which every component of the class set (see :func:`label_components`) with fewer
    than ``min_voxels`` voxels — and, with ``keep_largest``, every component but the largest (of equal sizes the first in C
    order) — is overwritten with ``fill``.  Voxels outside the class set keep their label."""
    import torch
    from .inr import _label_volume
    from .render import _ptr, _stream_ptr
    mask, conn = _mask(classes), _connectivity(connectivity)
    if int(min_voxels) < 0:
        raise ValueError("remove_small_components: min_voxels must not be negative")
    if not -32768 <= int(fill) <= 32767:
        raise ValueError("remove_small_components: fill must fit int16")
    dev = _device_of(labels)
    with torch.cuda.device(dev):
        lab = _label_volume(labels, dev, "labels")
        comp, n = _label(lab, mask, conn, None)
        sizes = _sizes(comp, n, None)
        out = torch.empty_like(lab)
        _lib.check(_lib.lib().mrirt_cc_filter(_ptr(lab), _ptr(comp), _ptr(sizes) if n else None, n, _hwd(lab), int(min_voxels),
                                              1 if keep_largest else 0, int(fill), _ptr(out), _stream_ptr(None)), "mrirt_cc_filter")
    return out


def slice_counts(labels):
    """int64 (D, 3) device tensor: per index z of the last axis A = #(p_z > 0), I = #((p_z == p_{z-1}) & (p_z > 0)) and
    U = #((p_z > 0) | (p_{z-1} > 0)), with I = U = 0 at z = 0 — the integers of the notebooks' slice-to-slice consistency."""
    import torch
    from .inr import _label_volume
    from .render import _ptr, _stream_ptr
    dev = _device_of(labels)
    with torch.cuda.device(dev):
        lab = _label_volume(labels, dev, "labels")
        out = torch.empty((lab.shape[2], 3), dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().mrirt_slice_counts(_ptr(lab), _hwd(lab), _ptr(out), _stream_ptr(None)), "mrirt_slice_counts")
    return out
