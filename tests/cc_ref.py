"""NumPy restatement of DESIGN.md section 21 (connected components of label volumes): the inside rule, the adjacency of the
three connectivities, a plain union-find whose links only decrease, the numbering by smallest linear index, the sizes, the
small-component filter and the slice counts.  What the GPU writes is compared with this element for element; this is compared
with scipy.ndimage.label (tests/test_cc_host.py, tests/golden/cc_scipy.npz)."""
import itertools

import numpy as np


def inside(labels, class_mask: int) -> np.ndarray:
    lab = np.asarray(labels).astype(np.int64)
    ok = (lab >= 0) & (lab < 32)
    return ok & (((int(class_mask) >> np.where(ok, lab, 0)) & 1) != 0)


def forward_offsets(connectivity: int):
    """The offsets whose neighbour has the larger linear index: 3, 9 or 13 of the 6, 18 or 26 neighbours."""
    if connectivity not in (1, 2, 3):
        raise ValueError("connectivity must be 1, 2 or 3")
    return [d for d in itertools.product((-1, 0, 1), repeat=3)
            if d > (0, 0, 0) and sum(1 for x in d if x) <= connectivity]


def adjacent_pairs(mask: np.ndarray, connectivity: int):
    """Linear indices (a, b), a < b, of every adjacent pair of inside voxels, each pair once."""
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    A, B = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for d in forward_offsets(connectivity):
        lo = tuple(slice(max(0, -x), mask.shape[k] - max(0, x)) for k, x in enumerate(d))
        hi = tuple(slice(max(0, x), mask.shape[k] - max(0, -x)) for k, x in enumerate(d))
        both = mask[lo] & mask[hi]
        A.append(idx[lo][both])
        B.append(idx[hi][both])
    return np.concatenate(A), np.concatenate(B)


def label(labels, class_mask: int, connectivity: int = 1):
    """(components int32 like labels, N): union-find over the adjacent pairs.  Every round links the larger of two roots to
    the smallest root proposed for it, then points every voxel at its root; it ends when every pair shares a root."""
    mask = inside(labels, class_mask)
    A, B = adjacent_pairs(mask, connectivity)
    parent = np.arange(mask.size, dtype=np.int64)
    while True:
        ra, rb = parent[A], parent[B]
        differ = ra != rb
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    flat = mask.reshape(-1)
    roots = np.flatnonzero(flat & (parent == np.arange(mask.size)))
    number = np.zeros(mask.size, dtype=np.int32)
    number[roots] = np.arange(1, len(roots) + 1, dtype=np.int32)
    return np.where(flat, number[parent], 0).astype(np.int32).reshape(mask.shape), int(len(roots))


def sizes(components, n: int) -> np.ndarray:
    return np.bincount(np.asarray(components).reshape(-1), minlength=n + 1)[1:n + 1].astype(np.int32)


def kept(sz: np.ndarray, min_voxels: int, keep_largest: bool) -> np.ndarray:
    k = sz >= min_voxels
    if keep_largest and len(sz):
        only = np.zeros(len(sz), dtype=bool)
        only[int(np.argmax(sz))] = True             # argmax: the first of equal sizes
        k &= only
    return k


def filter_small(labels, components, sz, min_voxels=0, keep_largest=False, fill=0) -> np.ndarray:
    labels, components = np.asarray(labels), np.asarray(components)
    keep = np.concatenate([[True], kept(np.asarray(sz), min_voxels, keep_largest)])       # number 0: not in the mask
    return np.where(keep[components], labels, np.int16(fill)).astype(np.int16)


def remove_small(labels, class_mask, min_voxels=0, connectivity=1, keep_largest=False, fill=0) -> np.ndarray:
    comp, n = label(labels, class_mask, connectivity)
    return filter_small(np.asarray(labels).astype(np.int16), comp, sizes(comp, n), min_voxels, keep_largest, fill)


def slice_counts(labels) -> np.ndarray:
    """int64 (n2, 3): A, I, U per index of the last axis, in the notebook's own expressions."""
    p = np.asarray(labels)
    out = np.zeros((p.shape[2], 3), dtype=np.int64)
    for z in range(p.shape[2]):
        pz = p[:, :, z]
        out[z, 0] = (pz > 0).sum()
        if z >= 1:
            pp = p[:, :, z - 1]
            out[z, 1] = ((pz == pp) & (pz > 0)).sum()
            out[z, 2] = ((pz > 0) | (pp > 0)).sum()
    return out


def first_occurrences_increase(components, n: int) -> bool:
    """The numbers are 1 .. n and the first raster-order voxel of k precedes that of k + 1."""
    flat = np.asarray(components).reshape(-1)
    vals, first = np.unique(flat, return_index=True)
    if vals[0] == 0:
        vals, first = vals[1:], first[1:]
    return np.array_equal(vals, np.arange(1, n + 1)) and bool(np.all(np.diff(first) > 0))
