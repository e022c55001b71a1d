"""References for the hybrid, uncertainty-guided sampler and the coordinate noise (csrc/inr_hybrid.hip):
the definition of include/mrirt.h restated with NumPy and Python integers.  No GPU.

  class_index      (index uint32, offsets int64 [C ncases + 1]): a stable sort of (label, case, offset)
  key              the order-preserving 32-bit key of the selection: -0 below +0, every NaN the one key above +inf
  select_largest   sorted(np.argsort(key, kind="stable")[-k:])
  normal3          Box-Muller in fp64 from the Philox words at counter word 3 = 2, each value rounded once to fp32
  mulhi64          floor(a b / 2^64) with Python integers
  candidates       (case, x, y, z) of the candidate stream (counter word 3 = 1)
  hybrid_rows      (case, x, y, z, kind) of every row of a hybrid micro-batch; kind 0 candidate, 1 from the class index, 2 the
                   fallback of an empty class, 3 uniform
  rows_of          coords / feats / labels of drawn voxels, as the samplers write them
  hybrid_counts    the notebook's int() truncations
"""
import numpy as np

import inr_loop_ref as lp

TWO_PI = 6.283185307179586
M64 = 2 ** 64 - 1


def class_index(cases, C):
    segs = [np.asarray(c["seg"]).reshape(-1).astype(np.int64) for c in cases]
    lab = np.concatenate(segs)
    cs = np.concatenate([np.full(len(s), i, np.int64) for i, s in enumerate(segs)])
    off = np.concatenate([np.arange(len(s), dtype=np.int64) for s in segs])
    keep = (lab >= 0) & (lab < C)
    lab, cs, off = lab[keep], cs[keep], off[keep]
    order = np.lexsort((off, cs, lab))                  # by label, then case, then offset
    counts = np.zeros((C, len(cases)), np.int64)
    np.add.at(counts, (lab, cs), 1)
    offsets = np.concatenate([[0], np.cumsum(counts.reshape(-1))]).astype(np.int64)
    return off[order].astype(np.uint32), offsets


def key(values):
    v = np.ascontiguousarray(values, np.float32)
    b = v.view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(v), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def select_largest(values, k):
    return np.sort(np.argsort(key(values), kind="stable")[-k:]).astype(np.uint32)


def words(seed, batch_index, i, stream):
    seed, b = int(seed) & M64, int(batch_index) & M64
    return lp.philox4x32_10((np.asarray(i, np.uint64), b & lp.MASK, b >> 32, stream), (seed & lp.MASK, seed >> 32))


def normal_of_words(r):
    """fp64 (n, 3) of four uint32 word arrays."""
    r = [np.asarray(v, np.uint32).astype(np.float64) for v in r]
    two_m32 = 2.0 ** -32
    R, a = np.sqrt(-2.0 * np.log((r[0] + 1.0) * two_m32)), TWO_PI * (r[1] * two_m32)
    R2, a2 = np.sqrt(-2.0 * np.log((r[2] + 1.0) * two_m32)), TWO_PI * (r[3] * two_m32)
    return np.stack([R * np.cos(a), R * np.sin(a), R2 * np.cos(a2)], -1)


def normal3(seed, batch_index, n):
    """fp64 restatement rounded once to fp32, (n, 3)."""
    return normal_of_words(words(seed, batch_index, np.arange(n), 2)).astype(np.float32)


def mulhi64(a, b):
    return (int(a) * int(b)) >> 64


def _uniform(r, ncases, hwd):
    return lp.mulhi32(r[0], ncases), lp.mulhi32(r[1], hwd[0]), lp.mulhi32(r[2], hwd[1]), lp.mulhi32(r[3], hwd[2])


def candidates(seed, batch_index, j, ncases, hwd):
    """(case, x, y, z) of the candidates ``j`` (an array of uint32 counters)."""
    return _uniform(words(seed, batch_index, np.asarray(j, np.uint64) & np.uint64(lp.MASK), 1), ncases, hwd)


def hybrid_rows(seed, batch_index, n, U, P, C, picks, index, offsets, ncases, hwd):
    r = words(seed, batch_index, np.arange(n), 0)
    cs, x, y, z = [np.array(v) for v in _uniform(r, ncases, hwd)]
    kind = np.full(n, 3, np.int64)
    if U > 0:
        pc = candidates(seed, batch_index, np.asarray(picks[:U], np.uint32), ncases, hwd)
        for dst, src in zip((cs, x, y, z), pc):
            dst[:U] = src
        kind[:U] = 0
    W, D = int(hwd[1]), int(hwd[2])
    for i in range(U, U + C * P):
        k = (i - U) // P
        first, total = int(offsets[k * ncases]), int(offsets[(k + 1) * ncases]) - int(offsets[k * ncases])
        if total == 0:
            kind[i] = 2
            continue
        slot = first + mulhi64((int(r[0][i]) << 32) | int(r[1][i]), total)
        v = int(index[slot])
        cs[i] = np.searchsorted(np.asarray(offsets[k * ncases:(k + 1) * ncases + 1]), slot, side="right") - 1
        x[i], y[i], z[i] = v // (W * D), (v // D) % W, v % D
        kind[i] = 1
    return cs, x, y, z, kind


def rows_of(cases, cs, x, y, z, fields=None):
    """coords (n, 3) fp32, feats (n, M) fp32, labels (n,) int32 (and the field's values) of the drawn voxels."""
    hwd = cases[0]["seg"].shape
    coords = np.stack([(v.astype(np.float32) / np.float32(e - 1)) * np.float32(2.0) - np.float32(1.0) for v, e in zip((x, y, z), hwd)], 1).astype(np.float32)
    mods = np.stack([np.asarray(c["mods"], np.float32) for c in cases])
    seg = np.stack([np.asarray(c["seg"]) for c in cases])
    feats = mods[cs, :, x, y, z].astype(np.float32).reshape(len(cs), mods.shape[1])
    out = [coords, feats, seg[cs, x, y, z].astype(np.int32)]
    if fields is not None:
        out.append(np.stack(fields)[cs, x, y, z].astype(np.float32))
    return out


def noisy(coords, sigma, z):
    """float32(c + float32(sigma z)): the product and the sum each rounded to fp32."""
    return (coords.astype(np.float32) + (np.float32(sigma) * z.astype(np.float32)).astype(np.float32)).astype(np.float32)


def hybrid_counts(micro, uncertainty_ratio, balanced_ratio, num_classes, use_uncertainty, max_candidates=10000):
    n_unc = int(micro * uncertainty_ratio) if use_uncertainty else 0
    return n_unc, int(micro * balanced_ratio) // num_classes, min(max_candidates, n_unc * 10)


def scratch_bytes(ncases, hwd, C):
    chunks = (int(np.prod([int(v) for v in hwd])) + 4095) // 4096
    return (ncases * chunks * C * 4 + 255) & ~255
