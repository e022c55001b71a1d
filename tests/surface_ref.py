"""Naive surface nets of a label volume — a vectorised NumPy restatement of the definition in DESIGN.md section 12, the
contract of csrc/surface.hip (mrirt_surface_count / mrirt_surface_extract): the GPU output equals this element for element.
Also the checks every output must pass: closedness, signed volume, Euler characteristic."""
import numpy as np

CYCLIC = ((0, 1, 2), (1, 2, 0), (2, 0, 1))


def class_mask(classes) -> int:
    m = 0
    for c in ([classes] if np.isscalar(classes) else classes):
        assert 0 <= int(c) < 32
        m |= 1 << int(c)
    return m


def inside(labels: np.ndarray, mask: int) -> np.ndarray:
    lab = np.asarray(labels).astype(np.int64)
    ok = (lab >= 0) & (lab < 32)
    return ok & (((int(mask) >> np.where(ok, lab, 0)) & 1) == 1)


def extract(labels: np.ndarray, mask: int, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """(verts float32 [V, 3], tris int32 [T, 3]) of the class set ``mask`` (bit l = label l is inside)."""
    n = labels.shape
    N = tuple(k + 1 for k in n)                                      # cells per axis
    pad = np.zeros(tuple(k + 2 for k in n), dtype=bool)              # voxel v lives at pad[v + 1]; outside the volume is outside
    pad[1:-1, 1:-1, 1:-1] = inside(labels, mask)

    def corner(b):                                                   # voxel c - 1 + b of every cell c
        return pad[b[0]:b[0] + N[0], b[1]:b[1] + N[1], b[2]:b[2] + N[2]]

    B = [(b0, b1, b2) for b0 in (0, 1) for b1 in (0, 1) for b2 in (0, 1)]
    count = sum(corner(b).astype(np.int32) for b in B)
    active = (count > 0) & (count < 8)
    S = np.zeros((3,) + N, dtype=np.int32)
    m = np.zeros(N, dtype=np.int32)
    for a in range(3):
        for b in B:
            if b[a]:
                continue
            e = tuple(b[k] + (k == a) for k in range(3))
            d = (corner(b) != corner(e)).astype(np.int32)
            m += d
            for k in range(3):
                S[k] += d * (2 * b[k] + (k == a))
    cells = np.argwhere(active)                                      # C order: increasing linear cell index
    V = len(cells)
    vid = np.full(N, -1, dtype=np.int64)
    vid[active] = np.arange(V)
    sp, org = np.asarray(spacing, dtype=np.float32), np.asarray(origin, dtype=np.float32)
    verts = np.zeros((V, 3), dtype=np.float32)
    two_m = (2 * m[active]).astype(np.float32)
    for k in range(3):
        q = S[k][active].astype(np.float32) / two_m
        verts[:, k] = ((cells[:, k] - 1).astype(np.float32) + q) * sp[k] + org[k]

    c000 = corner((0, 0, 0))
    idx = np.indices(N)
    emit = np.zeros(N + (3,), dtype=bool)
    for a, b, c in CYCLIC:
        e = tuple(int(k == a) for k in range(3))
        emit[..., a] = (c000 != corner(e)) & (idx[b] >= 1) & (idx[c] >= 1)
    quads = np.argwhere(emit)                                        # by owning cell, then by a
    tris = np.zeros((2 * len(quads), 3), dtype=np.int32)
    if len(quads):
        cc, a = quads[:, :3], quads[:, 3]
        b, c = (a + 1) % 3, (a + 2) % 3
        eb, ec = np.eye(3, dtype=np.int64)[b], np.eye(3, dtype=np.int64)[c]

        def Q(ib, ic):
            p = cc - (1 - ib) * eb - (1 - ic) * ec
            return vid[p[:, 0], p[:, 1], p[:, 2]]

        q00, q10, q01, q11 = Q(0, 0), Q(1, 0), Q(0, 1), Q(1, 1)
        assert min(q00.min(), q10.min(), q01.min(), q11.min()) >= 0
        ins = c000[cc[:, 0], cc[:, 1], cc[:, 2]]
        tris[0::2] = np.where(ins[:, None], np.stack([q00, q10, q11], 1), np.stack([q00, q11, q10], 1))
        tris[1::2] = np.where(ins[:, None], np.stack([q00, q11, q01], 1), np.stack([q00, q01, q11], 1))
    return verts, tris


def num_cells(shape) -> int:
    return int((shape[0] + 1) * (shape[1] + 1) * (shape[2] + 1))


def is_closed(tris: np.ndarray) -> bool:
    """Every directed edge u->v is used as often as v->u."""
    t = np.asarray(tris, dtype=np.int64)
    if len(t) == 0:
        return True
    u = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    v = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    big = int(max(u.max(), v.max())) + 1
    fwd, fn = np.unique(u * big + v, return_counts=True)
    bwd, bn = np.unique(v * big + u, return_counts=True)
    return np.array_equal(fwd, bwd) and np.array_equal(fn, bn)


def signed_volume(verts: np.ndarray, tris: np.ndarray) -> float:
    p = np.asarray(verts, dtype=np.float64)[np.asarray(tris, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def euler(verts: np.ndarray, tris: np.ndarray) -> int:
    t = np.sort(np.asarray(tris, dtype=np.int64), axis=1)
    e = np.unique(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [0, 2]]]), axis=0)
    return len(verts) - len(e) + len(t)
