"""Label volumes for the Hausdorff / distance-transform tests, and the reader of tests/golden/inr_hausdorff.npz.

``blob_labels`` builds a BraTS-like label volume (nested ellipsoids: class 1 around class 2 around class 3 in a background
of 0, every boundary roughened by a hash) from integer arithmetic only — integer ellipsoid inequalities and a 32-bit
integer hash — so every platform builds the same bytes and the fixture stores the large case as parameters, a CRC per
volume and the expected values, not as volumes."""
import pathlib
import zlib

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "inr_hausdorff.npz"
M32 = np.uint64(0xFFFFFFFF)


def _hash(x, y, z, seed: int):
    """32-bit integer mix of the voxel index and a seed, computed in uint64 and masked (wrap-around is defined)."""
    h = (x * np.uint64(73856093)) ^ (y * np.uint64(19349663)) ^ (z * np.uint64(83492791)) ^ np.uint64((seed * 2654435761) & 0xFFFFFFFF)
    h &= M32
    for mul, sh in ((0x85EBCA6B, 13), (0xC2B2AE35, 16)):
        h ^= h >> np.uint64(15)
        h = (h * np.uint64(mul)) & M32
        h ^= h >> np.uint64(sh)
    return h


def blob_labels(shape, seed: int, shift=(0, 0, 0), grow: int = 0) -> np.ndarray:
    """int16 (H, W, D): label = how many of three nested noisy ellipsoids hold the voxel.  ``shift`` moves the centre (in
    voxels) and ``grow`` widens every radius (in 64ths of the axis), which is how a "prediction" differs from its "truth"."""
    H, W, D = (int(v) for v in shape)
    x = np.arange(H, dtype=np.int64)[:, None, None]
    y = np.arange(W, dtype=np.int64)[None, :, None]
    z = np.arange(D, dtype=np.int64)[None, None, :]
    noise = _hash(x.astype(np.uint64), y.astype(np.uint64), z.astype(np.uint64), seed)
    lab = np.zeros((H, W, D), dtype=np.int16)
    cx, cy, cz = H // 2 + shift[0], W // 2 + shift[1], D // 2 + shift[2]
    for k, num in enumerate((24, 16, 9)):                 # radii in 64ths of each axis: outer, middle, core
        rx, ry, rz = (max(1, (n * (num + grow)) // 64) for n in (H, W, D))
        # centre of ellipsoid k drifts a little so the shells are not concentric
        dx, dy, dz = x - (cx + k * rx // 5), y - (cy - k * ry // 6), z - (cz + k * rz // 7)
        lhs = dx * dx * (ry * ry * rz * rz) + dy * dy * (rx * rx * rz * rz) + dz * dz * (rx * rx * ry * ry)
        rhs = rx * rx * ry * ry * rz * rz
        jitter = ((noise >> np.uint64(8 * k)) & np.uint64(63)).astype(np.int64)          # 0..63
        lab += (lhs * 256 <= rhs * (224 + jitter)).astype(np.int16)
    return lab


def crc(vol: np.ndarray) -> int:
    return zlib.crc32(np.ascontiguousarray(vol, dtype=np.int16).tobytes()) & 0xFFFFFFFF


def large_pair(shape):
    """The large synthetic prediction / truth pair of the fixture (and of tools/hausdorff_timing.py)."""
    return blob_labels(shape, 11, shift=(3, -2, 1), grow=1), blob_labels(shape, 5)


def load_cases():
    """[(name, pred, true, spacing (3 floats), num_classes, expected float64 [num_classes])] for the stored cases."""
    out = []
    with np.load(GOLDEN) as z:
        for name in [str(n) for n in z["names"]]:
            out.append((name, z[f"{name}_pred"], z[f"{name}_true"], tuple(float(s) for s in z[f"{name}_spacing"]),
                        int(z[f"{name}_nc"]), z[f"{name}_hd"]))
    return out


def load_large():
    """(shape, spacing, num_classes, crc_pred, crc_true, expected) of the large case."""
    with np.load(GOLDEN) as z:
        return (tuple(int(v) for v in z["large_shape"]), tuple(float(s) for s in z["large_spacing"]), int(z["large_nc"]),
                int(z["large_crc_pred"]), int(z["large_crc_true"]), z["large_hd"])


def same(a, b) -> bool:
    """== with NaN matching NaN (the contract is bit-identical values)."""
    a, b = float(a), float(b)
    return (a == b) or (a != a and b != b)
