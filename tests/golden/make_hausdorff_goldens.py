"""Generate tests/golden/inr_hausdorff.npz.  Runs ONLY where the reference checkout is mounted (MRIRT_REFERENCE, as
make_goldens.py); the fixture (data only) is committed, the reference source never is.

The expected values are what the reference's own ``hausdorff_distance`` (inr/inr/model.py:164-195: two scipy cKDTrees per
class over the float32 coordinate grid) returns, imported through the NumPy-backed ``jax`` stub of make_goldens.py.  Small
and medium cases store their volumes (blob volumes compress to a few KB); the large case stores its shape, spacing, the CRC
of each volume and the expected values only — tests/hausdorff_cases.large_pair rebuilds the volumes from integer arithmetic.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_hausdorff_goldens.py [H W D of the large case]
"""
from __future__ import annotations

import pathlib
import sys
import time

import numpy as np

sys.dont_write_bytecode = True
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import hausdorff_cases as hc                                          # noqa: E402
from make_goldens import REF, _import_reference_model                 # noqa: E402

ANISO = ((1.0, 1.0, 2.5), (0.9375, 1.1, 1.3), (0.7, 0.7, 3.3))


def small_cases():
    rng = np.random.default_rng(606)
    cases = []
    cases.append(("unit_blob", hc.blob_labels((40, 36, 30), 1, shift=(2, -1, 1), grow=1), hc.blob_labels((40, 36, 30), 2), (1.0, 1.0, 1.0), 4))
    for k, sp in enumerate(ANISO):
        shape = ((36, 40, 22), (31, 29, 37), (40, 40, 12))[k]
        cases.append((f"aniso{k}_blob", hc.blob_labels(shape, 10 + k, shift=(-1, 2, 0)), hc.blob_labels(shape, 20 + k, grow=2), sp, 4))
    a, b = (rng.integers(0, 4, (18, 16, 14)).astype(np.int16) for _ in range(2))
    cases.append(("unit_random", a, b, (1.0, 1.0, 1.0), 4))
    a, b = (np.where(rng.random((15, 17, 9)) < 0.9, 0, rng.integers(1, 5, (15, 17, 9))).astype(np.int16) for _ in range(2))
    cases.append(("aniso2_sparse_random", a, b, ANISO[2], 5))
    p, t = hc.blob_labels((30, 28, 26), 3, shift=(1, 1, -1)), hc.blob_labels((30, 28, 26), 4)
    p = np.where(p == 3, 2, p).astype(np.int16)
    cases.append(("absent_in_pred_only", p, t, ANISO[0], 4))
    t = hc.blob_labels((26, 30, 24), 6)
    cases.append(("identical", t.copy(), t, ANISO[1], 5))              # 0.0 for classes 0..3, NaN for class 4 (in neither)
    p, t = hc.blob_labels((28, 26, 30), 7, grow=1), hc.blob_labels((28, 26, 30), 8)
    t = np.where(t == 3, 2, t).astype(np.int16)
    t[20, 5, 17] = 3
    cases.append(("one_voxel_class", p, t, (1.0, 1.0, 1.0), 4))
    cases.append(("thin_axis1", hc.blob_labels((24, 1, 20), 9, shift=(1, 0, 1)), hc.blob_labels((24, 1, 20), 12), ANISO[0], 4))
    a, b = (rng.integers(0, 3, (1, 1, 17)).astype(np.int16) for _ in range(2))
    cases.append(("single_line", a, b, ANISO[2], 3))
    a, b = (rng.integers(-1, 7, (16, 12, 14)).astype(np.int16) for _ in range(2))
    cases.append(("labels_outside_classes", a, b, ANISO[1], 4))
    cases.append(("medium_blob", hc.blob_labels((96, 96, 62), 13, shift=(2, -1, 1), grow=1), hc.blob_labels((96, 96, 62), 14), ANISO[0], 4))
    return cases


def main():
    if not REF.exists():
        raise SystemExit(f"{REF} not found: goldens are generated where the reference is mounted only")
    model = _import_reference_model()
    out = {}
    names = []
    for name, pred, true, sp, nc in small_cases():
        assert max(pred.shape) <= 40 or name == "medium_blob"
        t0 = time.time()
        hd = model.hausdorff_distance(pred, true, spacing=sp, num_classes=nc)
        vals = np.array([float(hd[c]) for c in range(nc)], dtype=np.float64)
        print(f"{name:26s} {pred.shape} spacing {sp} nc {nc}: {vals}  ({time.time() - t0:.2f} s)")
        names.append(name)
        out[f"{name}_pred"], out[f"{name}_true"] = pred, true
        out[f"{name}_spacing"], out[f"{name}_nc"], out[f"{name}_hd"] = np.array(sp, dtype=np.float64), np.int64(nc), vals
    out["names"] = np.array(names)
    shape = tuple(int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (240, 240, 155)
    pred, true = hc.large_pair(shape)
    t0 = time.time()
    hd = model.hausdorff_distance(pred, true, num_classes=4)
    vals = np.array([float(hd[c]) for c in range(4)], dtype=np.float64)
    print(f"large {shape}: {vals}  (reference: {time.time() - t0:.1f} s)  counts pred {np.bincount(pred.ravel())} true {np.bincount(true.ravel())}")
    out["large_shape"], out["large_spacing"], out["large_nc"] = np.array(shape, dtype=np.int64), np.ones(3), np.int64(4)
    out["large_crc_pred"], out["large_crc_true"], out["large_hd"] = np.int64(hc.crc(pred)), np.int64(hc.crc(true)), vals
    out["large_reference_seconds"] = np.float64(time.time() - t0)
    np.savez_compressed(HERE / "inr_hausdorff.npz", **out)
    print("wrote", HERE / "inr_hausdorff.npz", (HERE / "inr_hausdorff.npz").stat().st_size, "B")


if __name__ == "__main__":
    main()
