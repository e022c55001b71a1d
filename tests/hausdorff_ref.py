"""NumPy restatement of the exact squared Euclidean distance transform and the Hausdorff distance built on it
("Hausdorff distance"): three 1-D passes, axis 0 then 1 then 2, each g'[i] = min_j (g[j] + d(i, j)^2) in fp64
with d(i, j) = c(i) - c(j) and c(i) = double(float32(i) * float32(spacing)).  No fused operations anywhere: NumPy
evaluates the subtraction, the square, the addition and the minimum as separate fp64 operations."""
import numpy as np


def coords(n: int, s) -> np.ndarray:
    return (np.arange(n, dtype=np.float32) * np.float32(s)).astype(np.float64)


def line_pass(g: np.ndarray, axis: int, s) -> np.ndarray:
    g = np.moveaxis(g, axis, 0)
    c = coords(g.shape[0], s)
    out = np.empty_like(g)
    for i in range(g.shape[0]):
        d = c[i] - c
        d2 = d * d
        out[i] = (g + d2.reshape((-1,) + (1,) * (g.ndim - 1))).min(axis=0)
    return np.moveaxis(out, 0, axis)


def edt_squared(mask: np.ndarray, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
    """F_M: fp64 squared distance to the nearest voxel of ``mask`` (+inf everywhere when it is empty)."""
    g = np.where(mask, 0.0, np.inf)
    for axis in range(3):
        g = line_pass(g, axis, spacing[axis])
    return np.ascontiguousarray(g)


def directed_sq(pred: np.ndarray, true: np.ndarray, cls: int, spacing=(1.0, 1.0, 1.0)):
    """(a_c, b_c) = (max over P of F_T, max over T of F_P); NaN when either mask is empty."""
    P, T = pred == cls, true == cls
    if not P.any() or not T.any():
        return float("nan"), float("nan")
    return float(edt_squared(T, spacing)[P].max()), float(edt_squared(P, spacing)[T].max())


def hausdorff(pred: np.ndarray, true: np.ndarray, spacing=(1.0, 1.0, 1.0), num_classes: int = 4) -> dict:
    out = {}
    for c in range(num_classes):
        a, b = directed_sq(pred, true, c, spacing)
        out[c] = float(np.sqrt(np.float64(max(a, b)))) if a == a else float("nan")
    return out
