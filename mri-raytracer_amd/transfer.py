"""RGBA transfer-function tables for the K1 march (``render_brats(..., tf=...)``, ``mrirt_render_brats_tf``).

A table is an ``(N, 4)`` float32 array of rows ``(r, g, b, sigma)``, 2 <= N <= 1024.  The march maps a sample's windowed,
gamma-corrected intensity ``val`` in [0, 1] to ``u = val * (N - 1)`` and blends rows ``floor(u)`` and ``floor(u) + 1`` linearly
(DESIGN.md section 22): row ``i`` is the table's value at ``val = i / (N - 1)``.  ``sigma`` is the extinction the sample's opacity
is made of, ``alpha = 1 - exp(-sigma * intensityAlpha * stepSize)``; a sample with ``sigma <= 0`` draws nothing.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

TF_MIN_ENTRIES, TF_MAX_ENTRIES = 2, 1024


def _check_n(n: int) -> int:
    n = int(n)
    if not TF_MIN_ENTRIES <= n <= TF_MAX_ENTRIES:
        raise ValueError(f"a transfer-function table has {TF_MIN_ENTRIES}..{TF_MAX_ENTRIES} entries, got {n}")
    return n


def tf_ramp(n: int = 2) -> np.ndarray:
    """The grey ramp ``r = g = b = sigma = x``: today's window / level / gamma frame.  With ``n == 2`` — rows (0,0,0,0) and
    (1,1,1,1) — the table render is bit-identical to the plain one in STRICT math."""
    n = _check_n(n)
    x = (np.arange(n, dtype=np.float64) / (n - 1)).astype(np.float32)
    return np.repeat(x[:, None], 4, axis=1)


def tf_from_points(points: Sequence[Sequence[float]], n: int = 256) -> np.ndarray:
    """Control points ``(x, r, g, b, sigma)`` with x ascending in [0, 1] -> an ``(n, 4)`` table: the piecewise-linear curve through
    the points evaluated in float64 at ``i / (n - 1)``, the first / last point's values held outside their x, rounded once to
    float32."""
    n = _check_n(n)
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 5 or pts.shape[0] < 1:
        raise ValueError("control points are rows of (x, r, g, b, sigma)")
    x = pts[:, 0]
    if not np.all(np.isfinite(pts)) or x[0] < 0.0 or x[-1] > 1.0 or np.any(np.diff(x) < 0.0):
        raise ValueError("control points must be finite with x ascending in [0, 1]")
    at = np.arange(n, dtype=np.float64) / (n - 1)
    return np.stack([np.interp(at, x, pts[:, k]) for k in range(1, 5)], axis=1).astype(np.float32)


# name -> control points; every preset is defined through tf_from_points
PRESETS = {
    "gray": [(0.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0, 1.0)],
    # black -> red -> yellow -> white, sigma = x
    "hot": [(0.0, 0.0, 0.0, 0.0, 0.0), (1.0 / 3.0, 1.0, 0.0, 0.0, 1.0 / 3.0), (2.0 / 3.0, 1.0, 1.0, 0.0, 2.0 / 3.0), (1.0, 1.0, 1.0, 1.0, 1.0)],
}


def tf_preset(name: str, n: int = 256) -> np.ndarray:
    """``"gray"`` (the ramp) or ``"hot"`` (black -> red -> yellow -> white, sigma = x) as an ``(n, 4)`` table."""
    if name not in PRESETS:
        raise ValueError(f"unknown transfer-function preset {name!r} (have {sorted(PRESETS)})")
    return tf_from_points(PRESETS[name], n)
