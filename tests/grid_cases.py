"""Inputs shared by tests/test_grid_ref_host.py, tests/test_gpu_grid_builders.py and tests/test_gpu_skip_map.py: the dims
that reach every branch of the load-time builders, value fields that make a misplaced or mangled voxel visible, and the
volumes constructed for the skip-map tests.  NumPy only."""
from __future__ import annotations

import itertools

import numpy as np

import grid_ref as gr

F = np.float32

# dims -> the branch of the builders it reaches
BUILDER_DIMS = [
    (1, 1, 1),       # fully degenerate (MOD4 and LABCELL refuse it)
    (2, 2, 2),       # smallest volume MOD4 accepts
    (5, 1, 3),       # a degenerate axis: both clamps land on the one voxel
    (9, 7, 5),       # odd on every axis
    (16, 8, 8),      # no padding anywhere
    (67, 9, 5),      # VGA copy 0 has 67 lines per row: row pitch padded to 72, slice pitch to 228
    (13, 70, 3),     # the slice pitch is padded while the row pitch is not
    (261, 5, 4),     # copies 1 and 2 have 66 lines per row: row padding on the 4-wide axis
]

# (rowLines, sliceLines) of the three axis-flat copies, worked out by hand from the layout's definition: bricks per axis
# (flat axis: dims; first other axis: ceil(d / 4); second: ceil(d / 2)), pitches of >= 64 lines moved up to 8 (rows) and
# 36 (slices) modulo 64.  A change of the phases or of the threshold shows up here, not as a silently unpadded case.
VGA_PITCHES = {
    (16, 8, 8): [(16, 32), (4, 32), (4, 16)],             # nothing reaches 64 lines
    (67, 9, 5): [(72, 228), (17, 164), (17, 100)],        # 67 -> 72; 72 * 3 = 216 -> 228; 17 * 9 = 153 -> 164; 17 * 5 = 85 -> 100
    (13, 70, 3): [(13, 292), (4, 292), (4, 164)],         # 13 * 18 = 234 -> 292; 4 * 70 = 280 -> 292; 4 * 35 = 140 -> 164
    (261, 5, 4): [(264, 548), (72, 420), (72, 228)],      # 261 -> 264; 264 * 2 = 528 -> 548; 66 -> 72; 72 * 5 = 360 -> 420; 72 * 3 = 216 -> 228
}
# bricks per axis (x, y, z) of the three copies: flat axis d, first other axis ceil(d / 4), second ceil(d / 2)
VGA_BRICKS = {(16, 8, 8): [(16, 2, 4), (4, 8, 4), (4, 4, 8)], (67, 9, 5): [(67, 3, 3), (17, 9, 3), (17, 5, 5)],
              (13, 70, 3): [(13, 18, 2), (4, 70, 2), (4, 35, 3)], (261, 5, 4): [(261, 2, 2), (66, 5, 2), (66, 3, 4)]}

MACRO_DIMS = [(8, 8, 8), (9, 9, 9), (17, 8, 1), (65, 41, 17)]     # (9,9,9): last macro cells one voxel thick
SKIP_DIMS = (65, 41, 17)                                          # 9 x 6 x 3 = 162 cells: the last ballot is ragged
SPIKE_DIMS = (33, 25, 17)


def nvox(dims) -> int:
    return int(dims[0]) * int(dims[1]) * int(dims[2])


def distinct_field(dims, scale: float = 1.0, offset: float = 1.0) -> np.ndarray:
    """Every voxel a different, exactly representable value."""
    return (np.arange(nvox(dims), dtype=np.float64) * scale + offset).astype(F)


def wild_field(dims, seed: int) -> np.ndarray:
    """A random field with +-0.0, denormals, +-inf and NaN planted in it (about a fifth of the voxels)."""
    rng = np.random.default_rng(seed)
    n = nvox(dims)
    v = rng.standard_normal(n).astype(F)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, np.inf, -np.inf, np.nan, 3e38, -3e38], dtype=F)
    pick = rng.random(n) < 0.2
    v[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return v


def same_floats(got: np.ndarray, want: np.ndarray) -> bool:
    """Bit patterns of the non-NaN elements, NaN-ness of the rest."""
    got, want = np.ascontiguousarray(got, F).reshape(-1), np.ascontiguousarray(want, F).reshape(-1)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def boundary_coords(D: int):
    """{0, 7, 8, 9, D - 1} as far as the axis holds them."""
    return sorted({c for c in (0, 7, 8, 9, D - 1) if 0 <= c < D})


def spike_field(dims):
    """Zeros with one spike at every combination of the boundary coordinates, each of another height (k + 1 for the k-th),
    so the bound of a macro cell names the highest spike it sees.  Returns (field, [(x, y, z, height)])."""
    X, Y, Z = dims
    v = np.zeros((Z, Y, X), F)
    spikes = []
    for k, (z, y, x) in enumerate(itertools.product(boundary_coords(Z), boundary_coords(Y), boundary_coords(X))):
        v[z, y, x] = F(k + 1)
        spikes.append((x, y, z, F(k + 1)))
    return v.reshape(-1), spikes


def cells_seeing(x, y, z, dims):
    """Linear indices of the macro cells whose inclusive range holds voxel (x, y, z)."""
    mx, my, _ = gr.macro_dims(dims)
    return [cx + mx * (cy + my * cz) for cz in gr.axis_cells(z, dims[2]) for cy in gr.axis_cells(y, dims[1])
            for cx in gr.axis_cells(x, dims[0])]


def sparse_labels(dims, seed: int) -> np.ndarray:
    """Random sparse labels 1..12 (so one >= 8), one at the last voxel."""
    rng = np.random.default_rng(seed)
    n = nvox(dims)
    lab = np.zeros(n, np.uint32)
    idx = rng.choice(n, size=max(1, n // 97), replace=False)
    lab[idx] = rng.integers(1, 13, idx.size)
    lab[idx[0]] = 9
    lab[n - 1] = 5
    return lab


# ----------------------------------------------------------------------------------------------------------------------
# skip-map inputs
# ----------------------------------------------------------------------------------------------------------------------
AIR_FROM_X = 48       # the skip volumes hold nothing at x >= 48: a label blob there floats in empty air


def air_labels(dims, label: int = 2, at=(9, 17, 55)) -> np.ndarray:
    """One small label blob (2 x 3 x 2 voxels from ``at`` = (z, y, x)) in the air region; the default one touches a
    macro-cell boundary plane (x = 56)."""
    X, Y, Z = dims
    z, y, x = at
    assert x >= AIR_FROM_X
    lab = np.zeros((Z, Y, X), np.uint32)
    lab[z:z + 2, y:y + 3, x:x + 2] = label
    return lab.reshape(-1)


def textured_volumes(dims, channels: int, seed: int):
    """Random fields whose amplitude varies slowly over the volume (so macro-cell bounds spread widely), zero in the air."""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    out = []
    for c in range(channels):
        amp = 0.5 + 0.5 * np.sin(0.11 * x + 0.9 * c) * np.cos(0.17 * y - 0.4 * c) * np.sin(0.35 * z + 0.2)
        v = (amp ** 3 * rng.random((Z, Y, X))).astype(F)
        v[:, :, AIR_FROM_X:] = 0
        out.append(v.reshape(-1))
    return out


def gap_volumes(dims, channels: int, seed: int):
    """Voxels exactly 0 or drawn from [0.3, 0.9]; every channel has the same support (a few boxes, none in the air), so a
    weighted mean over the channels is 0 or >= 0.3 as well."""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    support = np.zeros((Z, Y, X), bool)
    for _ in range(6):
        x0, y0, z0 = rng.integers(0, AIR_FROM_X - 12), rng.integers(0, Y - 6), rng.integers(0, Z - 4)
        support[z0:z0 + rng.integers(1, 7), y0:y0 + rng.integers(1, 12), x0:x0 + rng.integers(1, 12)] = True
    support[8, 16, 24] = True                           # and one lone voxel on three macro-cell boundary planes
    out = []
    for _ in range(channels):
        v = np.where(support, 0.3 + 0.6 * rng.random((Z, Y, X)), 0.0).astype(F)
        out.append(np.clip(v, 0, F(0.9)).reshape(-1))
    return out


GAP_WL, GAP_WW = F(0.45), F(0.7)                         # window floor fl(0.45 - 0.35): 0.1

WEIGHTS = {"equal": (1.0, 1.0, 1.0, 1.0), "unequal": (0.7, 0.0, 2.5, 1.3)}


def enabled_of(channels: int):
    return tuple(1 if m < channels else 0 for m in range(4))


# spikes of the frame tests, every coordinate from {0, 7, 8, 9, D - 1}: spread over the box, many voxels apart
FRAME_SPIKES = [(0, 0, 0), (8, 8, 8), (32, 24, 16), (24, 7, 9), (7, 16, 16), (9, 24, 0)]


def frame_spike_volume(dims=SPIKE_DIMS, dtype=F, height=1):
    X, Y, Z = dims
    v = np.zeros((Z, Y, X), dtype)
    for x, y, z in FRAME_SPIKES:
        v[z, y, x] = height
    return v.reshape(-1)


def frame_spike_cells(dims=SPIKE_DIMS) -> np.ndarray:
    """Boolean per macro cell: must stay non-empty."""
    need = np.zeros(int(np.prod(gr.macro_dims(dims))), bool)
    for x, y, z in FRAME_SPIKES:
        need[cells_seeing(x, y, z, dims)] = True
    return need
