"""The label volumes the connected-component tests share: (name, labels int16 (n0, n1, n2), class mask, {connectivity: N} or
None).  The listed counts follow from the shapes by hand, so they pin the NumPy restatement in cc_ref.py
as much as the kernels.  TILE is the label tile of csrc/cc_index.h; the tile cases have T - 1, T, T + 1 and 2 T + 1 voxels
along the axes and plant voxel pairs that touch only across a tile face, edge or corner."""
import functools
import itertools

import numpy as np

TILE = (8, 8, 32)
SERPENTINE_SHAPE = (33, 17, 70)
RANDOM_SHAPE = (33, 17, 65)


def _voxels(shape, *at) -> np.ndarray:
    v = np.zeros(shape, np.int16)
    for p in at:
        v[p] = 1
    return v


def serpentine(shape) -> np.ndarray:
    """A one-voxel-wide path that fills a box of odd extents along axes 0 and 1: full lines along axis 2 on the even rows of
    the even planes, joined at alternating ends through the odd rows, the planes joined through one voxel of the odd planes
    at the end the plane's path stops at.  One component under every connectivity."""
    n0, n1, n2 = shape
    assert n0 % 2 == 1 and n1 % 2 == 1 and n2 >= 3
    plane = np.zeros((n1, n2), np.int16)
    plane[0::2, :] = 1
    for r in range(1, n1, 2):
        plane[r, n2 - 1 if (r // 2) % 2 == 0 else 0] = 1
    rows = (n1 + 1) // 2
    end = (n1 - 1, n2 - 1 if (rows - 1) % 2 == 0 else 0)          # where the path that starts at (0, 0) stops
    v = np.zeros(shape, np.int16)
    v[0::2] = plane
    for p in range(1, n0, 2):
        v[(p,) + (end if (p // 2) % 2 == 0 else (0, 0))] = 1
    return v


def two_serpentines() -> np.ndarray:
    """Two serpentines in the halves of the last axis, the second mirrored along it and shifted by one voxel along
    the other two axes: no voxel of one shares a face with a voxel of the other, some share an edge or a corner."""
    v = np.zeros(SERPENTINE_SHAPE, np.int16)
    v[:, :, :35] = serpentine((33, 17, 35))
    v[1:32, 1:16, 35:] = serpentine((31, 15, 35))[:, :, ::-1]
    return v


def diagonal(kind: str) -> np.ndarray:
    v = np.zeros((9, 9, 9), np.int16)
    for i in range(9):
        v[(i, i, i) if kind == "main" else (i, i, 0)] = 1
    return v


def checkerboard(shape) -> np.ndarray:
    g = np.indices(shape).sum(axis=0)
    return (g % 2 == 0).astype(np.int16)


def isolated(count: int) -> np.ndarray:
    """`count` voxels no two of which are adjacent under any connectivity (every other voxel of every other row and plane)."""
    shape = (3, 33, 65)
    spots = [(a, b, c) for a in range(0, 3, 2) for b in range(0, 33, 2) for c in range(0, 65, 2)]
    assert count <= len(spots)
    return _voxels(shape, *spots[:count])


def random_labels(density: float, seed: int) -> np.ndarray:
    """Labels 1..5 on a `density` share of the voxels, 0 elsewhere, and a sprinkle of -1, 32 and 1000 (outside under every mask)."""
    rng = np.random.default_rng(seed)
    lab = np.where(rng.random(RANDOM_SHAPE) < density, rng.integers(1, 6, RANDOM_SHAPE), 0).astype(np.int16)
    odd = rng.random(RANDOM_SHAPE) < 0.01
    lab[odd] = rng.choice(np.array([-1, 32, 1000], np.int16), size=int(odd.sum()))
    return lab


def tile_case(shape, seed: int) -> np.ndarray:
    """Random voxels at density 0.45 (one giant component through every tile face under 6 neighbours), and at every interior
    tile corner pairs of voxels, alone in their 3 x 3 x 3 surroundings, that touch only across a tile face, a tile edge
    (both diagonals) or the tile corner (all four diagonals)."""
    rng = np.random.default_rng(seed)
    v = (rng.random(shape) < 0.45).astype(np.int16)
    planted = []

    def plant(a, b):
        for p in (a, b):
            if any(not 1 <= p[k] < shape[k] - 1 for k in range(3)):
                return
        for p in (a, b):
            v[p[0] - 1:p[0] + 2, p[1] - 1:p[1] + 2, p[2] - 1:p[2] + 2] = 0
        planted.extend([a, b])

    corners = itertools.product(*[range(TILE[k], shape[k], TILE[k]) for k in range(3)])
    for c in corners:
        c0, c1, c2 = c
        plant((c0 - 1, c1 - 1, c2 - 1), (c0, c1, c2))                       # the corner's main diagonal
        plant((c0 - 1, c1, c2 + 4), (c0, c1 - 1, c2 + 5))                          # (1, -1, 1) across an axis-2 edge region
        plant((c0 - 1, c1 + 3, c2 + 9), (c0, c1 + 3, c2 + 9))                      # a face along axis 0
        plant((c0 + 3, c1 - 1, c2 + 13), (c0 + 3, c1, c2 + 13))                    # a face along axis 1
        plant((c0 + 3, c1 + 3, c2 - 1), (c0 + 3, c1 + 3, c2))                      # a face along axis 2
        plant((c0 - 1, c1 - 1, c2 + 17), (c0, c1, c2 + 17))                        # an edge along axis 2
        plant((c0 - 1, c1, c2 + 21), (c0, c1 - 1, c2 + 21))                        # ... its other diagonal
        plant((c0 - 1, c1 - 4, c2 - 1), (c0, c1 - 4, c2))                          # an edge along axis 1
        plant((c0 - 1, c1 - 4, c2 - 6), (c0, c1 - 4, c2 - 7))                      # (1, 0, -1) inside the tile column: a plain pair
        plant((c0 - 4, c1 - 1, c2 - 1), (c0 - 4, c1, c2))                          # an edge along axis 0
        plant((c0 - 4, c1, c2 - 12), (c0 - 4, c1 - 1, c2 - 11))                    # ... (0, -1, 1)
    for p in planted:
        v[p] = 1
    return v


def _random_cases():
    out = []
    for density, seed, masks in ((0.2, 21, (0b111110, 0b10)), (0.31, 22, (0b111110, 0b101010, 0xFFFFFFFF)), (0.6, 23, (0b111110, 0b110))):
        lab = random_labels(density, seed)
        for m in masks:
            out.append((f"random_{density}_mask_{m:#x}", lab, m, None))
    return out


def _tile_cases():
    t0, t1, t2 = TILE
    shapes = [(t0 - 1, t1 - 1, t2 - 1), TILE, (t0 + 1, t1 + 1, t2 + 1), (2 * t0 + 1, 2 * t1 + 1, 2 * t2 + 1),
              (2 * t0 + 1, t1 - 1, t2 + 1), (t0 - 1, 2 * t1 + 1, t2), (t0 + 1, t1, 2 * t2 + 1)]
    return [("tile_%dx%dx%d" % s, tile_case(s, 40 + i), 0b10, None) for i, s in enumerate(shapes)]


@functools.lru_cache(maxsize=None)
def small_cases():
    corners = [(f"corner_{a}{b}{c}", _voxels((4, 5, 6), (3 * a, 4 * b, 5 * c)), 0b10, {1: 1, 2: 1, 3: 1})
               for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    return tuple([
        ("empty", np.zeros((4, 5, 6), np.int16), 0b10, {1: 0, 2: 0, 3: 0}),
        ("full_3x4x5", np.ones((3, 4, 5), np.int16), 0b10, {1: 1, 2: 1, 3: 1}),
        ("single_1x1x1", np.ones((1, 1, 1), np.int16), 0b10, {1: 1, 2: 1, 3: 1}),
        ("thin_1x7x1", np.array([0, 1, 1, 0, 1, 0, 1], np.int16).reshape(1, 7, 1), 0b10, {1: 3, 2: 3, 3: 3}),
        ("thin_5x1x1", np.array([1, 1, 0, 2, 1], np.int16).reshape(5, 1, 1), 0b110, {1: 2, 2: 2, 3: 2}),
        *corners,
        ("main_diagonal", diagonal("main"), 0b10, {1: 9, 2: 9, 3: 1}),
        ("face_diagonal", diagonal("face"), 0b10, {1: 9, 2: 1, 3: 1}),
        ("checkerboard_9x10x11", checkerboard((9, 10, 11)), 0b10, {1: 495, 2: 1, 3: 1}),
        ("serpentine", serpentine(SERPENTINE_SHAPE), 0b10, {1: 1, 2: 1, 3: 1}),
        ("two_serpentines", two_serpentines(), 0b10, {1: 2, 2: 1, 3: 1}),
        *_random_cases(),
        *_tile_cases(),
        *[(f"isolated_{k}", isolated(k), 0b10, {1: k, 2: k, 3: k}) for k in (1023, 1024, 1025)],
    ])


def by_name(name):
    return next(c for c in small_cases() if c[0] == name)


# --- the two larger cases: checked by properties and against the stored SciPy count and SHA-256 ---------------------------
LARGE_CHECKER_SHAPE = (128, 128, 130)
LARGE_CHECKER_ROOTS = 1064960                      # half of the voxels: more than 1024 * 1024, so the scan of the chunk sums recurses
BALL_SHAPE = (240, 240, 155)


@functools.lru_cache(maxsize=None)
def ball_with_noise() -> np.ndarray:
    """A ball of radius 40 centred in (240, 240, 155) plus 1 % of the voxels at random: one large component, tens of
    thousands of specks."""
    g = np.ogrid[:BALL_SHAPE[0], :BALL_SHAPE[1], :BALL_SHAPE[2]]
    d2 = sum((g[k] - (BALL_SHAPE[k] - 1) / 2.0) ** 2 for k in range(3))
    noise = np.random.default_rng(2024).random(BALL_SHAPE) < 0.01
    return ((d2 <= 40.0 * 40.0) | noise).astype(np.int16)


@functools.lru_cache(maxsize=None)
def large_cases():
    return (("checkerboard_128x128x130", checkerboard(LARGE_CHECKER_SHAPE), 0b10),
            ("ball_noise_240x240x155", ball_with_noise(), 0b10))


# --- prediction / truth pairs of the compute_multi_metrics goldens ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def metric_pairs():
    rng = np.random.default_rng(77)
    shape = (12, 11, 9)
    truth = rng.integers(0, 4, shape).astype(np.int16)
    pred = np.where(rng.random(shape) < 0.7, truth, rng.integers(0, 4, shape)).astype(np.int16)
    absent_p, absent_t = pred.copy(), truth.copy()
    absent_p[absent_p == 2] = 0                    # class 2 occurs in neither volume
    absent_t[absent_t == 2] = 0
    zeros = np.zeros(shape, np.int16)
    same = pred.copy()
    same[:, :, 3] = same[:, :, 2]                  # identical consecutive slices
    same[:, :, 4] = same[:, :, 2]
    same[:, :, 7] = 0                              # and an empty slice between non-empty ones
    return (("absent_class", absent_p, absent_t), ("all_background", zeros, zeros.copy()), ("identical_slices", same, truth))
