"""The label volumes the surface-net tests share: (name, labels int16 (n0, n1, n2), class mask, spacing, origin, (V, T) or
None).  The counts are literals worked out from the definition by hand-checked means, so the NumPy
restatement in surface_ref.py is pinned by them as much as the kernels are."""
import functools

import numpy as np

UNIT, ZERO = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
BALL_SPACING = (0.5, 1.25, 2.0)


def ball(shape, radius, centre=None, label=1) -> np.ndarray:
    c = [(k - 1) / 2.0 for k in shape] if centre is None else centre
    g = np.indices(shape).astype(np.float64)
    d2 = sum((g[k] - c[k]) ** 2 for k in range(3))
    return np.where(d2 <= radius * radius, label, 0).astype(np.int16)


def random_labels() -> np.ndarray:
    return np.random.default_rng(7).integers(0, 5, (9, 6, 5)).astype(np.int16)


def _voxels(shape, *at) -> np.ndarray:
    v = np.zeros(shape, np.int16)
    for p in at:
        v[p] = 1
    return v


def _odd_labels() -> np.ndarray:
    """Labels -1, 32 and 1000 are outside whatever the mask; label 31 is the last one a mask can name."""
    rng = np.random.default_rng(11)
    return rng.choice(np.array([-1, 0, 1, 31, 32, 1000], dtype=np.int16), size=(7, 5, 6))


def _six_faces() -> np.ndarray:
    v = np.zeros((6, 7, 5), np.int16)
    v[:, 3, 2] = 2
    v[2, :, 2] = 2
    v[2, 3, :] = 2
    return v


@functools.lru_cache(maxsize=None)
def small_cases():
    rnd = random_labels()
    b = ball((24, 22, 20), 7.3)
    return (
        ("single_voxel", np.ones((1, 1, 1), np.int16), 0b10, UNIT, ZERO, (8, 12)),
        ("all_inside_3x4x5", np.ones((3, 4, 5), np.int16), 0b10, UNIT, ZERO, (96, 188)),
        ("ball_24x22x20", b, 0b10, UNIT, ZERO, (986, 1968)),
        ("ball_24x22x20_spaced", b, 0b10, BALL_SPACING, (-3.5, 0.25, 10.0), (986, 1968)),
        ("random_0b10", rnd, 0b10, UNIT, ZERO, (260, 496)),
        ("random_0b1110", rnd, 0b1110, (0.9375, 1.1, 1.3), (0.1, -0.2, 0.3), (406, 988)),
        ("random_0b1", rnd, 0b1, UNIT, ZERO, (256, 516)),
        ("corner_touch", _voxels((4, 4, 4), (1, 1, 1), (2, 2, 2)), 0b10, UNIT, ZERO, (15, 24)),
        ("edge_touch", _voxels((4, 4, 4), (1, 1, 1), (2, 2, 1)), 0b10, UNIT, ZERO, (14, 24)),
        ("empty_class", rnd, 1 << 9, UNIT, ZERO, (0, 0)),
        ("odd_labels_0b10", _odd_labels(), 0b10, UNIT, ZERO, None),
        ("odd_labels_all_bits", _odd_labels(), 0xFFFFFFFF, (1.0, 1.0, 2.5), ZERO, None),
        ("thin_1x7x1", np.array([0, 1, 1, 0, 1, 0, 1], np.int16).reshape(1, 7, 1), 0b10, UNIT, ZERO, None),
        ("thin_5x1x1", np.array([1, 1, 0, 2, 1], np.int16).reshape(5, 1, 1), 0b110, (0.7, 0.7, 3.3), ZERO, None),
        ("six_faces", _six_faces(), 0b100, UNIT, (-1.0, -2.0, -3.0), None),
    )


LARGE_SHAPE = (127, 97, 95)
LARGE_COUNTS = (16928, 33852)
LARGE_CELLS = 1204224


@functools.lru_cache(maxsize=None)
def large_case():
    """Ball of radius 30 centred in (127, 97, 95): 1 204 224 cells, so the scan runs over more than one level."""
    return ("ball_127x97x95", ball(LARGE_SHAPE, 30.0), 0b10, (0.9375, 0.9375, 1.2), (-59.0, -45.0, -57.0), LARGE_COUNTS)


def all_cases():
    return small_cases() + (large_case(),)
