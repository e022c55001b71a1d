"""The cases of the coordinate-injection INR tests, shared by the CPU tests (which prove each exact case's preconditions)
and the GPU tests (which hold the kernels to them).  No GPU."""
import pathlib

import numpy as np

import inject_ref as ref

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"

# name, n, F, M, widths (head included), coord layers, mod layers, shift of the selection window
EXACT = [
    ("n1_F2_M0_L2", 1, 2, 0, (13, 4), (), (), 0),
    ("n63_F14_M1_L3_coords", 63, 14, 1, (16, 17, 1), (1,), (), 0),
    ("n64_F16_M4_L5_both_first_mods_last", 64, 16, 4, (17, 64, 65, 13, 4), (1,), (1, 3), 3),
    ("n65_F18_M8_L8_coords_first_both_last", 65, 18, 8, (64, 256, 16, 1, 65, 17, 13, 16), (1, 6), (6,), 7),
    ("n257_F128_M4_notebook", 257, 128, 4, (64, 64, 64, 4), (1, 2), (2,), 60),
    ("n257_F256_M8_L3_mods", 257, 256, 8, (256, 65, 16), (), (1,), 250),
    ("n65_F16_M1_L4_coords_last", 65, 16, 1, (1, 13, 1, 16), (2,), (), 0),
    ("n64_F2_M4_L5_mods_first_both_last", 64, 2, 4, (65, 16, 256, 17, 4), (3,), (1, 3), 11),
    ("n257_F16_M4_L3_none", 257, 16, 4, (17, 13, 4), (), (), 2),
]

# name, n, F, M, widths, coord layers, mod layers
TOLERANCE = [
    ("notebook_shape", 257, 128, 4, (64, 64, 64, 4), (1, 2), (2,)),
    ("widths_256_32_96", 257, 64, 4, (256, 32, 96, 4), (1,), (1, 2)),
]

INTEGER = [
    ("int_small", 65, 16, 4, (16, 17, 13, 4), (1, 2), (2,), 0.3),
    ("int_wide", 257, 128, 8, (64, 65, 4), (1,), (1,), 0.1),
]

VOLUMES = [(2, 2, 2), (12, 10, 8), (7, 33, 5)]


def seed_of(name):
    return int.from_bytes(name.encode()[:8].ljust(8, b"\0"), "little") % (2 ** 31)


def inputs(rng, n, M, special=True):
    """coords (n, 3) and mods (n, M); from 63 rows on, rows 3 .. 19 carry +-0, denormals, NaN and +-inf."""
    coords = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    mods = rng.normal(0, 1, (n, M)).astype(np.float32)
    if special and n >= 63:
        den = np.float32(1e-40)
        coords[3] = (0.0, -0.0, den)
        coords[7] = (np.nan, 0.5, -0.5)
        coords[11] = (np.inf, -np.inf, 0.25)
        coords[13] = (-den, np.float32(1e-45), np.float32(3e38))
        if M:
            mods[5] = np.resize(np.float32([0.0, -0.0, den, -den]), M)
            mods[17, 0] = np.nan
            mods[19, M - 1] = np.inf
            mods[21, 0] = -np.inf
    return coords, mods


def exact_case(case):
    name, n, F, M, widths, cl, ml, shift = case
    rng = np.random.default_rng(seed_of(name))
    params, rows = ref.selection_net(rng, F, M, widths, cl, ml, shift)
    if F >= 4:
        params["fourier"]["B"][-1] *= np.float32(1e6)          # |a| beyond 2^20 for most points: sin +0, cos 1
    coords, mods = inputs(rng, n, M)
    return params, rows, coords, mods


def tolerance_case(case):
    name, n, F, M, widths, cl, ml = case
    rng = np.random.default_rng(seed_of(name))
    params = ref.glorot_net(rng, F, M, widths, cl, ml)
    coords, mods = inputs(rng, n, M, special=False)
    return params, coords, mods


def integer_case(case):
    name, n, F, M, widths, cl, ml, density = case
    rng = np.random.default_rng(seed_of(name))
    params = ref.integer_net(rng, F, M, widths, cl, ml, density)
    coords8 = rng.integers(-8, 9, (n, 3))
    mods = rng.integers(-3, 4, (n, M))
    return params, coords8, mods


def tau(z32, z64):
    """The tolerance of the tolerance tier: 8 x the fp32 restatement's own distance from the fp64 tier (the project's margin
    for a different, equally valid fp32 summation order)."""
    return 8.0 * float(np.abs(np.asarray(z32, np.float64) - z64).max())


def load_golden():
    z = np.load(GOLDEN / "inject.npz")
    return {k: z[k] for k in z.files}


def load_boundary():
    z = np.load(GOLDEN / "boundary.npz")
    names = sorted(k[:-4] for k in z.files if k.endswith("_seg"))
    return [(n, z[n + "_seg"], z[n + "_w"]) for n in names]


def volume_case(hwd, M=4):
    rng = np.random.default_rng(hwd[0] * 10000 + hwd[1] * 100 + hwd[2])
    params = ref.glorot_net(rng, 16, M, (17, 64, 13, 4), (1, 2), (2,))
    mods = rng.normal(0, 1, (M, *hwd)).astype(np.float32)
    return params, mods
