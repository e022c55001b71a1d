"""The cases of the coordinate-injection INR's training-step tests, shared by the CPU tests (which prove each exact case's
preconditions) and the GPU tests (which hold the kernels to them).  Built on inject_ref's selection_net, integer_net and
glorot_net.  No GPU."""
import numpy as np

import inject_cases as ic
import inject_ref as ref
import inject_train_ref as tref

SEED = 0x51ED5EEDC0FFEE

# name, n, F, M, widths (head included), coord layers, mod layers, weight density, keep, accumulate.
# n: one point, 63 / 64 / 65 around the 64-row block, 257 (slabs of 256 + 1), 321 (five blocks + one row; 256 + 65), 4000 (the
# notebook's micro-batch: 15 slabs and a 160-point tail) and 16385 (33 slabs of 512, one point in the last).  Layer 1 of the
# second and third net takes 60 + 3 and 61 + 3 inputs: with the row of ones X^T . dZ has 64 and 65 rows.
INTEGER = [
    ("n1_F2_M0_L2_out4", 1, 2, 0, (13, 4), (), (), 1.0, 1.0, False),
    ("n63_F14_M1_L3_rows64_out1", 63, 14, 1, (60, 17, 1), (1,), (), 0.3, 0.5, True),
    ("n64_F16_M4_L3_rows65_out3", 64, 16, 4, (61, 16, 3), (1,), (), 0.3, 0.25, False),
    ("n65_F18_M8_L5_out15", 65, 18, 8, (17, 64, 65, 13, 15), (1,), (1, 3), 0.15, 0.5, False),
    ("n257_F16_M4_L8_out16", 257, 16, 4, (16, 13, 17, 16, 13, 16, 17, 16), (1, 6), (6,), 0.4, 0.5, True),
    ("n321_F128_M4_notebook", 321, 128, 4, (64, 64, 64, 4), (1, 2), (2,), 0.08, 0.5, False),
    ("n4000_F128_M4_notebook", 4000, 128, 4, (64, 64, 64, 4), (1, 2), (2,), 0.08, 1.0, True),
    ("n257_F256_M8_L3_w256", 257, 256, 8, (256, 65, 16), (), (1,), 0.04, 0.25, False),
    ("n4000_F14_M1_L3", 4000, 14, 1, (16, 17, 4), (1,), (1,), 0.3, 0.25, False),
    ("n65_F2_M1_L5_w1_coords_last", 65, 2, 1, (1, 13, 1, 16, 4), (3,), (), 1.0, 0.5, False),
    ("n16385_F2_M1_L3_narrow", 16385, 2, 1, (13, 16, 4), (1,), (), 0.3, 0.5, False),
]

# the EXACT nets of inject_cases.py; per net the rows (modulo the slab) that carry the one non-zero dlogits row of each slab:
# plain rows, the rows of +-0 / denormal coords (3, 13) and mods (5), NaN (7, 17) and +-inf (11, 19, 21) inputs
SELECTION_ROWS = (0, 1, 3, 5, 7, 11, 13, 17, 19, 21, 40, 62)

# name, n, net of inject_cases.TOLERANCE
TOLERANCE = [(f"{c[0]}_n{n}", n, c) for c in ic.TOLERANCE for n in (257, 4000)]
TOL_KEEP = 0.7
TOL_ORDERS = 5


def dropout_of(keep, s=3):
    return None if keep == 1.0 else dict(seed=SEED, keep=keep, s=s)


def sparse_dlogits(rng, n, C, density=0.1):
    return (rng.integers(-2, 3, (n, C)) * (rng.random((n, C)) < density)).astype(np.int64)


def integer_case(case):
    """params, coords8, mods, dlogits (int64), dropout, old (non-zero integer gradients to accumulate onto, or None)."""
    name, n, F, M, widths, cl, ml, density, keep, accumulate = case
    rng = np.random.default_rng(ic.seed_of(name) + n)
    params = ref.integer_net(rng, F, M, widths, cl, ml, density)
    coords8 = rng.integers(-8, 9, (n, 3))
    mods = rng.integers(-3, 4, (n, M))
    dl = sparse_dlogits(rng, n, widths[-1], 1.0 if n < 64 else 0.1)
    old = None
    if accumulate:
        old = dict(B=rng.integers(-4, 5, (F // 2, 3)).astype(np.float32), W=[rng.integers(-4, 5, p["W"].shape).astype(np.float32) for p in params["mlp"]],
                   b=[rng.integers(-4, 5, p["b"].shape).astype(np.float32) for p in params["mlp"]])
    return params, coords8, mods, dl, dropout_of(keep), old


def selection_case(case):
    """An EXACT net of inject_cases.py made a training case: real sines (B ~ N(0, 5), the last row beyond the domain), the
    special inputs, and in every hidden layer unit 0 without a bias (z == 0 wherever its input is +-0) and unit 1 dead (a bias
    of -1e30)."""
    params, rows, coords, mods = ic.exact_case(case)
    for p in params["mlp"][:-1]:
        p["b"][0] = 0.0
        if p["b"].size > 1:
            p["b"][1] = -1e30
    return params, rows, coords, mods


def one_row_per_slab(rng, n, C, row):
    """dlogits with one non-zero row in every slab (row `row` of the slab, the last one where the slab is shorter)."""
    dl = np.zeros((n, C), np.float32)
    length = tref.slab_len(n)
    for z0 in range(0, n, length):
        r = z0 + min(row, min(length, n - z0) - 1)
        dl[r] = (np.float32(2.0) ** rng.integers(-3, 4, C)).astype(np.float32) * rng.choice(np.float32([-1, 1]), C)
    return dl


def tolerance_case(tc):
    """params, coords, mods, dlogits (normal / n), dropout at keep 0.7."""
    name, n, (net, _, F, M, widths, cl, ml) = tc
    rng = np.random.default_rng(ic.seed_of(net) + n)
    params = ref.glorot_net(rng, F, M, widths, cl, ml)
    coords, mods = ic.inputs(rng, n, M, special=False)
    dl = (rng.normal(0, 1, (n, widths[-1])) / n).astype(np.float32)
    return params, coords, mods, dl, dropout_of(TOL_KEEP)


def tolerance_reference(tc):
    """What the tolerance tier needs, computed once: the case with the dlogits rows of the points near a ReLU kink zeroed (a
    condition on the inputs), grads64 of it, the share removed, and tol = 8 x the worst deviation of backward32 from grads64,
    relative to A, over TOL_ORDERS orders of the batch (the identity first)."""
    params, coords, mods, dl, drop = tolerance_case(tc)
    cl, ml = tc[2][5], tc[2][6]
    n = coords.shape[0]
    first = tref.grads64(params, coords, mods, cl, ml, dl, drop)
    bad = tref.near_kink(first["z"])
    dl = dl.copy()
    dl[bad] = 0.0
    g64 = tref.grads64(params, coords, mods, cl, ml, dl, drop)
    rng = np.random.default_rng(n)
    worst = 0.0
    for k in range(TOL_ORDERS):
        order = np.arange(n) if k == 0 else rng.permutation(n)
        g32 = tref.backward32(params, coords[order], mods[order], cl, ml, dl[order], drop, index=order)
        worst = max(worst, tref.relative_deviation(g32, g64))
    return dict(params=params, coords=coords, mods=mods, dlogits=dl, dropout=drop, g64=g64, removed=int(bad.sum()), tol=8.0 * worst)
