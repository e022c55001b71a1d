"""Inputs of the unified-loss tests: the golden configurations (tests/golden/unified_loss.npz is generated from them), the GPU
tolerance cases with their measured tolerances, and the conditions the inputs are built to meet so that no point has to be
left out of a comparison."""
import pathlib

import numpy as np

import unified_loss_ref as ref

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "unified_loss.npz"
NOTEBOOK_CW = [0.1, 1.5, 1.0, 2.0]

# name, n, C, seed, logit scale, class weights, gamma, lambda, tv weight, boundary weight, features
GOLDEN_CASES = [
    ("c4_plain", 200, 4, 11, 2.0, NOTEBOOK_CW, 0.5, 0.5, 0.02, 0.1, ()),
    ("c4_tv05", 193, 4, 12, 3.0, NOTEBOOK_CW, 0.5, 0.5, 0.05, 0.1, ()),
    ("c3_plain", 150, 3, 13, 2.0, [0.5, 1.0, 2.0], 0.5, 0.5, 0.02, 0.1, ()),
    ("c1", 40, 1, 14, 2.0, [1.0], 0.5, 0.5, 0.02, 0.1, ()),
    ("c4_absent_class", 180, 4, 15, 2.0, NOTEBOOK_CW, 0.5, 0.5, 0.05, 0.1, ("absent",)),
    ("c4_labels_outside", 170, 4, 16, 2.0, NOTEBOOK_CW, 0.5, 0.5, 0.02, 0.25, ("outside",)),
    ("c4_beyond_clip", 160, 4, 17, 2.0, NOTEBOOK_CW, 0.5, 0.5, 0.02, 0.1, ("big",)),
    ("c3_saturated", 140, 3, 18, 2.0, [1.0, 1.0, 1.0], 0.5, 0.5, 0.05, 0.1, ("saturated",)),
    ("c3_gamma1_lambda0", 130, 3, 19, 1.5, [0.5, 1.0, 2.0], 1.0, 0.0, 0.02, 0.1, ("outside",)),
    ("c4_gamma025_lambda1_no_boundary", 120, 4, 20, 1.5, NOTEBOOK_CW, 0.25, 1.0, 0.05, 0.0, ("big", "no_bw")),
]

EDGE, GAP, PROB = 1e-4, 1e-4, 1e-9      # the conditions below
PROB_HI = 6.5e-8                         # ... and the band around the fp32 value of 1 - 1e-7: one fp32 spacing below 1


def _prob_rows(z):
    """Rows with a clipped-softmax value within PROB of a probability clip (the fp32 and the fp64 value of each clip both), or
    within PROB_HI of the fp32 value of the upper one."""
    zc = np.clip(z.astype(np.float64), -10.0, 10.0)
    e = np.exp(zc - zc.max(1, keepdims=True))
    ps = e / e.sum(1, keepdims=True)
    hi32, hi64 = float(np.float32(1.0) - np.float32(1e-7)), 1.0 - 1e-7
    lo32, lo64 = float(np.float32(1e-7)), 1e-7
    # next to 1 the fp32 grid has a spacing of 6e-8: every value that rounds to the fp32 clip sits ON the closed edge there
    near_hi = (ps > hi32 - PROB_HI) & (ps < max(hi32 + PROB_HI, hi64 + PROB))
    near_lo = (ps > min(lo32, lo64) - PROB) & (ps < max(lo32, lo64) + PROB)
    return (near_hi | near_lo).any(1)


def condition(z):
    """Move the logits that sit within EDGE of +-10, leave a top-two gap below GAP or put a probability next to a clip (in place,
    fp32): the inputs are built to meet conditions_met, no point is dropped afterwards."""
    for _ in range(32):
        near = np.abs(np.abs(z) - 10.0) < 2 * EDGE
        z[near] += np.float32(0.01)
        bad = _prob_rows(z)
        if z.shape[1] > 1:
            win = np.zeros(z.shape, bool)
            win[np.arange(len(z)), np.argmax(z, 1)] = True
            z[bad[:, None] & ~win] -= np.float32(0.125)           # a winner beyond the clip cannot move the probabilities: the others do
            top = np.sort(z, 1)
            bad |= (top[:, -1] - top[:, -2]) < 2 * GAP
            z[bad, np.argmax(z[bad], 1)] += np.float32(0.125)
        if not near.any() and not bad.any():
            break
    return z


def make_inputs(n, C, seed, scale, features=(), dyadic_bw=False):
    """(logits (n, C) fp32, labels (n,) int32, boundary weights (n,) fp32 or None)."""
    rng = np.random.default_rng(seed)
    z = rng.normal(0.0, scale, (n, C)).astype(np.float32)
    labels = rng.integers(0, C, n).astype(np.int32)
    if "absent" in features and C > 2:
        labels[labels == 2] = 1
    if "outside" in features:
        labels[::7] = C + 1
        labels[3::11] = -2
        labels[5::29] = C + 7
    if "big" in features:
        for r, v in zip(range(2, n, 9), (12.0, -12.0, 20.0, -20.0, 12.0, 20.0)):
            z[r, r % C] = v
        if n > 60:
            z[60] = 20.0                                         # every logit beyond the clip
            z[60, 0] = 25.0
    if "saturated" in features and C > 1:
        z[1::17] = -9.5
        z[1::17, 0] = 9.5                                        # softmax of the clipped logits beyond 1 - 1e-7, no logit clipped
        z[2::17, 1:] -= 6.0                                      # and some probabilities below 1e-7 with a moderate winner
        z[2::17, 0] += 12.0
    z = condition(z)
    if "no_bw" in features:
        return z, labels, None
    bw = (rng.integers(0, 17, n) / 16.0).astype(np.float32) if dyadic_bw else rng.random(n).astype(np.float32)
    return z, labels, bw


def golden_case(case, round32=False):
    """Inputs and config of a golden case; the config in the notebook's own fp64 constants unless ``round32``."""
    name, n, C, seed, scale, cw, gamma, lam, tv, bd, features = case
    z, labels, bw = make_inputs(n, C, seed, scale, features)
    return z, labels, bw, ref.config(cw, gamma, lam, tv_w=tv, bd_w=bd, round32=round32)


def conditions_met(z):
    """What the tolerance cases promise: no |z| within EDGE of 10, no top-two gap below GAP, no clipped-softmax value within
    PROB of either probability clip (the fp32 and the fp64 value of 1 - 1e-7 both)."""
    z64 = z.astype(np.float64)
    if (np.abs(np.abs(z64) - 10.0) < EDGE).any():
        return False
    if z.shape[1] > 1:
        top = np.sort(z64, 1)
        if ((top[:, -1] - top[:, -2]) < GAP).any():
            return False
    return not _prob_rows(z).any()


# ---- GPU tolerance tier -----------------------------------------------------------------------------------------------------------
# name, n, C, seed, scale, class weights, gamma, lambda, tv weight, boundary weight, features
TOLERANCE_CASES = [
    ("n1_c4", 1, 4, 31, 2.0, NOTEBOOK_CW, 0.5, 0.5, 0.02, 0.1, ()),
    ("n255_c3", 255, 3, 32, 2.0, [0.5, 1.0, 2.0], 0.5, 0.5, 0.05, 0.1, ("outside",)),
    ("n256_c4", 256, 4, 33, 3.0, NOTEBOOK_CW, 0.5, 0.5, 0.02, 0.1, ("big",)),
    ("n257_c16", 257, 16, 34, 2.0, [0.25 + 0.125 * k for k in range(16)], 0.75, 0.25, 0.02, 0.1, ("outside", "big")),
    ("n257_c1", 257, 1, 35, 2.0, [1.0], 0.5, 0.5, 0.02, 0.1, ()),
    ("n4000_c4", 4000, 4, 36, 2.5, NOTEBOOK_CW, 0.5, 0.5, 0.05, 0.1, ("saturated", "big", "outside")),
    ("n4000_c4_gamma025", 4000, 4, 37, 2.0, NOTEBOOK_CW, 0.25, 0.75, 0.02, 0.1, ("absent",)),
    ("n65537_c4", 65537, 4, 38, 2.0, NOTEBOOK_CW, 0.5, 0.5, 0.02, 0.1, ("big",)),
]

# tol = 8 x the worst deviation of the fp32 restatement from the fp64 one over five batch orders, measured on the CPU
# (measure below; test_unified_loss_ref.py re-derives one).  "scalar": loss and every aux entry, relative to
# max(|fp64 value|, 1), the fp32 restatement's values rounded to fp32 as the ABI stores them; "grad": dlogits per element,
# relative to A (unified_loss_ref.closed_form).
TOLERANCES = {}          # filled by the block below


def measure(case, orders=5):
    """(scalar, grad): the worst deviations of the fp32 restatement from fp64 over `orders` batch orders."""
    name, n, C, seed, scale, cw, gamma, lam, tv, bd, features = case
    z, labels, bw = make_inputs(n, C, seed, scale, features)
    cfg = ref.config(cw, gamma, lam, tv_w=tv, bd_w=bd)
    worst_s = worst_g = 0.0
    rng = np.random.default_rng(seed + 1000)
    for o in range(orders):
        perm = np.arange(n) if o == 0 else rng.permutation(n)
        zz, ll, bb = z[perm], labels[perm], (bw[perm] if bw is not None else None)
        l64, a64, g64, _ = ref.forward(zz, ll, bb, cfg)
        l32, a32, g32, _ = ref.forward(zz, ll, bb, cfg, dtype=__import__("torch").float32)
        v64, v32 = np.concatenate([[l64], ref.aux_vector(a64)]), np.concatenate([[l32], ref.aux_vector(a32)])
        v32 = v32.astype(np.float32).astype(np.float64)      # loss and aux are fp32 in the ABI: the last rounding is part of the deviation
        worst_s = max(worst_s, float((np.abs(v32 - v64) / np.maximum(np.abs(v64), 1.0)).max()))
        _, A = ref.closed_form(zz, ll, bb, cfg)
        ok = A > 0
        worst_g = max(worst_g, float((np.abs(g32 - g64)[ok] / A[ok]).max()) if ok.any() else 0.0)
    return worst_s, worst_g


# measured 2026-10-21 on the CPU (x86-64, torch fp32 / fp64): 8 x measure(case)
TOLERANCES.update({
    "n1_c4": (2.418e-07, 3.478e-07),                 # one point has one batch order: 8 x a single deviation
    "n255_c3": (2.113e-07, 2.453e-06),
    "n256_c4": (2.017e-07, 2.606e-05),
    "n257_c16": (3.018e-07, 4.923e-06),
    "n257_c1": (7.761e-08, 0.000e+00),               # C == 1: every term of the gradient is exactly 0 in fp32 and in fp64
    "n4000_c4": (3.231e-07, 7.373e-04),              # saturated rows: 1 - pc_y carries the fp32 spacing next to 1
    "n4000_c4_gamma025": (2.369e-07, 3.738e-06),
    "n65537_c4": (3.725e-07, 1.010e-05),
})

if __name__ == "__main__":
    for case in TOLERANCE_CASES:
        s, g = measure(case)
        print(f'    "{case[0]}": ({8 * s:.3e}, {8 * g:.3e}),')
