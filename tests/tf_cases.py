"""Scenes and tables of the transfer-function tests (test_tf_host.py, test_gpu_tf.py): the smallest shapes at which the table
march can go wrong.  TEST INFRASTRUCTURE ONLY.

Geometry in the style of brats_soft_cases.py (brats_grad_cases._case builds the parameters): volumes of 13 x 9 x 7 and 8 x 8 x 8
voxels with values uniform in [-0.2, 1.2] (val reaches exactly 0 and exactly 1), frames of 24 x 20 (partial 8 x 8 packets), 8 x 8
and 1 x 1, at most 48 steps per ray, intensityAlpha 0.4 and 30, gamma 1 and 2.2, 1-4 weighted modalities, overlays off / seg /
seg + pred, the eye inside the box, a frame that misses, nearT / farT, the orthographic camera, an early-termination override,
shading on and off.

Tables: the two-entry ramp; N = 2, 3, 17, 256, 1024 with distinct r / g / b curves and a sigma curve that is 0 on [0, 0.3] and
reaches 1.75; one table with negative sigma entries; one all-zero table.  Every scene but the one whose rays all miss (where no
table can show) comes with a table that is not the ramp.
"""
import functools

import numpy as np

import brats_grad_cases as bc

# FAST tolerance of test_gpu_tf.py (rule of brats_soft_cases.py): 8 x the largest deviation of tf_ref evaluated in float32 from the
# same loop in float64 on FAST_CASES, capped at 1e-4.  Measured on the CPU on 2026-10-20 by
# test_tf_host.py::test_fp32_reference_error (it prints the figure and holds this constant to it).  Never derived from a kernel's output.
FP32_REF_ERROR = 2.4e-7       # measured 2.314e-07 (case n17_three_gamma_low; n256_shaded: 1.073e-07); 8 x it is 1.92e-6
TOL_FACTOR = 8.0
TOL_FAST = min(TOL_FACTOR * FP32_REF_ERROR, 1e-4)
RAMP_FAST_BAR = 2e-6          # the project's bar for FAST frames against the oracle (tests/test_gpu_parity.py)

SHADE = dict(shadeMode=1, ka=0.3, kd=0.6, ks=0.3, specPow2=5, gradEps=1e-6)


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def _curve(n):
    """Distinct r / g / b curves; sigma = 2.5 (x - 0.3) clipped at 0: zero on [0, 0.3], above 1 from x = 0.7."""
    x = np.arange(n, dtype=np.float64) / (n - 1)
    r = 0.05 + 0.9 * x
    g = 1.0 - 0.8 * x
    b = 0.5 + 0.45 * np.sin(6.0 * x)
    s = np.maximum(0.0, 2.5 * (x - 0.3))
    return np.stack([r, g, b, s], axis=1).astype(np.float32)


def _negative(n=17):
    """sigma = 1.5 cos(3 pi x): negative on (1/6, 1/2) and (5/6, 1]."""
    x = np.arange(n, dtype=np.float64) / (n - 1)
    return np.stack([0.2 + 0.7 * x, 0.9 - 0.5 * x, 0.3 + 0.4 * x * x, 1.5 * np.cos(3.0 * np.pi * x)], axis=1).astype(np.float32)


TABLES = {
    "ramp": np.array([[0, 0, 0, 0], [1, 1, 1, 1]], np.float32),
    "n2": _curve(2), "n3": _curve(3), "n17": _curve(17), "n256": _curve(256), "n1024": _curve(1024),
    "negative": _negative(),
    "zero": np.zeros((5, 4), np.float32),
}
for _t in TABLES.values():
    _t.setflags(write=False)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def _case(name, seed, dims, hw, enabled, weights, gamma, alpha, table, *, shade=False, overlays="off", dense=False, **kw):
    c = bc._case(name, seed, dims, hw, enabled, weights, gamma, alpha, **kw)
    c["params"].update(showSeg=int(overlays in ("seg", "seg+pred")), showPred=int(overlays == "seg+pred"))
    if shade:
        c["ext"].update(SHADE)
    c.update(table=table, shade=shade, overlays=overlays, dense=dense)
    del c["grad"]
    return c


ONE = (1.0, 1.0, 1.0, 1.0)
CASES = [
    # the ramp: the three scenes the definition was tried on, and the frame that misses
    _case("ramp_one", 201, (13, 9, 7), (20, 24), (1, 0, 0, 0), ONE, 1.0, 0.4, "ramp"),
    _case("ramp_three_gamma_seg", 202, (13, 9, 7), (20, 24), (1, 1, 0, 1), (0.7, 1.6, 1.0, 1.2), 2.2, 30.0, "ramp", overlays="seg", dense=True),
    _case("ramp_shaded_dense", 203, (8, 8, 8), (20, 24), (1, 0, 0, 0), ONE, 1.0, 30.0, "ramp", shade=True, dense=True),
    _case("ramp_shaded_low", 218, (13, 9, 7), (20, 24), (0, 1, 1, 0), (1.0, 0.6, 1.4, 1.0), 2.2, 0.4, "ramp", shade=True),
    _case("ramp_all_miss", 204, (8, 8, 8), (20, 24), (1, 0, 0, 0), ONE, 1.0, 0.4, "ramp", target=(5.0, 4.0, -2.1)),
    # general tables
    _case("n2_one", 205, (8, 8, 8), (20, 24), (1, 0, 0, 0), ONE, 1.0, 0.4, "n2"),
    _case("n3_two_gamma_seg", 206, (13, 9, 7), (20, 24), (1, 1, 0, 0), (0.7, 1.6, 1.0, 1.0), 2.2, 0.4, "n3", overlays="seg", ww=0.8, wl=0.45),
    _case("n17_four_dense_overlays", 207, (13, 9, 7), (20, 24), (1, 1, 1, 1), (0.5, 1.25, 0.75, 2.0), 2.2, 30.0, "n17", overlays="seg+pred", dense=True),
    _case("n17_three_gamma_low", 219, (13, 9, 7), (20, 24), (1, 1, 0, 1), (0.7, 1.6, 1.0, 1.2), 2.2, 0.4, "n17"),
    _case("n256_shaded", 208, (13, 9, 7), (20, 24), (1, 0, 0, 0), ONE, 1.0, 0.4, "n256", shade=True),
    _case("n1024_shaded_dense_seg", 209, (8, 8, 8), (20, 24), (1, 0, 1, 0), (1.5, 1.0, 0.5, 1.0), 1.0, 30.0, "n1024", shade=True, overlays="seg", dense=True),
    _case("negative_sigma", 210, (13, 9, 7), (20, 24), (1, 0, 0, 0), ONE, 1.0, 30.0, "negative"),
    _case("zero_table_seg", 211, (8, 8, 8), (20, 24), (1, 0, 0, 0), ONE, 1.0, 0.4, "zero", overlays="seg"),
    _case("eye_inside", 212, (13, 9, 7), (20, 24), (1, 0, 0, 0), (2.0, 1.0, 1.0, 1.0), 2.2, 0.4, "n17", eye=(0.1, 0.05, -0.1), target=(0.3, 0.1, 0.6), fov=1.2),
    _case("near_far_clip", 213, (13, 9, 7), (20, 24), (1, 1, 0, 0), ONE, 1.0, 30.0, "n256", near=2.1, far=2.6),
    _case("orthographic_shaded", 214, (8, 8, 8), (20, 24), (1, 0, 0, 0), ONE, 2.2, 0.4, "n3", shade=True, ortho=0.55),
    _case("one_packet_dense", 215, (8, 8, 8), (8, 8), (1, 0, 0, 0), ONE, 1.0, 30.0, "n17", dense=True),
    _case("one_pixel", 216, (8, 8, 8), (1, 1), (1, 0, 0, 0), ONE, 1.0, 30.0, "n1024"),
    _case("ert_override", 217, (8, 8, 8), (20, 24), (1, 0, 0, 0), ONE, 1.0, 30.0, "n17", ert=0.2, dense=True),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
RAMP_NAMES = [c["name"] for c in CASES if c["table"] == "ramp"]
GENERAL_NAMES = [c["name"] for c in CASES if c["table"] != "ramp"]
FAST_CASES = ["n17_three_gamma_low", "n256_shaded"]          # two low-opacity cases (intensityAlpha 0.4: no early termination)
# FAST against the oracle with the ramp: the low-opacity ramp scenes.  A FAST transmittance differs from the STRICT one in its last
# bits, so a ray whose T passes the early-termination threshold within that margin takes one sample more or less — a pixel error
# of up to threshold x colour, three orders above the bar; scenes where no ray terminates early have no such decision.
RAMP_FAST_CASES = ["ramp_one", "ramp_shaded_low"]


@functools.lru_cache(maxsize=None)
def data(name):
    """The case's arrays (made once, shared, never modified): vols [4 x (X*Y*Z) fp32 | None], labels / preds uint32 | None."""
    c = BY_NAME[name]
    rng = np.random.default_rng(c["seed"])
    n = int(np.prod(c["dims"]))
    vols = [rng.uniform(-0.2, 1.2, n).astype(np.float32) if c["params"]["volEnabled"][m] else None for m in range(4)]
    labels = rng.integers(0, 9, n).astype(np.uint32) if c["params"]["showSeg"] else None
    preds = rng.integers(0, 9, n).astype(np.uint32) if c["params"]["showPred"] else None
    for a in vols + [labels, preds]:
        if a is not None:
            a.setflags(write=False)
    return dict(vols=vols, labels=labels, preds=preds)


@functools.lru_cache(maxsize=None)
def reference(name, table=None):
    """tf_ref.march of the case in float32 with its own table (or another one of TABLES): computed once, shared, read-only."""
    import tf_ref
    c, d = BY_NAME[name], data(name)
    r = tf_ref.march(c["params"], d["vols"], d["labels"], d["preds"], c["ext"], TABLES[table or c["table"]])
    r["frame"].setflags(write=False)
    return r
