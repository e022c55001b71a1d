"""Scenes of the soft prediction overlay's tests (test_brats_soft_host.py, test_brats_soft_sanitizers.py, test_gpu_brats_soft.py):
the smallest shapes at which the two kernels can go wrong.  TEST INFRASTRUCTURE ONLY.

Geometry in the style of brats_grad_cases.py (its `_case` builds the parameters): volumes of 13 x 9 x 7 and 8 x 8 x 8 voxels,
frames of 24 x 20 (partial 8 x 8 packets) and 8 x 8, at most 48 steps per ray, C in {1, 2, 4, 9, 16} (the dword and the dwordx4 row
paths, classes >= 8 that draw nothing), intensityAlpha 0.4 and 30 (part of the rays terminate early), the ground-truth overlay
on and off, the eye inside the box, a frame that misses the box, nearT / farT clipping, the orthographic camera; G random
normal, all ones, zero on half the image; one case whose rays are laid out from the last pixel to the first with gap rows
between them (the kernels must go by `offsets`, not by a running count).

Seeds are chosen on the CPU (test_brats_soft_host.py::test_decisions_have_margin) so that no loop test sits on a knife edge
where fp32 and fp64 would decide differently; a case that needs another seed gets one here, no sample is ever excluded.
"""
import functools

import numpy as np

import brats_grad_cases as bc
import brats_soft_ref as ref

# Tolerances of the GPU comparisons.  Frame: |C - C_ref| <= TOL_F.  Gradients: |d - d_ref| <= TOL_G * A (A: brats_soft_ref.py).
# Both are 8 x the fp64 reference's OWN fp32 deviation (the same loop evaluated in float32), measured on the CPU on 2026-10-19
# by test_brats_soft_host.py::test_fp32_reference_error over all cases below, capped at 1e-5 / 1e-3: a dropped event or a wrong
# LUT row errs by >= 1e-3 of a pixel and >= 1e-2 A.  Never derived from a kernel's output.
FP32_REF_ERROR_FRAME = 3.3e-7      # measured 3.240e-07 (case reversed_gaps); 8 x it is 2.6e-6
FP32_REF_ERROR_GRAD = 1.8e-7       # measured 1.725e-07 of A (case reversed_gaps); 8 x it is 1.4e-6
FP32_REF_ERROR_E2E_FRAME = 3.7e-7  # the end-to-end composition (MLP + render), both networks: measured 3.676e-07 (SIREN)
FP32_REF_ERROR_E2E_GRAD = 5.0e-9   # measured 4.997e-09 of A (SIREN; A sums ~4400 samples' absolute terms per weight)
TOL_FACTOR = 8.0
TOL_F = min(TOL_FACTOR * FP32_REF_ERROR_FRAME, 1e-5)
TOL_G = min(TOL_FACTOR * FP32_REF_ERROR_GRAD, 1e-3)
TOL_E2E_F = min(TOL_FACTOR * FP32_REF_ERROR_E2E_FRAME, 1e-5)
TOL_E2E_G = min(TOL_FACTOR * FP32_REF_ERROR_E2E_GRAD, 1e-3)

LUT = bc.LUT


def _case(name, seed, dims, hw, enabled, weights, gamma, alpha, classes, *, seg=False, offsets="natural", **kw):
    c = bc._case(name, seed, dims, hw, enabled, weights, gamma, alpha, **kw)
    c["params"].update(showSeg=int(seg), showPred=0)
    c.update(seg=seg, classes=classes, offsets=offsets)
    del c["overlays"]
    return c


ONE = (1.0, 1.0, 1.0, 1.0)
CASES = [
    _case("c4_random", 31, (13, 9, 7), (20, 24), (1, 0, 0, 0), ONE, 1.0, 0.4, 4),
    _case("c2_seg_ones", 32, (13, 9, 7), (20, 24), (1, 1, 0, 0), (0.7, 1.6, 1.0, 1.0), 2.2, 0.4, 2, seg=True, grad="ones", ww=0.8, wl=0.45),
    _case("c9_half_zero", 33, (13, 9, 7), (20, 24), (1, 1, 1, 1), (0.5, 1.25, 0.75, 2.0), 2.2, 0.4, 9, grad="half"),
    _case("c16_dense_ert", 34, (8, 8, 8), (20, 24), (1, 0, 0, 0), ONE, 1.0, 30.0, 16),
    _case("c4_dense_ert_seg", 35, (13, 9, 7), (20, 24), (0, 1, 0, 1), (1.0, 0.6, 1.0, 1.4), 2.2, 30.0, 4, seg=True, grad="ones"),
    _case("c1_no_events", 36, (8, 8, 8), (20, 24), (1, 0, 0, 0), ONE, 1.0, 0.4, 1),
    _case("eye_inside", 37, (13, 9, 7), (20, 24), (1, 0, 0, 0), (2.0, 1.0, 1.0, 1.0), 2.2, 0.4, 4, eye=(0.1, 0.05, -0.1), target=(0.3, 0.1, 0.6), fov=1.2),
    _case("all_miss", 38, (8, 8, 8), (20, 24), (1, 0, 0, 0), ONE, 1.0, 0.4, 4, target=(5.0, 4.0, -2.1)),
    _case("near_far_clip", 39, (13, 9, 7), (20, 24), (1, 1, 0, 0), ONE, 1.0, 0.4, 9, seg=True, near=2.1, far=2.6),
    _case("orthographic", 40, (8, 8, 8), (20, 24), (1, 0, 0, 0), ONE, 2.2, 0.4, 2, ortho=0.55, grad="ones"),
    _case("one_packet", 41, (8, 8, 8), (8, 8), (1, 0, 0, 0), ONE, 1.0, 0.4, 16, seg=True),
    _case("reversed_gaps", 42, (8, 8, 8), (20, 24), (1, 0, 0, 0), ONE, 1.0, 12.0, 4, seg=True, grad="half", offsets="reversed"),
    _case("reversed_gaps_c9", 43, (13, 9, 7), (20, 24), (1, 0, 0, 0), ONE, 1.0, 0.4, 9, offsets="reversed"),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]

GUARD_ROWS = 5          # rows past the last ray's (the GPU test fills them, and the gap rows, with NaN)


@functools.lru_cache(maxsize=None)
def geo(name):
    return ref.geometry(BY_NAME[name])


@functools.lru_cache(maxsize=None)
def data(name):
    """The case's arrays (made once, shared, never modified): vols [4 x (X*Y*Z) fp32 | None], labels uint32 | None, G (H, W, 4)
    fp32, counts / offsets int64 [H*W], rows (all rows below it belong to a ray or a gap; GUARD_ROWS more follow), logits
    (rows + GUARD_ROWS, C) fp32 standard normal x 2."""
    c = BY_NAME[name]
    rng = np.random.default_rng(c["seed"])
    n = int(np.prod(c["dims"]))
    vols = [rng.uniform(-0.2, 1.2, n).astype(np.float32) if c["params"]["volEnabled"][m] else None for m in range(4)]
    labels = rng.integers(0, 9, n).astype(np.uint32) if c["seg"] else None
    H, W = c["hw"]
    G = rng.standard_normal((H, W, 4)).astype(np.float32)
    if c["grad"] == "ones":
        G[...] = 1.0
    elif c["grad"] == "half":
        G[:, W // 2:, :3] = 0.0
    counts = geo(name).counts
    offsets, rows = ref.make_offsets(counts, c["offsets"])
    logits = (2.0 * rng.standard_normal((rows + GUARD_ROWS, c["classes"]))).astype(np.float32)
    for a in vols + [labels, G, counts, offsets, logits]:
        if a is not None:
            a.setflags(write=False)
    return dict(vols=vols, labels=labels, G=G, counts=counts, offsets=offsets, rows=rows, logits=logits)


def owned_rows(name):
    """bool [rows + GUARD_ROWS]: the rows some ray owns."""
    d = data(name)
    own = np.zeros(d["rows"] + GUARD_ROWS, bool)
    for o, n in zip(d["offsets"], d["counts"]):
        own[o:o + n] = True
    return own


# --- the end-to-end composition (MLP + render): one small scene, the two networks of the issue ---------------------------------
ZMU = (0.45, 0.5, 0.55, 0.4)
ZSIGMA = (0.35, 0.4, 0.3, 0.45)
E2E_CASE = _case("e2e", 51, (8, 8, 8), (20, 24), (1, 1, 1, 1), (1.0, 0.5, 0.75, 1.25), 1.0, 3.0, 4, seg=True)
E2E_NETS = {"siren": ("siren", 30.0, [7, 32, 32, 4]), "fourier": ("fourier", 2, [19, 32, 32, 4])}


def _net_layers(kind, dims, seed, scale=1.0):
    """Deterministic start weights: the SIREN's and Glorot's uniform ranges, biases uniform +-0.1 (so that grad_b is not at a
    symmetric point)."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        lim = (np.sqrt(6.0 / a) / (30.0 if i == 0 else 1.0)) if kind == "siren" else np.sqrt(6.0 / (a + b))
        out.append({"W": (scale * rng.uniform(-lim, lim, (a, b))).astype(np.float32), "b": rng.uniform(-0.1, 0.1, b).astype(np.float32)})
    return out


@functools.lru_cache(maxsize=None)
def e2e_data():
    c = E2E_CASE
    rng = np.random.default_rng(c["seed"])
    n = int(np.prod(c["dims"]))
    vols = [rng.uniform(-0.2, 1.2, n).astype(np.float32) for _ in range(4)]
    labels = rng.integers(0, 9, n).astype(np.uint32)
    H, W = c["hw"]
    G = rng.standard_normal((H, W, 4)).astype(np.float32)
    counts = ref.geometry(c).counts
    offsets, rows = ref.make_offsets(counts, "natural")
    for a in vols + [labels, G, counts, offsets]:
        a.setflags(write=False)
    return dict(vols=vols, labels=labels, G=G, counts=counts, offsets=offsets, rows=rows, zmu=ZMU, zsigma=ZSIGMA,
                logits=np.zeros((rows, 4), np.float32))


def e2e_layers(which):
    kind, _, dims = E2E_NETS[which]
    return _net_layers(kind, dims, 61 if kind == "siren" else 62)


# --- the fit: 3 cameras, an 8 x 8 x 8 volume, 16 x 16 frames, SIREN 7 -> 2 x 32 -> 4 --------------------------------------------
FIT_STEPS = 24
FIT_CONFIG = dict(STEPS=FIT_STEPS, LR=2e-3, W0=30.0, CLIP_NORM=0.0, WEIGHT_DECAY=0.0)
FIT_EYES = [(0.9, 0.7, -2.1), (-1.4, 0.5, -1.8), (0.3, -1.2, -2.0)]
FIT_CASES = [_case(f"fit_view{i}", 70, (8, 8, 8), (16, 16), (1, 1, 1, 1), ONE, 1.0, 1.5, 4, eye=e) for i, e in enumerate(FIT_EYES)]
FIT_PERTURBATION = 0.35       # start = teacher + FIT_PERTURBATION x (another draw of the same ranges)


@functools.lru_cache(maxsize=None)
def fit_data():
    """(per view data dicts without logits / G, teacher layers, start layers)."""
    rng = np.random.default_rng(70)
    n = 512
    vols = [rng.uniform(-0.2, 1.2, n).astype(np.float32) for _ in range(4)]
    views = []
    for c in FIT_CASES:
        counts = ref.geometry(c).counts
        offsets, rows = ref.make_offsets(counts, "natural")
        views.append(dict(vols=vols, labels=None, counts=counts, offsets=offsets, rows=rows, zmu=ZMU, zsigma=ZSIGMA,
                          logits=np.zeros((rows, 4), np.float32), G=np.zeros((16, 16, 4), np.float32)))
    teacher = _net_layers("siren", [7, 32, 32, 4], 71)
    other = _net_layers("siren", [7, 32, 32, 4], 72)
    start = [{k: (t[k] + np.float32(FIT_PERTURBATION) * o[k]).astype(np.float32) for k in ("W", "b")} for t, o in zip(teacher, other)]
    return views, teacher, start


# The fp64 CPU loop's loss history (test_brats_soft_host.py::test_fit_reference_converges prints it; recorded 2026-10-19) and the
# largest relative deviation of the same loop run in float32 from it: the GPU history must follow within 8 x that.
FIT_HISTORY_FP64 = [1.044489685e-02, 3.728439328e-03, 4.763328044e-03, 3.924498186e-03, 2.834632289e-03, 2.494034451e-03,
                    2.475599975e-03, 2.346491830e-03, 2.104307488e-03, 1.861956911e-03, 1.616820470e-03, 1.351706412e-03,
                    1.109858977e-03, 9.656610021e-04, 9.468661719e-04, 9.787568491e-04, 9.580888103e-04, 8.660232081e-04,
                    7.608623093e-04, 6.974930266e-04, 6.717799157e-04, 6.455080786e-04, 6.034278157e-04, 5.616877406e-04]
FIT_FP32_DEVIATION = 2.6e-7       # measured 2.533e-07 of the largest loss; the GPU bar is 8 x it = 2.1e-6
FIT_TOL = 8.0 * FIT_FP32_DEVIATION
