"""Scenes of the K1 backward tests (test_brats_grad_host.py, test_brats_grad_sanitizers.py, test_gpu_brats_grad.py): the smallest
shapes at which the backward kernel can go wrong.  TEST INFRASTRUCTURE ONLY.

Volumes of 13 x 9 x 7 and 8 x 8 x 8 voxels with values in [-0.2, 1.2] (both saturation ends of the window occur), frames of
24 x 20 (partial 8 x 8 packets) and 8 x 8, at most 48 steps per ray, 1 / 2 / 4 modalities with unequal weights, a modality
disabled in the middle, gamma 1 and 2.2, intensityAlpha 0.4 (no early termination) and 30 (part of the rays terminate early),
both overlays with labels 0..8, the eye inside the box, a frame that misses the box, nearT / farT clipping, the orthographic
camera; G random normal, all ones, zero on half the image.

Seeds are chosen on the CPU (test_brats_grad_host.py::test_decisions_have_margin) so that no sample sits on a knife edge where
fp32 and fp64 would decide differently; a case that needs another seed gets one here, no sample is ever excluded.
"""
import functools

import numpy as np

# Tolerance of the GPU comparison, |g - g_ref| <= TOL * A (A = sum of the absolute per-sample contributions).
# Measured on the CPU on 2026-10-18 (test_brats_grad_host.py::test_fp32_reference_error prints it): the largest
# |g_fp32,shuffled - g_fp64| / A of the reference's own fp32 evaluation over all cases and five shuffles is FP32_REF_ERROR;
# TOL = 8 x that (the kernel's atomics sum in an order nobody controls and more rays meet in a voxel than one shuffle shows),
# capped at 1e-3 (one wrong corner weight or a dropped term errs by >= 1e-2 A).  Never derived from the kernel's output.
FP32_REF_ERROR = 4.8e-4     # measured 4.795e-04 (case eye_inside); 8 x it is 3.8e-3, so the cap of 1e-3 is what holds
TOL_FACTOR = 8.0
TOL = min(TOL_FACTOR * FP32_REF_ERROR, 1e-3)

LUT = np.array([[0.0, 0.0, 0.0, 0.0], [1.0, 0.2, 0.1, 2.0], [0.2, 0.9, 0.3, 4.0], [0.1, 0.3, 1.0, 6.0],
                [0.9, 0.8, 0.1, 3.0], [0.7, 0.1, 0.8, 5.0], [0.2, 0.8, 0.8, 1.0], [0.6, 0.6, 0.6, 7.0]], dtype=np.float32)


def _look_at(eye, target):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    W = target - eye
    W /= np.linalg.norm(W)
    up = np.array([0.0, 1.0, 0.0]) if abs(W[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    U = np.cross(W, up)
    U /= np.linalg.norm(U)
    V = np.cross(U, W)
    return [eye.astype(np.float32), U.astype(np.float32), V.astype(np.float32), W.astype(np.float32)]


def _case(name, seed, dims, hw, enabled, weights, gamma, alpha, *, eye=(0.9, 0.7, -2.1), target=None, ww=1.0, wl=0.5,
          overlays=False, near=0.0, far=0.0, ortho=None, grad="normal", step=0.04, fov=0.5, ert=None):
    dims = tuple(dims)
    vox = np.float32(1.0 / max(dims))
    vol_min = np.array([-0.5 * vox * d for d in dims], dtype=np.float32)
    eye_, U, V, W = _look_at(eye, (0.02, -0.03, 0.01) if target is None else target)
    params = dict(imageSize=[hw[1], hw[0]], fovY=fov, eye=eye_, U=U, V=V, W=W, volMin=vol_min, voxelSize=[vox] * 3, dims=list(dims),
                  stepSize=step, nearT=near, farT=far, bgColor=[0.05, 0.1, 0.15], volEnabled=list(enabled), volWeight=list(weights),
                  ww=ww, wl=wl, intensityAlpha=alpha, gamma=gamma, showSeg=int(overlays), showPred=int(overlays), lutColorAlpha=LUT)
    ext = {}
    if ortho is not None:
        ext.update(cameraMode=1, orthoHalfHeight=ortho)
    if ert is not None:
        ext.update(ertThreshold=ert)
    return dict(name=name, seed=seed, params=params, ext=ext, overlays=overlays, grad=grad, hw=tuple(hw), dims=dims)


CASES = [
    _case("one_modality", 11, (13, 9, 7), (20, 24), (1, 0, 0, 0), (1.0, 1.0, 1.0, 1.0), 1.0, 0.4),
    _case("two_modalities_gamma", 12, (13, 9, 7), (20, 24), (1, 1, 0, 0), (0.7, 1.6, 1.0, 1.0), 2.2, 0.4, grad="ones", ww=0.8, wl=0.45),
    _case("four_modalities_half_zero", 13, (13, 9, 7), (20, 24), (1, 1, 1, 1), (0.5, 1.25, 0.75, 2.0), 2.2, 0.4, grad="half"),
    _case("middle_disabled", 14, (8, 8, 8), (20, 24), (1, 0, 1, 1), (1.5, 9.0, 0.5, 1.0), 1.0, 0.4, ww=1.1, wl=0.5),
    _case("dense_ert", 15, (8, 8, 8), (20, 24), (1, 0, 0, 0), (1.0, 1.0, 1.0, 1.0), 1.0, 30.0),
    _case("dense_ert_gamma_two", 116, (13, 9, 7), (20, 24), (0, 1, 0, 1), (1.0, 0.6, 1.0, 1.4), 2.2, 30.0, grad="ones"),
    _case("overlays", 17, (13, 9, 7), (20, 24), (1, 1, 0, 0), (1.0, 0.5, 1.0, 1.0), 2.2, 0.4, overlays=True),
    _case("overlays_dense", 18, (8, 8, 8), (20, 24), (1, 0, 0, 0), (1.0, 1.0, 1.0, 1.0), 1.0, 12.0, overlays=True, grad="half"),
    _case("eye_inside", 19, (13, 9, 7), (20, 24), (1, 0, 0, 0), (2.0, 1.0, 1.0, 1.0), 2.2, 0.4, eye=(0.1, 0.05, -0.1), target=(0.3, 0.1, 0.6), fov=1.2),
    _case("all_miss", 20, (8, 8, 8), (20, 24), (1, 0, 0, 0), (1.0, 1.0, 1.0, 1.0), 1.0, 0.4, target=(5.0, 4.0, -2.1)),
    _case("near_far_clip", 21, (13, 9, 7), (20, 24), (1, 1, 0, 0), (1.0, 1.0, 1.0, 1.0), 1.0, 0.4, near=2.1, far=2.6),
    _case("orthographic", 22, (8, 8, 8), (20, 24), (1, 0, 0, 0), (1.0, 1.0, 1.0, 1.0), 2.2, 0.4, ortho=0.55, grad="ones"),
    _case("one_packet", 23, (8, 8, 8), (8, 8), (1, 0, 0, 0), (1.0, 1.0, 1.0, 1.0), 1.0, 0.4),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def data(name):
    """The case's arrays (made once, shared, never modified): vols [4 x (X*Y*Z) fp32 | None], labels / preds uint32 | None, G (H, W, 4) fp32."""
    c = BY_NAME[name]
    rng = np.random.default_rng(c["seed"])
    n = int(np.prod(c["dims"]))
    vols = [rng.uniform(-0.2, 1.2, n).astype(np.float32) if c["params"]["volEnabled"][m] else None for m in range(4)]
    labels = rng.integers(0, 9, n).astype(np.uint32) if c["overlays"] else None
    preds = rng.integers(0, 9, n).astype(np.uint32) if c["overlays"] else None
    H, W = c["hw"]
    G = rng.standard_normal((H, W, 4)).astype(np.float32)
    if c["grad"] == "ones":
        G[...] = 1.0
    elif c["grad"] == "half":
        G[:, W // 2:, :3] = 0.0
    for a in vols + [labels, preds, G]:
        if a is not None:
            a.setflags(write=False)
    return dict(vols=vols, labels=labels, preds=preds, G=G)
