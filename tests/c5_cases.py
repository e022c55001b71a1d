"""The case grid of the chunked C5 render (mrirt_render_brats_inr, csrc/brats_c5.hip).  TEST INFRASTRUCTURE ONLY.

A case is a scene (volumes, layout, camera, frame, transfer function, termination) plus a DECISIVE network: one whose argmax
is the sign of ONE input feature x_f (f in 0..6: three sample coordinates, four z-scored modalities), carried to the head
through a path that is monotone and odd, so that no rounding of the bf16 pass can change it:

  Fourier/ReLU kind  layer 0 has two live units, relu(+s x_f) at j+ and relu(-s x_f) at j-, s a power of two (the product is
                     exact in any format); later hidden layers copy them with weight 1; in the head class `a` reads j+ and
                     class `b` reads j-; every other class has zero weights and a bias of -4.  Exactly one of the two live
                     logits is positive, the other is +0.
  SIREN kind         one live unit sin(w0 s x_f) at j+ with w0 s max|x_f| <= 1, copied with weight 1 through later sine layers
                     (arguments stay inside (-pi/2, pi/2), where the sine is odd and increasing); the head gives class `a`
                     weight +1 and class `b` weight -1, the others a bias of -4.

Every other hidden unit carries seeded random finite weights that the head does not read (0 x finite = 0 exactly).  The class
is therefore `a` where x_f > 0 and `b` where x_f < 0 — rule() — provided no sample has x_f near 0, which
tests/test_c5_cases_host.py asserts for every sample of every case (min |x_f| >= 2^-20).  The frame then has an exact
reference: the oracle march with rule() as its class source (tests/c5_ref.py), no MLP and no GPU involved.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np

from mrirt import synth

W0 = 30.0
MARGIN = 2.0 ** -20

# every label 1..7 draws something, each in its own colour and opacity (the viewer's own LUT leaves 5..7 empty)
LUT = np.array([[0.0, 0.0, 0.0, 0.0], [0.0, 0.4, 1.0, 0.9], [0.0, 0.8, 0.0, 0.7], [1.0, 0.1, 0.1, 0.9], [0.9, 0.8, 0.1, 0.5],
                [0.7, 0.0, 0.9, 0.8], [0.1, 0.9, 0.9, 0.6], [1.0, 0.5, 0.0, 1.1]], dtype=np.float32)


@dataclass(frozen=True)
class Net:
    kind: str                     # "fourier" | "siren"
    hidden: int
    depth: int                    # hidden layers
    out: int
    f: int                        # the deciding input: 0..2 coordinates, 3..6 modalities
    a: int                        # class where x_f > 0
    b: int                        # class where x_f < 0
    jp: int                       # the live unit (Fourier/ReLU: of +s x_f)
    jm: int = 0                   # Fourier/ReLU: the unit of -s x_f
    s_log2: int = 0               # s = 2^s_log2
    K: int = 0                    # Fourier frequencies (their rows of layer 0 are zero everywhere)
    seed: int = 0


@dataclass(frozen=True)
class Camera:
    radius: float = 3.0
    phi_deg: float = 80.0
    theta_deg: float = 25.0
    fov_deg: float = 45.0
    shift_u: float = 0.0          # the eye moved along U (the frame slides off the box)
    ortho: Optional[float] = None  # orthoHalfHeight
    diagonal: bool = False        # eye on the extended box diagonal, `radius` from the centre


@dataclass(frozen=True)
class Case:
    name: str
    dims: Tuple[int, int, int]
    frame: Tuple[int, int]        # (width, height)
    layout: str                   # "linear" | "brick" | "vg" | "quad" | "mod4"
    labels: Optional[str]         # layout of the ground-truth grid; None: showSeg off and nothing bound
    shade: bool
    enabled: Tuple[int, int, int, int]
    weights: Tuple[float, float, float, float]
    cam: Camera
    alpha: float
    ert: Optional[float]          # None: the shader's 0.01
    net: Net
    steps: int = 40               # stepSize = box diagonal of the cube / steps
    step_size: Optional[float] = None   # ... or given outright
    variant: int = 0              # MrirtRenderExt.kernelVariant
    near: float = 0.0
    far: float = 0.0
    vol_seed: int = 1234
    bg: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    gamma: float = 1.0
    chunks: Optional[Tuple[Optional[int], ...]] = None      # None: c5_ref.chunks_of()
    refused_chunk: Optional[int] = None                     # a pass length that needs more than 1024 passes
    claims: frozenset = field(default_factory=frozenset)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def volumes(dims, seed):
    """The four modalities and the label grid (linear, x fastest) and the z-score constants of the viewer."""
    vols = tuple(synth.synth_volume(0, seed + m, phase=0.3 * m, dims=dims) for m in range(4))
    lab = synth.synth_labels(0, dims=dims)
    zmu = tuple(float(v[v != 0].mean()) for v in vols)
    zsg = tuple(float(v[v != 0].std() + 1e-6) for v in vols)
    for a in vols + (lab,):
        a.setflags(write=False)
    return vols, lab, zmu, zsg


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def camera_frame(cam: Camera, box_ext):
    """(eye, U, V, W) float32 of an orbit camera looking at the box centre (the origin)."""
    if cam.diagonal:
        eye = _unit(box_ext) * cam.radius
    else:
        ph, th = math.radians(cam.phi_deg), math.radians(cam.theta_deg)
        eye = cam.radius * np.array([math.sin(ph) * math.cos(th), math.cos(ph), math.sin(ph) * math.sin(th)])
    Wv = _unit(-eye)
    U = _unit(np.cross(Wv, [0.0, 1.0, 0.0]))
    V = np.cross(U, Wv)
    eye = eye + cam.shift_u * U
    return tuple(np.asarray(x, np.float32) for x in (eye, U, V, Wv))


def params_of(case: Case) -> Dict:
    Wd, H = case.frame
    p = synth.brats_scene(0, 0, case.steps, dims=case.dims, image_hw=(H, Wd), show_seg=case.labels is not None, show_pred=True,
                          intensity_alpha=case.alpha, fov_deg=case.cam.fov_deg)
    ext = np.asarray(p["voxelSize"], np.float64) * np.asarray(case.dims, np.float64)
    p["eye"], p["U"], p["V"], p["W"] = camera_frame(case.cam, ext)
    p["volEnabled"], p["volWeight"] = tuple(case.enabled), tuple(case.weights)
    p["nearT"], p["farT"] = float(case.near), float(case.far)
    if case.step_size is not None:
        p["stepSize"] = float(np.float32(case.step_size))
    p["bgColor"], p["gamma"] = np.asarray(case.bg, np.float32), float(case.gamma)
    p["lutColorAlpha"] = [tuple(map(float, row)) for row in LUT.tolist()]
    return p


def oracle_ext(case: Case) -> Dict:
    e = {}
    if case.cam.ortho is not None:
        e.update(cameraMode=1, orthoHalfHeight=case.cam.ortho)
    if case.shade:
        e.update(synth.SHADE_EXT)
    if case.ert is not None:
        e["ertThreshold"] = case.ert
    return e


def gpu_ext(case: Case, **more) -> Dict:
    return dict(oracle_ext(case), layout=case.layout, kernelVariant=case.variant, **more)


# ---- decisive nets ----------------------------------------------------------------------------------------------------------------
def input_row(net: Net) -> int:
    """Row of x_f in the network's input: build_input puts the Fourier features between coordinates and modalities."""
    return net.f if net.f < 3 or net.kind == "siren" else net.f + 6 * net.K


def scale(net: Net) -> float:
    return 2.0 ** net.s_log2


def layers_of(net: Net):
    """[{"W": [in][out], "b": [out]}, ...] fp32 — the list layout pack_mlp and the oracle's apply_mlp take."""
    rng = np.random.default_rng(1000 + net.seed)
    siren = net.kind == "siren"
    ind = 7 if siren else 3 + 6 * net.K + 4
    sizes = [ind] + [net.hidden] * net.depth + [net.out]
    live = (net.jp,) if siren else (net.jp, net.jm)
    assert 0 <= net.f < 7 and net.a != net.b and max(net.a, net.b) < net.out and len(set(live)) == len(live) and max(live) < net.hidden
    out = []
    for l in range(net.depth):
        fan_in, fan_out = sizes[l], sizes[l + 1]
        if siren:
            r = math.sqrt(6.0 / fan_in) / (W0 if l == 0 else 1.0)
        else:
            r = math.sqrt(6.0 / (fan_in + fan_out))
        Wm = rng.uniform(-r, r, (fan_in, fan_out)).astype(np.float32)          # junk the head never reads
        b = rng.uniform(-0.2, 0.2, fan_out).astype(np.float32)
        if l == 0 and not siren:
            Wm[3:3 + 6 * net.K] = 0.0                                          # no Fourier feature reaches any unit
        Wm[:, live] = 0.0
        b[list(live)] = 0.0
        if l == 0:
            Wm[input_row(net), net.jp] = scale(net)
            if not siren:
                Wm[input_row(net), net.jm] = -scale(net)
        else:
            for j in live:
                Wm[j, j] = 1.0
        out.append({"W": Wm, "b": b})
    Wh = np.zeros((net.hidden, net.out), np.float32)
    bh = np.full(net.out, -4.0, np.float32)
    bh[[net.a, net.b]] = 0.0
    Wh[net.jp, net.a] = 1.0
    if siren:
        Wh[net.jp, net.b] = -1.0
    else:
        Wh[net.jm, net.b] = 1.0
    out.append({"W": Wh, "b": bh})
    assert all(np.isfinite(l["W"]).all() and np.isfinite(l["b"]).all() for l in out)
    return out


def siren_dict(layers):
    return {f"l{i}": {"w": l["W"], "b": l["b"]} for i, l in enumerate(layers)}


def feature(net: Net, coords, feats):
    return np.concatenate([coords, feats], axis=-1)[:, net.f]


def rule(net: Net, coords, feats):
    """The class of a sample with MLP inputs (coords, feats): `a` where x_f > 0, `b` where x_f < 0."""
    return np.where(feature(net, coords, feats) > 0, net.a, net.b).astype(np.int64)


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
BIG, MID, SMALL = (24, 20, 18), (13, 11, 10), (9, 8, 7)
DRIFT_STEP = float(np.float32(20.4 * 2.0 ** -14))       # 20.4 ulps of t in [512, 1024): every t += stepSize rounds to 20 ulps
OUTSIDE = Camera()


def _cases():
    c = [
        # the existing test's scene, shaded on the plain ABI, every modality drawn with its own weight
        Case("linear_shaded_56x40", BIG, (56, 40), "linear", "linear", True, (1, 1, 1, 1), (1.0, 0.5, 0.25, 2.0), OUTSIDE, 6.0, None,
             Net("fourier", 64, 4, 4, f=0, a=1, b=2, jp=0, jm=63, s_log2=1, seed=1), steps=48,
             claims=frozenset({"early", "ert_boundary", "both_classes", "multiple", "last_pass_empty"})),
        # eye inside the box: every ray marches from t = 0, so chunk 1 fills the first batch to exactly cap = 37 * 29 rows
        Case("brick_inside_37x29", BIG, (37, 29), "brick", "brick", True, (0, 1, 0, 1), (0.7, 1.3, 0.2, 0.6), Camera(radius=0.25), 40.0, None,
             Net("siren", 64, 2, 4, f=4, a=3, b=0, jp=63, s_log2=-8, seed=2), variant=2,
             claims=frozenset({"all_hit", "early", "ert_boundary", "both_classes", "multiple"})),
        # the 4 x 256 SIREN: the weight-stationary kernel behind a device-side count (and, with the flag, the streaming one)
        Case("vg_ert05_9x9", MID, (9, 9), "vg", None, True, (1, 1, 1, 1), (0.3, 0.2, 0.4, 0.1), OUTSIDE, 6.0, 0.5,
             Net("siren", 256, 4, 4, f=1, a=2, b=3, jp=255, s_log2=-8, seed=3), bg=(0.05, 0.1, 0.15), gamma=2.2,
             claims=frozenset({"early", "ert_boundary", "both_classes", "multiple", "last_pass_empty"})),
        # no modality drawn: the overlays alone composite
        Case("quad_overlays_8x8", SMALL, (8, 8), "quad", "brick", False, (0, 0, 0, 0), (1.0, 2.0, 3.0, 4.0), Camera(radius=2.5), 6.0, None,
             Net("fourier", 64, 4, 4, f=5, a=0, b=2, jp=5, jm=40, s_log2=-2, K=1, seed=4), variant=2,
             claims=frozenset({"none_terminate", "both_classes", "multiple"})),
        # one row of 64 pixels sliding off the box: some rays miss
        Case("mod4_partial_64x1", BIG, (64, 1), "mod4", "linear", False, (0, 1, 0, 1), (0.25, 0.75, 0.5, 1.5), Camera(fov_deg=1.0, shift_u=0.5), 0.4, -1.0,
             Net("fourier", 64, 4, 4, f=6, a=2, b=1, jp=63, jm=0, s_log2=0, seed=5), bg=(0.1, 0.2, 0.3),
             claims=frozenset({"miss_some", "none_terminate", "both_classes", "multiple"})),
        # a frame that misses the box altogether
        Case("linear_miss_8x8", SMALL, (8, 8), "linear", None, False, (1, 1, 1, 1), (1.0, 1.0, 2.0, 0.5), Camera(shift_u=6.0), 6.0, None,
             Net("siren", 64, 2, 4, f=2, a=1, b=3, jp=17, s_log2=-8, seed=6), bg=(0.25, 0.5, 0.125), claims=frozenset({"miss_all"})),
        # nearT / farT cut a slab out of the middle; both variant bits
        Case("brick_slab_9x9", MID, (9, 9), "brick", "linear", False, (1, 1, 1, 1), (2.0, 1.0, 0.5, 0.25), OUTSIDE, 6.0, -1.0,
             Net("fourier", 64, 4, 4, f=3, a=1, b=3, jp=31, jm=32, s_log2=3, seed=7), variant=3, near=2.7, far=3.2, gamma=0.7,
             claims=frozenset({"clipped", "none_terminate", "both_classes", "multiple"})),
        # orthographic 7:1, dense; eight outputs: classes 4..7 are drawn
        Case("quad_ortho_56x8", BIG, (56, 8), "quad", "brick", False, (1, 1, 1, 1), (1.0, 0.5, 2.0, 0.25), Camera(ortho=0.3), 40.0, None,
             Net("siren", 64, 2, 8, f=4, a=5, b=7, jp=0, s_log2=-8, seed=8), variant=2, bg=(0.3, 0.0, 0.6),
             claims=frozenset({"miss_some", "early", "ert_boundary", "both_classes", "multiple"})),
        # orthographic 1:7; sixteen outputs, both classes >= 8: the prediction overlay draws nothing
        Case("mod4_ortho_5x35", BIG, (5, 35), "mod4", None, False, (1, 1, 1, 1), (0.5, 0.25, 0.125, 1.0), Camera(ortho=1.0), 6.0, 0.5,
             Net("fourier", 64, 4, 16, f=1, a=9, b=12, jp=40, jm=5, s_log2=2, seed=9),
             claims=frozenset({"early", "multiple"})),
        # one pixel; sixteen outputs, one class of the pair drawn
        Case("vg_1x1", SMALL, (1, 1), "vg", "brick", True, (0, 1, 0, 1), (1.0, 0.5, 1.0, 2.0), Camera(radius=2.5), 6.0, None,
             Net("fourier", 64, 4, 16, f=0, a=3, b=11, jp=63, jm=31, s_log2=-1, seed=10), claims=frozenset({"multiple"})),
        # fp32 drift of the running sum t += stepSize: the eye far out on the box diagonal, ulp(t) = 2^-14 ~ stepSize / 20.4
        Case("linear_drift_8x8", SMALL, (8, 8), "linear", None, False, (1, 1, 1, 1), (1.0, 1.0, 1.0, 1.0),
             Camera(radius=600.0, fov_deg=7.6e-4, diagonal=True), 0.05, -1.0,
             Net("siren", 64, 2, 4, f=3, a=1, b=2, jp=33, s_log2=-8, seed=11), step_size=DRIFT_STEP, chunks=(8,), refused_chunk=2,
             claims=frozenset({"drift", "none_terminate", "both_classes"})),
    ]
    return {k.name: k for k in c}


CASES = _cases()
NAMES = tuple(CASES)
FAST_CASES = ("linear_shaded_56x40", "brick_inside_37x29", "vg_ert05_9x9", "quad_ortho_56x8", "mod4_partial_64x1")   # one per layout
RAW_ABI_CASES = ("brick_inside_37x29", "vg_1x1", "quad_overlays_8x8", "mod4_ortho_5x35")                            # one per layout family
