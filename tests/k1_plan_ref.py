"""The K1 launch plan restated in Python, the grid of configurations that reaches every march kernel it can choose, and the tiny
scene those configurations are rendered on.  TEST INFRASTRUCTURE ONLY.

``plan()`` follows ``plan_k1()`` + ``layout_kernel()`` / ``pipe_kernel()`` / ``roll_kernel()`` of csrc/brats_march.hip branch by
branch, for launches of the size the tests use: grids far below 4 GiB, no class stream, no LDS kernel asked for, a rank that
owns pixels.  It maps a configuration to a kernel IDENTITY, the template instantiation the launch runs:

    ("generic", STRICT, LAYOUT, SHADE)
    ("pipe",    STRICT, LAYOUT, SHADE, NCH, GAMMA1, LABELS, SKIP, CELLS, TAG)
    ("roll",    STRICT, LAYOUT, SHADE, NCH, GAMMA1, LABELS, SKIP)

with LAYOUT as in include/mrirt.h.  ``library_kernels()`` reads the same identities out of the built library's code objects,
so a test can demand that the two sets are equal (tests/test_k1_plan_host.py).
"""
from __future__ import annotations

import itertools
import math
import pathlib
import re
import subprocess
import tempfile
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent

# include/mrirt.h: MRIRT_LAYOUT_*
LAYOUT_CODE = {"linear": 0, "brick": 1, "vg": 2, "quad": 3, "vga": 4, "mod4": 6}
LAYOUT_NAME = {v: k for k, v in LAYOUT_CODE.items()}

# kernelVariant bits (csrc/brats_march.hip, above prepare())
VARIANT_FLIP_WORKGROUP = 2       # bit 1: 16 x 16 instead of 8 x 8 workgroups (on launches of this size)
VARIANT_NO_PIPE = 4              # bit 2: the generic kernel, no skipping
VARIANT_COUNT_UNFETCHED = 128    # bit 7: stats[1] also counts the samples a skipping kernel did NOT fetch
VARIANT_TAG = 32768              # bit 15: the tagged twin of the benched kernel


class Config(NamedTuple):
    math: str                    # "strict" | "fast"
    layout: str                  # of the intensity grids
    shade: bool
    mods: Tuple[int, ...]        # the enabled modalities
    gamma: float
    overlays: str                # "none" | "seg" | "seg+pred"
    cells: bool                  # labels bound as a label-cell grid (QUAD / MOD4 only)
    skip: bool                   # a skip map is offered (render_brats(..., skip=True))
    nopipe: bool                 # kernelVariant bit 2
    tag: bool = False            # kernelVariant bit 15


class Plan(NamedTuple):
    family: str                  # as render.kernel_family reports it
    skipping: bool
    label_cells: bool
    kernel: Tuple                # the identity


REFUSED = "MRIRT_ERR_LAYOUT"


def plan(c: Config):
    """The Plan of a configuration, or REFUSED where the render call returns MRIRT_ERR_LAYOUT."""
    strict = c.math == "strict"
    lay = LAYOUT_CODE[c.layout]
    nch = len(c.mods)
    overlays = c.overlays != "none"
    # prepare(): cfg.pipe
    pipe = nch >= 1 and not c.nopipe
    # plan_k1(): the family
    family = "generic"
    if c.layout in ("vg", "vga"):
        if pipe and nch == 1:
            family = "pipelined"
        elif pipe and not overlays:
            family = "rolling"
    elif c.layout == "linear":
        if pipe and not c.shade:
            family = "pipelined"
    elif c.layout == "quad":
        if c.shade:
            return REFUSED
        if pipe:
            family = "pipelined"
    elif c.layout == "mod4":
        if c.shade:
            return REFUSED
        family = "pipelined"                     # whatever is enabled, and whatever bit 2 says
        nch = 4
    gamma1 = strict and c.gamma == 1.0
    skip_kernel = (family == "pipelined" and c.layout != "linear") or family == "rolling"
    # (the offered map is sound on this scene: positive window width, gamma and weights, a summary for every bound grid)
    skipping = c.skip and pipe and skip_kernel and (not strict or c.gamma == 1.0)
    cells = family == "pipelined" and c.cells and overlays and not skipping
    labels = (overlays or not gamma1) and not (family == "rolling" and skipping)
    tag = c.tag and family == "pipelined" and c.layout == "vga" and c.shade and len(c.mods) == 1 and gamma1 and not labels and not skipping
    # layout_kernel()
    if c.layout in ("vg", "vga") and family == "pipelined":
        kernel = _pipe_kernel(strict, lay, c.shade, 1, gamma1, labels, skipping, cells, tag)
    elif c.layout in ("vg", "vga") and family == "rolling":
        kernel = _roll_kernel(strict, lay, c.shade, nch if nch in (2, 3) else 4, gamma1, skipping)
    elif c.layout in ("linear", "quad") and not c.shade and family == "pipelined":
        kernel = _pipe_kernel(strict, lay, c.shade, nch if nch in (1, 2, 3) else 4, gamma1, labels, skipping, cells, tag)
    elif c.layout == "mod4":
        kernel = _pipe_kernel(strict, lay, c.shade, 4, gamma1, labels, skipping, cells, tag)
    else:
        kernel = ("generic", strict, lay, c.shade)
    return Plan(family, skipping, cells, kernel)


def _pipe_kernel(strict, lay, shade, nch, gamma1, labels, skipping, cells, tag):
    """pipe_kernel<STRICT, LAYOUT, SHADE, NCH>(pl): the template arguments after NCH are GAMMA1, LABELS, SKIP, CELLS, TAG."""
    head = ("pipe", strict, lay, shade, nch)
    if lay in (LAYOUT_CODE["quad"], LAYOUT_CODE["mod4"]) and cells:
        return head + ((strict if gamma1 else False), True, False, True, False)
    if lay != LAYOUT_CODE["linear"] and skipping:
        if not gamma1:
            return head + (False, True, not strict, False, False)
        return head + ((strict, True, True, False, False) if labels else (strict, not strict, True, False, False))
    if strict and lay == LAYOUT_CODE["vga"] and shade and nch == 1 and tag:
        return head + (strict, not strict, False, False, True)
    if not gamma1:
        return head + (False, True, False, False, False)
    return head + ((strict, True, False, False, False) if labels else (strict, not strict, False, False, False))


def _roll_kernel(strict, lay, shade, nch, gamma1, skipping):
    """roll_kernel<STRICT, LAYOUT, SHADE, NCH>(pl): GAMMA1, LABELS, SKIP."""
    head = ("roll", strict, lay, shade, nch)
    if skipping:
        return head + (strict, False, True)
    return head + ((strict, not strict, False) if gamma1 else (False, True, False))


def kernel_id(k: Tuple) -> str:
    """A readable pytest id: pipe-S-vga-sh-n1-g1-L0-K0-C0-T0."""
    kind, strict, lay, shade = k[:4]
    s = f"{kind}-{'S' if strict else 'F'}-{LAYOUT_NAME[lay]}-{'sh' if shade else 'un'}"
    if kind == "generic":
        return s
    s += f"-n{k[4]}-g{int(k[5])}-L{int(k[6])}-K{int(k[7])}"
    if kind == "pipe":
        s += f"-C{int(k[8])}-T{int(k[9])}"
    return s


# ----------------------------------------------------------------------------------------------------------------------
# the case grid
# ----------------------------------------------------------------------------------------------------------------------
MATHS = ("strict", "fast")
LAYOUTS = ("linear", "brick", "vg", "quad", "vga", "mod4")
MODS = ((), (2,), (0, 3), (1, 2, 3), (0, 1, 2, 3))         # deliberately no prefixes: K1Args::chan[] is not 0, 1, 2, ...
GAMMA_NOT_1 = 0.6
GAMMAS = (1.0, GAMMA_NOT_1)
OVERLAYS = ("none", "seg", "seg+pred")
WEIGHTS = (0.7, 1.3, 0.45, 1.9)                            # distinct, none of them 1


def grid() -> List[Config]:
    """Every combination of the axes that can be bound: label cells go with QUAD / MOD4 grids and need an overlay to show
    (without one no label grid is bound at all).  Shaded QUAD / MOD4 stay in: the plan refuses them."""
    out = []
    for m, lay, sh, mods, g, ov, cells, skip, nopipe in itertools.product(MATHS, LAYOUTS, (False, True), MODS, GAMMAS, OVERLAYS,
                                                                          (False, True), (False, True), (False, True)):
        if cells and (lay not in ("quad", "mod4") or ov == "none"):
            continue
        out.append(Config(m, lay, sh, mods, g, ov, cells, skip, nopipe))
    return out


TAG_CONFIG = Config("strict", "vga", True, (2,), 1.0, "none", False, False, False, tag=True)


def cases_by_kernel() -> Dict[Tuple, List[Config]]:
    """{kernel identity: the grid configurations that launch it}, refusals left out."""
    by = {}
    for c in grid():
        pl = plan(c)
        if pl != REFUSED:
            by.setdefault(pl.kernel, []).append(c)
    return by


# ----------------------------------------------------------------------------------------------------------------------
# the built library's kernels
# ----------------------------------------------------------------------------------------------------------------------
_MANGLED = re.compile(r"^_ZN5mrirt\d+brats_march(_pipe|_roll|)_kernelI((?:L[bi]\d+E)+)E")


def parse_kernel_name(name: str) -> Optional[Tuple]:
    """The identity of an Itanium-mangled march kernel name (template arguments: a run of Lb0E / Lb1E / Li<n>E), else None."""
    m = _MANGLED.match(name)
    if not m:
        return None
    args = tuple(bool(int(v)) if t == "b" else int(v) for t, v in re.findall(r"L([bi])(\d+)E", m.group(2)))
    kind = {"": "generic", "_pipe": "pipe", "_roll": "roll"}[m.group(1)]
    want = {"generic": 3, "pipe": 9, "roll": 7}[kind]
    if len(args) != want:
        raise ValueError(f"{name}: {len(args)} template arguments, the {kind} kernel has {want}")
    return (kind,) + args


def library_kernels(so: pathlib.Path) -> List[Tuple]:
    """The identities of every brats_march_kernel / _pipe_kernel / _roll_kernel in the library's gfx950 code objects, from
    the amdhsa.kernels metadata notes (as tools/compare_code_objects.py reads its figures)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_async_loads", ROOT / "tools" / "check_async_loads.py")
    cal = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cal)
    out = []
    with tempfile.TemporaryDirectory() as td:
        for co in cal.code_objects(so, pathlib.Path(td)):
            notes = subprocess.run([str(cal.llvm_bin() / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
            for name in re.findall(r"^\s+\.name:\s+(\S+)$", notes, re.M):
                k = parse_kernel_name(name)
                if k is not None:
                    out.append(k)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the scene
# ----------------------------------------------------------------------------------------------------------------------
DIMS = (40, 34, 27)              # odd and unequal: padded bricks, partial macro cells (5 x 5 x 4 of them)
IMAGE_WH = (40, 28)              # a multiple of neither 8 nor 16
STEPS = 60
WL, WW = 0.45, 0.7               # window floor 0.1 above the air's 0
_CENTRE = (20.0, 17.0, 16.0)     # of the blob, in voxels
_RADII = (11.5, 8.5, 7.0)       # modality 0's: inside macro cells 1..3 x 1..3 x 1..2, their overlap planes included


def scene() -> Dict[str, Any]:
    """Four blob-in-air modalities (texture inside zeros, the blob a little smaller from one modality to the next), a ground
    truth grid with one label blob in the tissue and one in the air, and a prediction grid with other labels elsewhere."""
    X, Y, Z = DIMS
    rng = np.random.default_rng(5)
    z, y, x = np.meshgrid(np.arange(Z, dtype=np.float32), np.arange(Y, dtype=np.float32), np.arange(X, dtype=np.float32), indexing="ij")
    u, v, w = (x - _CENTRE[0]) / _RADII[0], (y - _CENTRE[1]) / _RADII[1], (z - _CENTRE[2]) / _RADII[2]
    r = np.sqrt(u * u + v * v + w * w)
    vols = []
    for c in range(4):
        t = np.clip(1.25 - r, 0, None) * (0.75 + 0.2 * np.sin((3 + c) * u + 0.4 * c) * np.cos(4 * v)) + 0.04 * rng.random((Z, Y, X), dtype=np.float32)
        t[r > 1.0 - 0.04 * c] = 0.0
        vols.append(np.ascontiguousarray(np.clip(t, 0, 1).astype(np.float32)).reshape(-1))
    lab = np.zeros((Z, Y, X), np.uint32)
    lab[r < 0.4] = 3
    lab[(np.abs(x - 35) <= 2) & (np.abs(y - 4) <= 2) & (np.abs(z - 22) <= 1)] = 2          # in the air
    prd = np.zeros((Z, Y, X), np.uint32)
    prd[(r < 0.7) & (u > 0.1)] = 1
    prd[(np.abs(x - 5) <= 1) & (np.abs(y - 28) <= 2) & (np.abs(z - 4) <= 2)] = 4           # in the air, elsewhere
    return dict(dims=DIMS, vols=vols, lab=lab.reshape(-1), prd=prd.reshape(-1))


def step_size() -> float:
    return float(np.float32(1.8 * math.sqrt(3.0) / STEPS))


# intensityAlpha on both sides of the kernels' run-time exp switch: |intensityAlpha * stepSize| <= 1/8 takes the short
# polynomial (K1Args::expSmall)
EXP_RANGES = {"small": float(np.float32(0.1249 / step_size())), "large": 16.0}


def exp_small(intensity_alpha: float) -> bool:
    """prepare(): a.expSmall, in fp32."""
    return bool(np.abs(np.float32(intensity_alpha) * np.float32(step_size())) <= np.float32(0.125))


def params(c: Config, exp_range: str) -> Dict[str, Any]:
    """gParams of a configuration: an oblique perspective camera outside the box."""
    from mrirt import OrbitalCamera, synth
    cam = OrbitalCamera(initial_radius=1.75, initial_phi=np.radians(62), initial_theta=np.radians(-38))
    p = synth.brats_scene(0, 0, STEPS, dims=DIMS, image_hw=(IMAGE_WH[1], IMAGE_WH[0]), camera=cam, fov_deg=32.0, intensity_alpha=EXP_RANGES[exp_range],
                          show_seg=c.overlays != "none", show_pred=c.overlays == "seg+pred")
    p["volEnabled"] = tuple(np.uint32(1 if m in c.mods else 0) for m in range(4))
    p["volWeight"] = tuple(np.float32(w) for w in WEIGHTS)
    p["wl"], p["ww"], p["gamma"] = np.float32(WL), np.float32(WW), np.float32(c.gamma)
    return p


def shade_ext(c: Config) -> Dict[str, Any]:
    from mrirt import synth
    return dict(synth.SHADE_EXT) if c.shade else {}


def reference_key(c: Config, exp_range: str) -> Tuple:
    """What the oracle's frame depends on: neither the layout, nor how labels are bound, nor the kernel taken."""
    return (c.shade, c.mods, c.gamma, c.overlays, exp_range)


_REFS: Dict[Tuple, Any] = {}
_SCENE: Optional[Dict[str, Any]] = None


def shared_scene() -> Dict[str, Any]:
    global _SCENE
    if _SCENE is None:
        _SCENE = scene()
    return _SCENE


def reference(c: Config, exp_range: str):
    """(frame, aux) of the oracle for a configuration, computed once per process: oracle_c (bit-faithful) for STRICT,
    oracle_np (which also flags knife-edge pixels) for FAST."""
    key = (c.math,) + reference_key(c, exp_range)
    if key not in _REFS:
        from oracle import oracle_c, oracle_np
        s = shared_scene()
        o = oracle_c if c.math == "strict" else oracle_np
        ref, aux = o.brats_main(params(c, exp_range), s["vols"], s["lab"], s["prd"], shade_ext(c), return_aux=True)
        ref.setflags(write=False)
        _REFS[key] = (ref, aux)
    return _REFS[key]


def skippable_fraction(c: Config) -> float:
    """The fraction of macro cells the skip mask of a configuration flags as empty, from tests/grid_ref.py's restatement."""
    import grid_ref
    s = shared_scene()
    en = [1 if m in c.mods else 0 for m in range(4)]
    ubs = [grid_ref.macro_max_ref(s["vols"][m], DIMS) for m in c.mods]
    seg = grid_ref.macro_labels_ref(s["lab"], DIMS) if c.overlays != "none" else None
    prd = grid_ref.macro_labels_ref(s["prd"], DIMS) if c.overlays == "seg+pred" else None
    empty = grid_ref.skip_mask_ref(ubs, [WEIGHTS[m] for m in c.mods], grid_ref.weight_sum(en, WEIGHTS), grid_ref.window_floor(WL, WW), seg, prd)
    return float(np.mean(empty))
