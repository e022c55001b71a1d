"""ctypes binding of libmrirt.so (the C ABI declared in include/mrirt.h).

The HIP library is the product: there is NO CPU fallback.  If the shared object is missing or
stale, :func:`lib` raises — render calls never silently route anywhere else.
"""
from __future__ import annotations

import ctypes as C
import os
import pathlib
import subprocess
import sys
from typing import List, Optional

PKG_DIR = pathlib.Path(__file__).resolve().parent
CSRC = PKG_DIR / "csrc"
INCLUDE = PKG_DIR.parent / "include"
SO_PATH = pathlib.Path(os.environ.get("MRIRT_LIB", PKG_DIR / "libmrirt.so"))   # override: A/B builds in development
HIP_SOURCES = ["brats_march.hip", "brats_order.hip", "brats_skip.hip", "brats_c5.hip", "brats_slab.hip", "brats_ring.hip", "brats_backward.hip", "brats_soft.hip", "brats_tf.hip", "volume_march.hip", "grid_ops.hip", "inr_mlp.hip",
               "inr_stream.hip", "inr_ws.hip", "inr_refine.hip", "inr_train.hip", "inr_optim.hip", "inr_muon.hip", "inr_lossx.hip", "inr_inject.hip", "inr_inject_fused.hip", "inr_inject_train.hip", "inr_unified.hip", "inr_hybrid.hip", "mesh_rt.hip", "edt.hip", "surface.hip", "prep.hip", "components.hip", "abort_trace.cpp"]
HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-Wall"]

# every extern "C" symbol include/mrirt.h declares
ABI_SYMBOLS = [
    "mrirt_render_brats", "mrirt_render_brats_ex", "mrirt_brats_sample_counts", "mrirt_brats_emit_samples",
    "mrirt_render_brats_stream", "mrirt_brats_inr_scratch_bytes", "mrirt_render_brats_inr", "mrirt_brick_elems", "mrirt_brick_grid",
    "mrirt_unbrick_grid", "mrirt_vec4_elems", "mrirt_vga_elems", "mrirt_build_vec4_grid", "mrirt_build_label_cells", "mrirt_build_mod4_grid", "mrirt_bc4_decode", "mrirt_macro_cells", "mrirt_skip_mask_words",
    "mrirt_build_macro_max", "mrirt_build_macro_labels", "mrirt_render_brats_skip", "mrirt_render_volume", "mrirt_build_cell8", "mrirt_render_sdf", "mrirt_render_mesh", "mrirt_tiles_for_rank",
    "mrirt_detile", "mrirt_inr_pack_bytes", "mrirt_inr_pack_weights", "mrirt_inr_calibrate", "mrirt_inr_forward", "mrirt_inr_forward_refined",
    "mrirt_inr_predict_volume", "mrirt_abi_version", "mrirt_status_string", "mrirt_last_hip_error",
    "mrirt_sizeof", "mrirt_brats_skip_applicable", "mrirt_brats_kernel_family", "mrirt_install_abort_trace",
    "mrirt_edt_scratch_bytes", "mrirt_edt_squared", "mrirt_hausdorff",
    "mrirt_surface_scratch_bytes", "mrirt_surface_count", "mrirt_surface_extract",
    "mrirt_render_brats_backward", "mrirt_render_brats_soft", "mrirt_render_brats_soft_backward",
    "mrirt_inr_train_scratch_bytes", "mrirt_inr_loss_scratch_bytes", "mrirt_inr_forward_f32", "mrirt_inr_loss", "mrirt_inr_backward",
    "mrirt_inr_sample_batch", "mrirt_inr_adamw_scratch_bytes", "mrirt_inr_adamw_step", "mrirt_inr_lr_schedule",
    "mrirt_inr_train_run_scratch_bytes", "mrirt_inr_train_run",
    "mrirt_siren_train_scratch_bytes", "mrirt_siren_forward_f32", "mrirt_siren_backward",
    "mrirt_siren_train_run_scratch_bytes", "mrirt_siren_train_run",
    "mrirt_muon_scratch_bytes", "mrirt_muon_orthogonalize", "mrirt_muon_step",
    "mrirt_inr_train_run_muon_scratch_bytes", "mrirt_inr_train_run_muon",
    "mrirt_inr_loss_ext_scratch_bytes", "mrirt_inr_loss_ext", "mrirt_inr_tumour_count", "mrirt_inr_tumour_index_scratch_bytes",
    "mrirt_inr_tumour_index", "mrirt_inr_sample_batch_mix", "mrirt_inr_train_run_ext_scratch_bytes", "mrirt_inr_train_run_ext",
    "mrirt_order_words", "mrirt_render_brats_ordered", "mrirt_brats_order_applicable", "mrirt_order_build_host",
    "mrirt_prep_scratch_bytes", "mrirt_prep_window", "mrirt_prep_normalize", "mrirt_prep_zscore_scratch_bytes",
    "mrirt_prep_zscore_stats", "mrirt_prep_zscore_apply", "mrirt_prep_gaussian3d",
    "mrirt_cc_scratch_bytes", "mrirt_cc_label", "mrirt_cc_sizes", "mrirt_cc_filter", "mrirt_slice_counts",
    "mrirt_render_brats_tf",
    "mrirt_inject_scratch_bytes", "mrirt_inject_forward", "mrirt_inject_uncertainty", "mrirt_inject_predict_volume",
    "mrirt_boundary_weights_scratch_bytes", "mrirt_boundary_weights",
    "mrirt_inject_train_scratch_bytes", "mrirt_inject_forward_train", "mrirt_inject_backward",
    "mrirt_unified_loss_scratch_bytes", "mrirt_unified_loss", "mrirt_inr_sample_field",
    "mrirt_inr_class_count", "mrirt_inr_class_index_scratch_bytes", "mrirt_inr_class_index", "mrirt_select_largest",
    "mrirt_inr_normal3", "mrirt_inr_sample_candidates", "mrirt_inr_sample_batch_hybrid",
    "mrirt_inject_fused_lds_bytes", "mrirt_inject_classify", "mrirt_render_brats_inject",
]

ABI_VERSION = 4          # MRIRT_ABI_VERSION of include/mrirt.h this binding was written against
OK = 0
LAYOUT_LINEAR, LAYOUT_BRICK, LAYOUT_VG, LAYOUT_QUAD, LAYOUT_VGA, LAYOUT_LABCELL, LAYOUT_MOD4 = 0, 1, 2, 3, 4, 5, 6
MATH_STRICT, MATH_FAST = 0, 1
OUT_RGBA32F, OUT_RGBA16F = 0, 1
VOX_U32X4, VOX_U8, VOX_F32, VOX_CELL8 = 0, 1, 2, 3
INR_FOURIER_RELU, INR_SIREN = 0, 1
INR_NO_WEIGHT_STATIONARY, INR_NO_REFINE, INR_MARK_ONLY = 1, 2, 4      # MrirtInrFlags
KERNEL_NONE, KERNEL_GENERIC, KERNEL_PIPELINED, KERNEL_ROLLING, KERNEL_SLAB, KERNEL_RING = 0, 1, 2, 3, 4, 5   # MrirtKernelFamily
KERNEL_SKIPPING, KERNEL_LABEL_CELLS = 16, 32

f32, u32 = C.c_float, C.c_uint32


class BratsParams(C.Structure):
    """MrirtBratsParams == struct Params of inr/viewer/brats_rt.slang:12-31."""
    _fields_ = [
        ("imageSize", u32 * 2), ("fovY", f32), ("pad0", f32),
        ("eye", f32 * 3), ("pad1", f32),
        ("U", f32 * 3), ("pad2", f32), ("V", f32 * 3), ("pad3", f32), ("W", f32 * 3), ("pad4", f32),
        ("volMin", f32 * 3), ("pad5", f32), ("voxelSize", f32 * 3), ("pad6", f32), ("dims", u32 * 3), ("pad7", u32),
        ("stepSize", f32), ("nearT", f32), ("farT", f32), ("pad8", f32),
        ("bgColor", f32 * 3), ("pad9", f32),
        ("volEnabled", u32 * 4), ("volWeight", f32 * 4),
        ("ww", f32), ("wl", f32), ("intensityAlpha", f32), ("padInt", f32),
        ("gamma", f32), ("gradBoost", f32), ("gradScale", f32), ("padTone", f32),
        ("showSeg", u32), ("showPred", u32), ("padFlags", u32 * 2),
        ("lutColorAlpha", (f32 * 4) * 8),
    ]


class RenderExt(C.Structure):
    _fields_ = [
        ("cameraMode", u32), ("orthoHalfHeight", f32),
        ("shadeMode", u32), ("ka", f32), ("kd", f32), ("ks", f32), ("specPow2", u32), ("gradEps", f32),
        ("ertOverride", u32), ("ertThreshold", f32),
        ("math", u32), ("outFormat", u32), ("layout", u32), ("labelLayout", u32),
        ("tileSize", u32), ("tileRank", u32), ("tileWorld", u32),
        ("kernelVariant", u32), ("tileSkew", u32), ("reserved", u32),
    ]


class VolumeParams(C.Structure):
    """MrirtVolumeParams == struct Params of scripts/volumeRendering/volume_render.slang:9-21."""
    _fields_ = [
        ("imageSize", u32 * 2), ("fovY", f32), ("stepCount", f32), ("nearPlane", f32), ("farPlane", f32),
        ("eye", f32 * 3), ("padEye", f32), ("U", f32 * 3), ("padU", f32), ("V", f32 * 3), ("padV", f32),
        ("W", f32 * 3), ("padW", f32), ("volDim", u32 * 3), ("padDim", u32),
    ]


class SdfParams(C.Structure):
    """MrirtSdfParams == struct Params + gEye/gU/gV/gW of scripts/raymarch/raymarch.slang:7-21."""
    _fields_ = [
        ("imageSize", u32 * 2), ("fovY", f32), ("maxSteps", u32),
        ("maxDistance", f32), ("hitThreshold", f32), ("normalEps", f32), ("pad0", f32),
        ("gEye", f32 * 3), ("pad1", f32), ("gU", f32 * 3), ("pad2", f32), ("gV", f32 * 3), ("pad3", f32),
        ("gW", f32 * 3), ("pad4", f32),
    ]


class MeshParams(C.Structure):
    """MrirtMeshParams == struct Params of scripts/mesh_rt/mesh_rt.slang:12-21 (cbuffer packing, 80 bytes)."""
    _fields_ = [
        ("imageSize", u32 * 2), ("fovY", f32), ("maxBounces", u32),
        ("eye", f32 * 3), ("padEye", f32), ("U", f32 * 3), ("padU", f32), ("V", f32 * 3), ("padV", f32),
        ("W", f32 * 3), ("padW", f32),
    ]


class InrDesc(C.Structure):
    _fields_ = [
        ("kind", u32), ("numLayers", u32), ("inDim", u32), ("outDim", u32), ("hidden", u32),
        ("fourierFreqs", u32), ("numMods", u32), ("w0", f32),
        ("weights", C.c_void_p), ("biases", C.c_void_p),
        ("flags", u32), ("tieSigmas", f32),
    ]


class InrCache(C.Structure):
    """MrirtInrCache: device tables of per-case mods / seg pointers."""
    _fields_ = [("mods", C.c_void_p), ("seg", C.c_void_p), ("ncases", u32), ("numMods", u32), ("hwd", u32 * 3), ("reserved", u32)]


class AdamW(C.Structure):
    _fields_ = [("lr", f32), ("b1", f32), ("b2", f32), ("eps", f32), ("weightDecay", f32), ("clipNorm", f32)]


class InrTrainCfg(C.Structure):
    _fields_ = [("microBatch", C.c_int64), ("accum", u32), ("warmupSteps", u32), ("decaySteps", u32), ("reserved", u32),
                ("seed", C.c_uint64), ("peakLr", C.c_double), ("minLr", C.c_double), ("classWeights", f32 * 16), ("diceWeight", f32),
                ("adamw", AdamW)]


class InrTrainState(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("w", "b", "mu_w", "mu_b", "nu_w", "nu_b")]


class Muon(C.Structure):
    """MrirtMuon: the hyper-parameters of optax's scale_by_muon."""
    _fields_ = [("beta", f32), ("eps", f32), ("weightDecay", f32), ("nsCoeffs", f32 * 3), ("nsSteps", u32), ("nesterov", u32)]


LOSS_PER_CLASS_DICE, LOSS_FOCAL_ALPHA = 1, 2          # MrirtInrLossExt.flags


class InrLossExt(C.Structure):
    """MrirtInrLossExt: the loss options of scripts/jax_inr_brats.py:205-257."""
    _fields_ = [("classWeights", f32 * 16), ("focalAlpha", f32 * 16), ("diceWeight", f32), ("focalGamma", f32), ("labelSmoothing", f32),
                ("edemaFpWeight", f32), ("tverskyAlpha", f32), ("tverskyBeta", f32), ("tverskyWeight", f32), ("edemaLogitReg", f32),
                ("edemaClass", u32), ("flags", u32)]


class InrTumourIndex(C.Structure):
    """MrirtInrTumourIndex: device pointers to the ascending tumour voxel offsets and the per-case ranges."""
    _fields_ = [("index", C.c_void_p), ("offsets", C.c_void_p)]


class InrTrainExt(C.Structure):
    """MrirtInrTrainExt: what mrirt_inr_train_run_ext takes beyond the plain run; every member may be NULL / 0."""
    _fields_ = [("loss", C.POINTER(InrLossExt)), ("muon", C.POINTER(Muon)), ("tumour", InrTumourIndex), ("nTumour", C.c_int64)]


class InjectDesc(C.Structure):
    """MrirtInjectDesc: the coordinate-injection network of notebooks/improved.ipynb."""
    _fields_ = [("numLayers", u32), ("fourierDim", u32), ("numMods", u32), ("width", u32 * 8), ("coordLayers", u32), ("modLayers", u32)]


class InjectDropout(C.Structure):
    """MrirtInjectDropout: the Philox mask stream of one call."""
    _fields_ = [("seed", C.c_uint64), ("keep", f32), ("samples", u32), ("sample0", u32), ("reserved", u32), ("index0", C.c_uint64)]


class UnifiedLoss(C.Structure):
    """MrirtUnifiedLoss: the loss of notebooks/improved.ipynb, cell 8."""
    _fields_ = [("classWeights", f32 * 16), ("gamma", f32), ("lambda_", f32), ("tverskyAlpha", f32), ("tverskyBeta", f32),
                ("uflWeight", f32), ("diceWeight", f32), ("tvWeight", f32), ("boundaryWeight", f32), ("flags", u32)]


class InrClassIndex(C.Structure):
    """MrirtInrClassIndex: device pointers to the voxel offsets by (class, case) and to the starts of those lists."""
    _fields_ = [("index", C.c_void_p), ("offsets", C.c_void_p), ("numClasses", u32), ("reserved", u32)]


class InrHybrid(C.Structure):
    """MrirtInrHybrid: the segments of one hybrid micro-batch and the sigma of its coordinate noise."""
    _fields_ = [("nUncertain", C.c_int64), ("nPerClass", C.c_int64), ("picks", C.c_void_p), ("noiseSigma", f32), ("reserved", u32)]


class Skip(C.Structure):
    """MrirtSkip: macro-cell summaries + mask scratch for exact empty-space skipping."""
    _fields_ = [("macroUb", C.c_void_p * 4), ("macroSeg", C.c_void_p), ("macroPred", C.c_void_p), ("mask", C.c_void_p),
                ("maskWords", u32), ("mapReady", u32)]


class Order(C.Structure):
    """MrirtOrder: the dispatch-order table and the step record of one stream's K1 launches."""
    _fields_ = [("order", C.c_void_p), ("steps", C.c_void_p), ("words", u32), ("classes", u32)]


class MrirtError(RuntimeError):
    def __init__(self, status: int, where: str):
        l = lib()
        msg = l.mrirt_status_string(status).decode()
        extra = f" (hipError {l.mrirt_last_hip_error()})" if status == -4 else ""
        super().__init__(f"{where}: {msg}{extra} [status {status}]")
        self.status = status


OBJ_DIR = PKG_DIR / "build"          # per-source objects (git-ignored; they do not travel to history)
MAX_BUILD_JOBS = 16                  # compilers at once: os.cpu_count() is the whole machine's, a job may own far fewer


def _hipcc() -> str:
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def hipcc_command(out: Optional[pathlib.Path] = None, extra: Optional[List[str]] = None) -> List[str]:
    """The one-command form of the build (every source in one hipcc call); build() compiles the same sources with the same
    flags one object at a time, in parallel, and links them."""
    return [_hipcc(), *HIPCC_FLAGS, *(extra or []), f"-I{INCLUDE}", *[str(CSRC / s) for s in HIP_SOURCES],
            "-o", str(out or SO_PATH)]


def _headers() -> List[pathlib.Path]:
    return list(CSRC.glob("*.h")) + [INCLUDE / "mrirt.h"]


def _stale() -> bool:
    if not SO_PATH.exists():
        return True
    t = SO_PATH.stat().st_mtime
    srcs = [CSRC / s for s in HIP_SOURCES] + _headers()
    return any(p.stat().st_mtime > t for p in srcs)


def build(force: bool = False, verbose: bool = False, check: bool = True) -> pathlib.Path:
    """Cross-compile every HIP source for gfx950 into the in-tree libmrirt.so (no GPU needed): one object per source, the
    stale ones in parallel, then one link.  A rebuilt library is then checked by tools/check_async_loads.py — the
    pipelined march kernels issue their gathers as inline asm and retire them with hand-counted waits, which is sound only
    as long as no instruction touches a gather destination before its wait; that scan is a correctness gate of the build,
    whichever path (``__graft_entry__.build()``, the test session's rebuild of a stale library) triggered it."""
    if not (force or _stale()):
        return SO_PATH
    from concurrent.futures import ThreadPoolExecutor
    OBJ_DIR.mkdir(exist_ok=True)
    hdr_t = max(p.stat().st_mtime for p in _headers())
    flags = [f for f in HIPCC_FLAGS if f != "-shared"]
    jobs = []
    for src in HIP_SOURCES:
        sp, op = CSRC / src, OBJ_DIR / (src + ".o")
        if force or not op.exists() or op.stat().st_mtime < max(sp.stat().st_mtime, hdr_t):
            jobs.append([_hipcc(), *flags, f"-I{INCLUDE}", "-c", str(sp), "-o", str(op)])

    def run(cmd):
        return cmd, subprocess.run(cmd, capture_output=True, text=True)
    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1, MAX_BUILD_JOBS) or 1) as pool:
        for cmd, r in pool.map(run, jobs):
            if verbose or r.returncode != 0:
                print(" ".join(cmd))
                print(r.stdout + r.stderr)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed on {cmd[-3]}")
    link = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", *[str(OBJ_DIR / (s + ".o")) for s in HIP_SOURCES], "-o", str(SO_PATH)]
    r = subprocess.run(link, capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(" ".join(link))
        print(r.stdout + r.stderr)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed linking libmrirt.so")
    if check:
        tool = PKG_DIR.parent / "tools" / "check_async_loads.py"
        r = subprocess.run([sys.executable, str(tool), str(SO_PATH)], capture_output=True, text=True)
        if verbose or r.returncode != 0:
            print(r.stdout + r.stderr)
        if r.returncode != 0:
            SO_PATH.unlink(missing_ok=True)         # a library that fails the gate must not be loadable
            raise RuntimeError("tools/check_async_loads.py rejected the built libmrirt.so (see output above)")
    return SO_PATH


# --- the C++ PyTorch extension (csrc/torch_binding.cpp -> libmrirt_torch.so: torch.ops.mrirt_native.*) ------------
TORCH_SO_PATH = PKG_DIR / "libmrirt_torch.so"


def torch_binding_command() -> List[str]:
    """Host-compiler command for the operator library: no device code, torch headers + libmrirt.so."""
    import torch
    from torch.utils import cpp_extension as ce
    libdir = pathlib.Path(torch.__file__).resolve().parent / "lib"
    inc = list(ce.include_paths()) + ["/opt/rocm/include", str(INCLUDE)]
    return [os.environ.get("CXX", "g++"), "-O2", "-fPIC", "-shared", "-std=c++17", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
            f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}", "-Wno-deprecated-declarations",
            *[f"-I{i}" for i in inc], str(CSRC / "torch_binding.cpp"), "-o", str(TORCH_SO_PATH),
            f"-L{libdir}", "-lc10", "-ltorch_cpu", "-ltorch", "-lc10_hip", "-ltorch_hip",
            f"-L{PKG_DIR}", "-lmrirt", "-Wl,-rpath,$ORIGIN", f"-Wl,-rpath,{libdir}"]


def build_torch_binding(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """Compile csrc/torch_binding.cpp against this interpreter's torch and the in-tree libmrirt.so."""
    src = CSRC / "torch_binding.cpp"
    stale = (not TORCH_SO_PATH.exists() or src.stat().st_mtime > TORCH_SO_PATH.stat().st_mtime
             or (INCLUDE / "mrirt.h").stat().st_mtime > TORCH_SO_PATH.stat().st_mtime)
    if force or stale:
        build()                                   # links against libmrirt.so
        cmd = torch_binding_command()
        r = subprocess.run(cmd, capture_output=True, text=True)
        if verbose or r.returncode != 0:
            print(" ".join(cmd))
            print(r.stdout + r.stderr)
        if r.returncode != 0:
            raise RuntimeError("building libmrirt_torch.so failed")
    return TORCH_SO_PATH


_LIB: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load libmrirt.so.  Raises if it is absent: the HIP library is the only render path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not SO_PATH.exists():
        raise ImportError(
            f"{SO_PATH} is missing — the HIP extension is the product and has no fallback. "
            "Build it with `python -c \"import __graft_entry__ as g; g.build()\"`.")
    l = C.CDLL(str(SO_PATH))
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    l.mrirt_render_brats.argtypes = [C.POINTER(BratsParams), C.POINTER(vp), vp, vp, vp, i64, vp]
    l.mrirt_render_brats_ex.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp), vp, vp, vp, i64, vp, vp]
    l.mrirt_render_brats_tf.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp), vp, vp, vp, u32, vp, i64, vp, vp]
    l.mrirt_render_brats_tf.restype = i32
    l.mrirt_brats_sample_counts.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), vp, vp]
    l.mrirt_brats_emit_samples.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp),
                                           C.POINTER(f32), C.POINTER(f32), vp, vp, vp, vp]
    l.mrirt_render_brats_stream.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp), vp, vp, vp,
                                            vp, i64, vp, vp]
    for fn in ("mrirt_brats_sample_counts", "mrirt_brats_emit_samples", "mrirt_render_brats_stream"):
        getattr(l, fn).restype = i32
    l.mrirt_brats_inr_scratch_bytes.argtypes = [C.POINTER(BratsParams), u32]
    l.mrirt_brats_inr_scratch_bytes.restype = i64
    l.mrirt_render_brats_inr.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp), vp, C.POINTER(InrDesc),
                                         C.POINTER(f32), C.POINTER(f32), u32, vp, i64, vp, i64, vp, vp]
    l.mrirt_render_brats_inr.restype = i32
    l.mrirt_brick_elems.argtypes = [C.POINTER(u32)]
    l.mrirt_brick_elems.restype = i64
    l.mrirt_brick_grid.argtypes = [vp, vp, C.POINTER(u32), u32, vp]
    l.mrirt_unbrick_grid.argtypes = [vp, vp, C.POINTER(u32), u32, vp]
    l.mrirt_vec4_elems.argtypes = [C.POINTER(u32)]
    l.mrirt_vec4_elems.restype = i64
    l.mrirt_vga_elems.argtypes = [C.POINTER(u32)]
    l.mrirt_vga_elems.restype = i64
    l.mrirt_build_vec4_grid.argtypes = [vp, vp, C.POINTER(u32), u32, vp]
    l.mrirt_build_label_cells.argtypes = [vp, vp, C.POINTER(u32), vp, vp]
    l.mrirt_build_label_cells.restype = i32
    l.mrirt_build_mod4_grid.argtypes = [C.POINTER(vp), vp, C.POINTER(u32), vp]
    l.mrirt_build_mod4_grid.restype = i32
    l.mrirt_macro_cells.argtypes = [C.POINTER(u32)]
    l.mrirt_macro_cells.restype = i64
    l.mrirt_skip_mask_words.argtypes = [C.POINTER(u32)]
    l.mrirt_skip_mask_words.restype = i64
    l.mrirt_build_macro_max.argtypes = [vp, C.POINTER(u32), vp, vp]
    l.mrirt_build_macro_max.restype = i32
    l.mrirt_build_macro_labels.argtypes = [vp, C.POINTER(u32), vp, vp]
    l.mrirt_build_macro_labels.restype = i32
    l.mrirt_render_brats_skip.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp), vp, vp, C.POINTER(Skip), vp, i64, vp, vp]
    l.mrirt_render_brats_skip.restype = i32
    l.mrirt_brats_skip_applicable.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp), vp, vp, C.POINTER(Skip)]
    l.mrirt_brats_skip_applicable.restype = i32
    l.mrirt_brats_kernel_family.argtypes = l.mrirt_brats_skip_applicable.argtypes
    l.mrirt_brats_kernel_family.restype = i32
    l.mrirt_order_words.argtypes = [C.POINTER(u32), C.POINTER(RenderExt)]
    l.mrirt_order_words.restype = i64
    l.mrirt_render_brats_ordered.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp), vp, vp, C.POINTER(Skip), C.POINTER(Order),
                                             vp, i64, vp, vp]
    l.mrirt_render_brats_ordered.restype = i32
    l.mrirt_brats_order_applicable.argtypes = l.mrirt_brats_skip_applicable.argtypes
    l.mrirt_brats_order_applicable.restype = i32
    l.mrirt_order_build_host.argtypes = [vp, u32, u32, vp]
    l.mrirt_order_build_host.restype = i32
    l.mrirt_install_abort_trace.argtypes = [i32]
    l.mrirt_install_abort_trace.restype = i32
    l.mrirt_build_cell8.argtypes = [vp, u32, C.POINTER(u32), vp, vp]
    l.mrirt_build_cell8.restype = i32
    l.mrirt_bc4_decode.argtypes = [vp, u32, u32, u32, vp, vp]
    l.mrirt_bc4_decode.restype = i32
    l.mrirt_render_volume.argtypes = [C.POINTER(VolumeParams), C.POINTER(RenderExt), vp, u32, vp, i64, vp, vp]
    l.mrirt_render_sdf.argtypes = [C.POINTER(SdfParams), u32, u32, vp, i64, vp]
    l.mrirt_render_mesh.argtypes = [C.POINTER(MeshParams), C.POINTER(RenderExt), vp, u32, vp, u32, vp, u32, u32, vp, i64, vp, vp, vp]
    l.mrirt_render_mesh.restype = i32
    l.mrirt_tiles_for_rank.argtypes = [u32, u32, u32, u32, u32]
    l.mrirt_tiles_for_rank.restype = i64
    l.mrirt_detile.argtypes = [vp, vp, u32, u32, i64, u32, u32, u32, u32, vp]
    l.mrirt_inr_pack_bytes.argtypes = [C.POINTER(InrDesc)]
    l.mrirt_inr_pack_bytes.restype = i64
    l.mrirt_inr_pack_weights.argtypes = [C.POINTER(InrDesc), vp, vp, vp]
    l.mrirt_inr_forward.argtypes = [C.POINTER(InrDesc), vp, vp, i64, vp, vp, vp]
    l.mrirt_inr_forward_refined.argtypes = [C.POINTER(InrDesc), vp, vp, i64, vp, vp, vp]
    l.mrirt_inr_calibrate.argtypes = [C.POINTER(InrDesc), vp]
    l.mrirt_inr_predict_volume.argtypes = [C.POINTER(InrDesc), vp, C.POINTER(u32), vp, vp]
    l.mrirt_edt_scratch_bytes.argtypes = [C.POINTER(u32), u32]
    l.mrirt_edt_scratch_bytes.restype = i64
    l.mrirt_edt_squared.argtypes = [vp, C.POINTER(u32), i32, C.POINTER(f32), vp, vp, i64, vp]
    l.mrirt_edt_squared.restype = i32
    l.mrirt_hausdorff.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(f32), u32, vp, vp, i64, vp]
    l.mrirt_hausdorff.restype = i32
    l.mrirt_surface_scratch_bytes.argtypes = [C.POINTER(u32)]
    l.mrirt_surface_scratch_bytes.restype = i64
    l.mrirt_surface_count.argtypes = [vp, C.POINTER(u32), u32, vp, i64, vp, vp]
    l.mrirt_surface_count.restype = i32
    l.mrirt_surface_extract.argtypes = [vp, C.POINTER(u32), u32, C.POINTER(f32), C.POINTER(f32), vp, i64, vp, i64, vp, i64, vp, vp]
    l.mrirt_surface_extract.restype = i32
    l.mrirt_render_brats_backward.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp), vp, vp, vp, i64, C.POINTER(vp), vp, vp]
    l.mrirt_render_brats_backward.restype = i32
    l.mrirt_render_brats_soft.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp), vp, vp, u32, vp, vp, i64, vp, vp]
    l.mrirt_render_brats_soft.restype = i32
    l.mrirt_render_brats_soft_backward.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp), vp, vp, u32, vp, vp, i64, vp, vp]
    l.mrirt_render_brats_soft_backward.restype = i32
    l.mrirt_inr_train_scratch_bytes.argtypes = [C.POINTER(InrDesc), i64]
    l.mrirt_inr_train_scratch_bytes.restype = i64
    l.mrirt_inr_loss_scratch_bytes.argtypes = [i64]
    l.mrirt_inr_loss_scratch_bytes.restype = i64
    l.mrirt_inr_forward_f32.argtypes = [C.POINTER(InrDesc), vp, vp, vp, vp, i64, vp, vp, i64, vp]
    l.mrirt_inr_forward_f32.restype = i32
    l.mrirt_inr_loss.argtypes = [vp, vp, i64, u32, C.POINTER(f32), f32, vp, vp, vp, vp, i64, vp]
    l.mrirt_inr_loss.restype = i32
    l.mrirt_inr_backward.argtypes = [C.POINTER(InrDesc), vp, i64, vp, vp, vp, u32, vp, i64, vp]
    l.mrirt_inr_backward.restype = i32
    u64 = C.c_uint64
    l.mrirt_inr_sample_batch.argtypes = [C.POINTER(InrCache), u64, u64, i64, vp, vp, vp, vp]
    l.mrirt_inr_sample_batch.restype = i32
    l.mrirt_inr_adamw_scratch_bytes.argtypes = [i64]
    l.mrirt_inr_adamw_scratch_bytes.restype = i64
    l.mrirt_inr_adamw_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, C.POINTER(AdamW), u64, f32, vp, vp, i64, vp]
    l.mrirt_inr_adamw_step.restype = i32
    l.mrirt_inr_lr_schedule.argtypes = [C.c_double, C.c_double, u32, u32, u64, C.POINTER(C.c_double)]
    l.mrirt_inr_lr_schedule.restype = i32
    l.mrirt_inr_train_run_scratch_bytes.argtypes = [C.POINTER(InrDesc), C.POINTER(InrCache), C.POINTER(InrTrainCfg)]
    l.mrirt_inr_train_run_scratch_bytes.restype = i64
    l.mrirt_inr_train_run.argtypes = [C.POINTER(InrDesc), C.POINTER(InrCache), C.POINTER(InrTrainCfg), C.POINTER(InrTrainState), u64, u32,
                                      vp, vp, i64, vp]
    l.mrirt_inr_train_run.restype = i32
    for twin in ("train_scratch_bytes", "forward_f32", "backward", "train_run_scratch_bytes", "train_run"):     # the SIREN twins
        src, dst = getattr(l, "mrirt_inr_" + twin), getattr(l, "mrirt_siren_" + twin)
        dst.argtypes, dst.restype = src.argtypes, src.restype
    l.mrirt_muon_scratch_bytes.argtypes = [C.POINTER(InrDesc)]
    l.mrirt_muon_scratch_bytes.restype = i64
    l.mrirt_muon_orthogonalize.argtypes = [C.POINTER(InrDesc), vp, vp, C.POINTER(Muon), vp, i64, vp]
    l.mrirt_muon_orthogonalize.restype = i32
    l.mrirt_muon_step.argtypes = [C.POINTER(InrDesc), vp, vp, vp, vp, vp, vp, vp, C.POINTER(Muon), C.POINTER(AdamW), u64, f32, vp, vp, i64, vp]
    l.mrirt_muon_step.restype = i32
    l.mrirt_inr_train_run_muon_scratch_bytes.argtypes = [C.POINTER(InrDesc), C.POINTER(InrCache), C.POINTER(InrTrainCfg)]
    l.mrirt_inr_train_run_muon_scratch_bytes.restype = i64
    l.mrirt_inr_train_run_muon.argtypes = [C.POINTER(InrDesc), C.POINTER(InrCache), C.POINTER(InrTrainCfg), C.POINTER(Muon),
                                           C.POINTER(InrTrainState), u64, u32, vp, vp, i64, vp]
    l.mrirt_inr_train_run_muon.restype = i32
    l.mrirt_inr_loss_ext_scratch_bytes.argtypes = [i64]
    l.mrirt_inr_loss_ext_scratch_bytes.restype = i64
    l.mrirt_inr_loss_ext.argtypes = [vp, vp, i64, u32, C.POINTER(InrLossExt), vp, vp, vp, vp, vp, i64, vp]
    l.mrirt_inr_loss_ext.restype = i32
    l.mrirt_inr_tumour_count.argtypes = [C.POINTER(InrCache), vp, vp]
    l.mrirt_inr_tumour_count.restype = i32
    l.mrirt_inr_tumour_index_scratch_bytes.argtypes = [C.POINTER(InrCache)]
    l.mrirt_inr_tumour_index_scratch_bytes.restype = i64
    l.mrirt_inr_tumour_index.argtypes = [C.POINTER(InrCache), vp, vp, vp, i64, vp]
    l.mrirt_inr_tumour_index.restype = i32
    l.mrirt_inr_sample_batch_mix.argtypes = [C.POINTER(InrCache), C.POINTER(InrTumourIndex), u64, u64, i64, i64, vp, vp, vp, vp]
    l.mrirt_inr_sample_batch_mix.restype = i32
    l.mrirt_inr_train_run_ext_scratch_bytes.argtypes = [C.POINTER(InrDesc), C.POINTER(InrCache), C.POINTER(InrTrainCfg), C.POINTER(InrTrainExt)]
    l.mrirt_inr_train_run_ext_scratch_bytes.restype = i64
    l.mrirt_inr_train_run_ext.argtypes = [C.POINTER(InrDesc), C.POINTER(InrCache), C.POINTER(InrTrainCfg), C.POINTER(InrTrainExt),
                                          C.POINTER(InrTrainState), u64, u32, vp, vp, i64, vp]
    l.mrirt_inr_train_run_ext.restype = i32
    l.mrirt_prep_scratch_bytes.argtypes = [i64]
    l.mrirt_prep_scratch_bytes.restype = i64
    l.mrirt_prep_window.argtypes = [vp, i64, f32, f32, vp, vp, i64, vp]
    l.mrirt_prep_window.restype = i32
    l.mrirt_prep_normalize.argtypes = [vp, C.POINTER(u32), vp, vp, vp, vp]
    l.mrirt_prep_normalize.restype = i32
    l.mrirt_prep_zscore_scratch_bytes.argtypes = [i64, u32]
    l.mrirt_prep_zscore_scratch_bytes.restype = i64
    l.mrirt_prep_zscore_stats.argtypes = [vp, i64, u32, vp, vp, i64, vp]
    l.mrirt_prep_zscore_stats.restype = i32
    l.mrirt_prep_zscore_apply.argtypes = [vp, i64, u32, vp, vp, vp]
    l.mrirt_prep_zscore_apply.restype = i32
    l.mrirt_prep_gaussian3d.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_double), i32, vp, vp, vp]
    l.mrirt_prep_gaussian3d.restype = i32
    l.mrirt_cc_scratch_bytes.argtypes = [C.POINTER(u32)]
    l.mrirt_cc_scratch_bytes.restype = i64
    l.mrirt_cc_label.argtypes = [vp, C.POINTER(u32), u32, u32, vp, vp, vp, i64, vp]
    l.mrirt_cc_label.restype = i32
    l.mrirt_cc_sizes.argtypes = [vp, C.POINTER(u32), i64, vp, vp]
    l.mrirt_cc_sizes.restype = i32
    l.mrirt_cc_filter.argtypes = [vp, vp, vp, i64, C.POINTER(u32), i64, i32, C.c_int16, vp, vp]
    l.mrirt_cc_filter.restype = i32
    l.mrirt_slice_counts.argtypes = [vp, C.POINTER(u32), vp, vp]
    l.mrirt_slice_counts.restype = i32
    inj = [C.POINTER(InjectDesc), vp, vp, vp]
    l.mrirt_inject_scratch_bytes.argtypes = [C.POINTER(InjectDesc), i64]
    l.mrirt_inject_scratch_bytes.restype = i64
    l.mrirt_inject_forward.argtypes = [*inj, vp, vp, i64, C.POINTER(InjectDropout), vp, vp, vp, i64, vp]
    l.mrirt_inject_forward.restype = i32
    l.mrirt_inject_uncertainty.argtypes = [*inj, vp, vp, i64, C.POINTER(InjectDropout), vp, vp, vp, i64, vp]
    l.mrirt_inject_uncertainty.restype = i32
    l.mrirt_inject_predict_volume.argtypes = [*inj, vp, C.POINTER(u32), i64, C.POINTER(InjectDropout), vp, vp, vp, i64, vp]
    l.mrirt_inject_predict_volume.restype = i32
    l.mrirt_inject_train_scratch_bytes.argtypes = [C.POINTER(InjectDesc), i64]
    l.mrirt_inject_train_scratch_bytes.restype = i64
    l.mrirt_inject_forward_train.argtypes = [*inj, vp, vp, i64, C.POINTER(InjectDropout), vp, vp, i64, vp]
    l.mrirt_inject_forward_train.restype = i32
    l.mrirt_inject_backward.argtypes = [C.POINTER(InjectDesc), vp, vp, vp, vp, i64, C.POINTER(InjectDropout), vp, vp, vp, vp, u32, vp, i64, vp]
    l.mrirt_inject_backward.restype = i32
    l.mrirt_boundary_weights_scratch_bytes.argtypes = [C.POINTER(u32)]
    l.mrirt_boundary_weights_scratch_bytes.restype = i64
    l.mrirt_boundary_weights.argtypes = [vp, C.POINTER(u32), u32, vp, vp, i64, vp]
    l.mrirt_boundary_weights.restype = i32
    l.mrirt_unified_loss_scratch_bytes.argtypes = [i64]
    l.mrirt_unified_loss_scratch_bytes.restype = i64
    l.mrirt_unified_loss.argtypes = [vp, vp, vp, i64, u32, C.POINTER(UnifiedLoss), vp, vp, vp, vp, i64, vp]
    l.mrirt_unified_loss.restype = i32
    l.mrirt_inr_sample_field.argtypes = [C.POINTER(InrCache), C.POINTER(InrTumourIndex), vp, u64, u64, i64, i64, vp, vp]
    l.mrirt_inr_sample_field.restype = i32
    l.mrirt_inr_class_count.argtypes = [C.POINTER(InrCache), u32, vp, vp]
    l.mrirt_inr_class_count.restype = i32
    l.mrirt_inr_class_index_scratch_bytes.argtypes = [C.POINTER(InrCache), u32]
    l.mrirt_inr_class_index_scratch_bytes.restype = i64
    l.mrirt_inr_class_index.argtypes = [C.POINTER(InrCache), u32, vp, vp, vp, i64, vp]
    l.mrirt_inr_class_index.restype = i32
    l.mrirt_select_largest.argtypes = [vp, i64, i64, vp, vp]
    l.mrirt_select_largest.restype = i32
    l.mrirt_inr_normal3.argtypes = [u64, u64, i64, vp, vp]
    l.mrirt_inr_normal3.restype = i32
    l.mrirt_inr_sample_candidates.argtypes = [C.POINTER(InrCache), u64, u64, i64, vp, vp, vp, vp]
    l.mrirt_inr_sample_candidates.restype = i32
    l.mrirt_inr_sample_batch_hybrid.argtypes = [C.POINTER(InrCache), C.POINTER(InrClassIndex), C.POINTER(InrHybrid), vp, u64, u64, i64, vp, vp, vp,
                                                vp, vp]
    l.mrirt_inr_sample_batch_hybrid.restype = i32
    l.mrirt_inject_fused_lds_bytes.argtypes = [C.POINTER(InjectDesc)]
    l.mrirt_inject_fused_lds_bytes.restype = i64
    l.mrirt_inject_classify.argtypes = [*inj, vp, vp, i64, vp, vp, vp, vp]
    l.mrirt_inject_classify.restype = i32
    l.mrirt_render_brats_inject.argtypes = [C.POINTER(BratsParams), C.POINTER(RenderExt), C.POINTER(vp), vp, *inj,
                                            C.POINTER(f32), C.POINTER(f32), u32, vp, i64, vp, i64, vp, vp]
    l.mrirt_render_brats_inject.restype = i32
    l.mrirt_status_string.argtypes = [i32]
    l.mrirt_status_string.restype = C.c_char_p
    l.mrirt_sizeof.argtypes = [u32]
    l.mrirt_sizeof.restype = u32
    for fn in ("mrirt_render_brats", "mrirt_render_brats_ex", "mrirt_brick_grid", "mrirt_unbrick_grid", "mrirt_build_vec4_grid",
               "mrirt_render_volume", "mrirt_render_sdf", "mrirt_detile", "mrirt_inr_pack_weights",
               "mrirt_inr_forward", "mrirt_inr_forward_refined", "mrirt_inr_calibrate", "mrirt_inr_predict_volume",
               "mrirt_abi_version", "mrirt_last_hip_error"):
        getattr(l, fn).restype = i32
    if l.mrirt_abi_version() != ABI_VERSION:
        raise ImportError(f"ABI mismatch: {SO_PATH} reports version {l.mrirt_abi_version()}, this binding expects {ABI_VERSION} "
                          "(rebuild: python -c \"import __graft_entry__ as g; g.build()\")")
    for which, st in enumerate((BratsParams, RenderExt, VolumeParams, SdfParams, InrDesc, Skip, MeshParams, InrCache, AdamW, InrTrainCfg,
                                InrTrainState, Muon, None, InrLossExt, InrTumourIndex, InrTrainExt)):          # index 12 is unassigned
        if st is not None and l.mrirt_sizeof(which) != C.sizeof(st):
            raise ImportError(f"ABI mismatch: {st.__name__} is {C.sizeof(st)} B here, {l.mrirt_sizeof(which)} B in {SO_PATH}")
    for which, st in ((17, InjectDesc), (18, InjectDropout), (20, UnifiedLoss), (22, InrClassIndex), (23, InrHybrid)):   # 16, 19 and 21 are unassigned
        if l.mrirt_sizeof(which) != C.sizeof(st):
            raise ImportError(f"ABI mismatch: {st.__name__} is {C.sizeof(st)} B here, {l.mrirt_sizeof(which)} B in {SO_PATH}")
    _LIB = l
    return l


def check(status: int, where: str) -> None:
    if status != OK:
        raise MrirtError(status, where)
