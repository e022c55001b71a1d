"""Host-side logic, no GPU: the C-ABI library loads and exports every symbol include/mrirt.h
declares (no compute calls), parameter marshalling, volume preparation vs the oracle, tile
bookkeeping, and the product's refusal to run without the HIP path."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import mrirt
from mrirt import _lib, params, synth, tiles, volume
from oracle import oracle_np as onp

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_header_symbols_are_exported():
    hdr = (ROOT / "include" / "mrirt.h").read_text()
    declared = set(re.findall(r"\b(mrirt_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.ABI_SYMBOLS), declared ^ set(_lib.ABI_SYMBOLS)
    lib = _lib.lib()                       # dlopen works without a GPU; no kernel is launched here
    for s in declared:
        assert hasattr(lib, s), s
    assert lib.mrirt_abi_version() == _lib.ABI_VERSION == 4
    assert lib.mrirt_status_string(0) == b"ok" and b"NULL" in lib.mrirt_status_string(-1)


def test_struct_sizes_match_the_library_and_slang_layout():
    lib = _lib.lib()
    for which, st in enumerate((_lib.BratsParams, _lib.RenderExt, _lib.VolumeParams, _lib.SdfParams, _lib.InrDesc)):
        assert lib.mrirt_sizeof(which) == C.sizeof(st)
    # struct Params of brats_rt.slang:12-31: 16-byte rows; 8 float4 LUT rows at the end
    assert C.sizeof(_lib.BratsParams) == 16 * 15 + 16 * 8
    assert _lib.BratsParams.lutColorAlpha.offset == 16 * 15
    assert _lib.BratsParams.eye.offset == 16 and _lib.BratsParams.dims.offset == 16 * 7
    assert C.sizeof(_lib.VolumeParams) == 24 + 16 * 5     # volume_render.slang:9-21
    assert C.sizeof(_lib.RenderExt) % 4 == 0


def test_null_and_argument_errors_without_launching():
    lib = _lib.lib()
    assert lib.mrirt_render_brats(None, None, None, None, None, 0, None) == -1
    d = (C.c_uint32 * 3)(8, 8, 8)
    assert lib.mrirt_brick_elems(d) == 2 * 2 * 4 * 32
    assert lib.mrirt_vec4_elems(d) == 4 * 4 * 4 * 8
    d2 = (C.c_uint32 * 3)(9, 7, 5)
    assert lib.mrirt_brick_elems(d2) == 3 * 2 * 3 * 32 and lib.mrirt_vec4_elems(d2) == 5 * 4 * 3 * 8
    assert lib.mrirt_brick_grid(None, None, d, 4, None) == -1
    assert lib.mrirt_tiles_for_rank(100, 100, 64, 0, 3) == 2 and lib.mrirt_tiles_for_rank(100, 100, 64, 3, 3) == 0


def test_brats_params_from_the_viewer_dict():
    p = synth.brats_scene(16, 32, 64, channels=3, show_seg=True)
    P = params.brats_params(p)
    assert tuple(P.imageSize) == (32, 32) and tuple(P.dims) == (16, 16, 16)
    assert list(P.volEnabled) == [1, 1, 1, 0] and P.showSeg == 1 and P.showPred == 0
    assert np.allclose(list(P.eye), p["eye"]) and abs(P.stepSize - p["stepSize"]) < 1e-9
    assert np.allclose(np.array([list(r) for r in P.lutColorAlpha]), synth.VIEWER_LUT)
    assert P.gradBoost == 1.5 and P.gradScale == 1.0          # bound by the viewer, unread by the shader
    with pytest.raises(KeyError):
        params.brats_params({k: v for k, v in p.items() if k != "lutColorAlpha"})
    with pytest.raises(TypeError):
        params.brats_params(dict(p, lutColorAlpha=[(0, 0, 0, 0)] * 7))
    E = params.render_ext(dict(synth.SHADE_EXT, math="fast", layout="vg", labelLayout="brick", ertThreshold=0.0))
    assert (E.shadeMode, E.math, E.layout, E.labelLayout, E.ertOverride) == (1, 1, 2, 1, 1)
    assert params.render_ext(None).ertOverride == 0
    with pytest.raises(KeyError):
        params.render_ext({"no_such_field": 1})


def test_volume_prep_matches_oracle():
    rng = np.random.default_rng(3)
    raw = (rng.gamma(2.0, 200.0, (11, 9, 7))).astype(np.float32)
    lin, norm, dims = volume.normalize_intensity(raw)
    olin, onorm, odims = onp.normalize_volume(raw)
    assert np.array_equal(lin, olin) and np.array_equal(norm, onorm) and np.array_equal(dims, odims)
    assert lin.dtype == np.float32 and lin.min() == 0.0 and lin.max() == 1.0
    assert lin[3 + 2 * 11 + 5 * 99] == norm[3, 2, 5]                      # x fastest
    flat = np.full((4, 4, 4), 7.0, np.float32)                              # degenerate percentiles
    assert np.array_equal(volume.normalize_intensity(flat)[0], onp.normalize_volume(flat)[0])
    seg = rng.integers(0, 5, (11, 9, 7)).astype(np.float32) + rng.uniform(-0.2, 0.2, (11, 9, 7)).astype(np.float32)
    a, ad = volume.labels_to_uint(seg)
    b, bd = onp.flatten_labels(seg)
    assert np.array_equal(a, b) and a.dtype == np.uint32 and np.array_equal(ad, bd)
    for dims_, zooms in (((240, 240, 155), (1.0, 1.0, 1.0)), ((64, 128, 32), (0.5, 0.5, 2.0))):
        got, want = volume.world_frame(dims_, zooms), onp.world_scale(dims_, zooms)
        for g, w in zip(got, want):
            assert np.array_equal(np.asarray(g), np.asarray(w))
    vs, vmin, tgt, rad = volume.world_frame((240, 240, 155), (1.0, 1.0, 1.0))
    assert abs(vs[0] * 240 - 1.8) < 1e-6 and np.allclose(tgt, 0, atol=1e-7)


def test_u8_pack_mask_and_bc4_match_oracle():
    rng = np.random.default_rng(4)
    u8 = rng.integers(0, 256, 105).astype(np.uint8)
    assert np.array_equal(volume.pack_u8_as_u32x4(u8), onp.pack_u8_volume(u8))
    m = rng.choice([0.0, 1.0, 2.0, 4.0, 0.6], (6, 5, 4)).astype(np.float32)
    for mode in ("occupancy", "labels"):
        assert np.array_equal(volume.mask_to_u8(m, mode), onp.mask_to_u8(m, mode))
    with pytest.raises(ValueError):
        volume.mask_to_u8(m, "nope")
    W, H, D = 10, 7, 3                                   # not multiples of 4: cropped tiles
    blob = rng.integers(0, 256, D * 3 * 2 * 8).astype(np.uint8).tobytes()
    assert np.array_equal(volume.bc4_decode(blob, W, H, D), onp.bc4_decode(blob, W, H, D))
    with pytest.raises(RuntimeError):
        volume.bc4_decode(blob[:-1], W, H, D)
    z = rng.standard_normal((5, 4, 3)).astype(np.float32)
    z[0, 0, 0] = 0.0
    assert np.array_equal(volume.zscore_nonzero(z), onp.zscore_modality(z))


def test_tile_bookkeeping():
    for (w, h, t, world) in ((1024, 1024, 64, 8), (150, 100, 32, 3), (64, 64, 64, 4), (2880, 2880, 64, 8)):
        n = tiles.num_tiles(w, h, t)
        counts = [tiles.local_tile_count(w, h, t, r, world) for r in range(world)]
        assert sum(counts) == n and max(counts) - min(counts) <= 1 and counts[0] == max(counts)
        lib = _lib.lib()
        assert counts == [lib.mrirt_tiles_for_rank(w, h, t, r, world) for r in range(world)]
    assert tiles.tile_origin(5, 150, 32) == (0, 32) and tiles.tile_origin(4, 150, 32) == (128, 0)
    e = tiles.shard_ext(dict(math="fast"), 2, 8)
    assert e == dict(math="fast", tileSize=64, tileRank=2, tileWorld=8, tileSkew=0)
    # the diagonal deal (tileSkew): a permutation of every tile row, rank(tx, ty) = (tx + ty) mod world when tilesX % world == 0
    for (w, t, world) in ((2048, 64, 8), (2048, 32, 4), (150, 32, 3), (64, 64, 1)):
        skew = tiles.balanced_skew(w, t, world)
        tiles_x = (w + t - 1) // t
        seen = set()
        for tid in range(tiles_x * 6):
            x0, y0 = tiles.tile_origin(tid, w, t, skew)
            assert 0 <= x0 < tiles_x * t and y0 == (tid // tiles_x) * t and (x0, y0) not in seen
            seen.add((x0, y0))
            if tiles_x % world == 0:
                assert tid % world == (x0 // t + y0 // t) % world
    assert tiles.balanced_skew(2048, 64, 8) == 7 and tiles.balanced_skew(2048, 64, 1) == 0


def test_assemble_frame_on_host_tensors():
    import torch
    w, h, t, world = 150, 100, 32, 3
    tx, ty = 5, 4
    frame = torch.arange(ty * t * tx * t * 4, dtype=torch.float32).reshape(ty * t, tx * t, 4)
    maxl = tiles.local_tile_count(w, h, t, 0, world)
    g = torch.zeros(world, maxl, t, t, 4)
    for skew in (0, 2, 4):
        for tid in range(tx * ty):
            x0, y0 = tiles.tile_origin(tid, w, t, skew)
            g[tid % world, tid // world] = frame[y0:y0 + t, x0:x0 + t]
        out = tiles.assemble_frame(g, w, h, t, world, skew)
        assert out.shape == (h, w, 4) and torch.equal(out, frame[:h, :w]), skew


def test_no_cpu_fallback():
    """Without a GPU the product must fail loudly, never route to the oracle."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = synth.brats_scene(8, 8, 8, channels=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mrirt.render_brats(p, [np.zeros(512, np.float32)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mrirt.shim.Device()
    src = "".join(f.read_text() for f in (ROOT / "mri-raytracer_amd").glob("*.py"))
    assert "import oracle" not in src and "from oracle" not in src


def test_synth_is_deterministic_and_in_range():
    a, b = synth.synth_volume(16), synth.synth_volume(16)
    assert np.array_equal(a, b) and a.dtype == np.float32 and a.min() >= 0 and a.max() <= 1
    lab = synth.synth_labels(16)
    assert set(np.unique(lab)) <= {0, 1, 2, 3} and lab.dtype == np.uint32
    assert not np.array_equal(a, synth.synth_volume(16, seed=1235))


def test_model_load_both_layouts(golden_dir, tmp_path):
    import json
    g = np.load(golden_dir / "inr_fourier.npz")
    params = [{"W": g[f"k2h32x2_W{i}"], "b": g[f"k2h32x2_b{i}"]} for i in range(3)]
    flat = {}
    for i, p in enumerate(params):
        flat[f"W_{i}"], flat[f"b_{i}"] = p["W"], p["b"]
    np.savez(tmp_path / "ckpt.npz", **flat)
    (tmp_path / "ckpt_info.json").write_text(json.dumps({"config": {"FOURIER_FREQS": 2}, "NUM_CLASSES": 4}))
    got, cfg = mrirt.inr.model_load(tmp_path / "ckpt.npz", config_override={"DATA_ROOT": "/x"})
    assert cfg["config"]["FOURIER_FREQS"] == 2 and cfg["DATA_ROOT"] == "/x"
    assert all(np.array_equal(a["W"], b["W"]) and np.array_equal(a["b"], b["b"]) for a, b in zip(got, params))
    arr = np.empty((), dtype=object)
    arr[()] = params
    np.savez(tmp_path / "final.npz", params=arr)
    (tmp_path / "final_info.json").write_text("{}")
    with pytest.raises(ValueError):
        mrirt.inr.model_load(tmp_path / "final.npz")                               # pickle refused by default
    got2, _ = mrirt.inr.model_load(tmp_path / "final.npz", config_override={"ALLOW_PICKLE": True})
    assert np.array_equal(got2[0]["W"], params[0]["W"])
    with pytest.raises(FileNotFoundError):
        mrirt.inr.model_load(tmp_path / "missing.npz")


def test_torch_ops_are_registered_with_shape_functions():
    """torch.ops.mrirt.*: present, the parameter blobs are the C structs byte for byte, and the shape
    functions answer on meta tensors (no GPU, no compute)."""
    import ctypes as C
    import torch
    from mrirt import _lib, torch_ops
    for name in ("render_brats", "render_volume", "render_sdf", "inr_forward"):
        assert hasattr(torch.ops.mrirt, name)
    p = synth.brats_scene(32, 64, 32, channels=1)
    blob, ext = torch_ops.pack_brats_params(p), torch_ops.pack_render_ext({"layout": "vg", "outFormat": "rgba16f"})
    assert blob.numel() == C.sizeof(_lib.BratsParams) == 368 and ext.numel() == C.sizeof(_lib.RenderExt)
    back = _lib.BratsParams.from_buffer_copy(blob.numpy().tobytes())
    assert tuple(back.imageSize) == (64, 64) and tuple(back.dims) == (32, 32, 32)
    v = torch.empty(4 * 16 ** 3 * 8, device="meta")
    o = torch.ops.mrirt.render_brats(blob, ext, v, None, None, None, None, None)
    assert o.shape == (64, 64, 4) and o.dtype == torch.float16 and o.device.type == "meta"
    tiled = torch_ops.pack_render_ext({"tileSize": 16, "tileRank": 1, "tileWorld": 3})
    o = torch.ops.mrirt.render_brats(blob, tiled, torch.empty(32 ** 3, device="meta"), None, None, None, None, None)
    assert o.shape == (mrirt.tiles.local_tile_count(64, 64, 16, 1, 3), 16, 16, 4)
    o = torch.ops.mrirt.inr_forward(torch.empty(1, dtype=torch.uint8, device="meta"), torch.empty(1, device="meta"),
                                    1, 3, 7, 4, 64, 0, 4, 30.0, None, None, 10)
    assert o.shape == (10, 4)
    with pytest.raises(TypeError):
        torch.ops.mrirt.render_brats(blob[:-4], ext, v, None, None, None, None, None)


def test_native_operator_library_builds_and_registers():
    """csrc/torch_binding.cpp (the C++ PyTorch extension over the C ABI): compiles against this torch, loads without a
    GPU, registers its operators (all 19: tests/test_torch_ops_contract.py), and its argument checks fire before anything touches
    the device."""
    import torch
    from mrirt import torch_ops
    _lib.build_torch_binding()
    ops = torch_ops.load_native()
    for name in ("render_brats", "render_volume", "render_sdf", "inr_forward"):
        assert hasattr(ops, name)
    p = synth.brats_scene(32, 64, 32, channels=1)
    blob, ext = torch_ops.pack_brats_params(p), torch_ops.pack_render_ext({"layout": "vg"})
    with pytest.raises(TypeError):
        ops.render_brats(blob[:-4], ext, None, None, None, None, None, None)          # not a MrirtBratsParams
    with pytest.raises(ValueError):
        ops.render_brats(blob, ext, None, None, None, None, None, None)               # the enabled modality is not bound
    with pytest.raises(TypeError):
        ops.render_brats(blob, ext, torch.zeros(8), None, None, None, None, None)     # a host tensor as gIntensity0


def test_bad_steps_are_refused_on_the_host_not_hung_on_the_gpu():
    """a step that is <= 0, NaN or too small to advance t in fp32 would spin the march loop
    (`while (t < t1 && T > ert) ... t += stepSize`, and the C5 count/emit loops have no transmittance exit).
    prepare() refuses those with MRIRT_ERR_ARG before anything is launched — checked here without a GPU by
    passing non-NULL dummy pointers that are never dereferenced on an error return."""
    lib = _lib.lib()
    good = synth.brats_scene(32, 64, 64, channels=1)
    dummy = C.c_void_p(0x1000)
    vp = (C.c_void_p * 4)(dummy, None, None, None)

    def rc_ex(p):
        P = params.brats_params(p)
        return lib.mrirt_render_brats_ex(C.byref(P), None, vp, None, None, dummy, 64, None, None)

    for bad in (0.0, -0.01, float("nan"), float("inf"), 1e-9, 1.8 * 3 ** 0.5 / (1 << 21)):
        assert rc_ex(dict(good, stepSize=bad)) == -5, bad
    far = dict(good, eye=np.asarray(good["eye"]) * 1e6)          # t ~ 3e6: a 0.01 step no longer moves it
    assert rc_ex(dict(far, stepSize=0.01)) == -5
    assert rc_ex(dict(good, voxelSize=(0.0, 0.01, 0.01))) == -5
    assert rc_ex(dict(good, voxelSize=(float("nan"), 0.01, 0.01))) == -5
    # the same gate guards the C5 passes
    P = params.brats_params(dict(good, stepSize=0.0))
    assert lib.mrirt_brats_sample_counts(C.byref(P), None, dummy, None) == -5
    assert b"argument" in lib.mrirt_status_string(-5).lower() or b"arg" in lib.mrirt_status_string(-5).lower()
    # K2: the loop count is uint(max(1, stepCount)); K3: maxSteps
    V = params.volume_params(synth.volume_scene(16, 32, 64))
    for bad in (float("nan"), float("inf"), 3e9):
        V.stepCount = bad
        assert lib.mrirt_render_volume(C.byref(V), None, dummy, 1, dummy, 32, None, None) == -5
    sp, eye, U, Vv, W = synth.sdf_scene()
    S = params.sdf_params(dict(sp, maxSteps=np.uint32(1 << 24)), eye, U, Vv, W)
    assert lib.mrirt_render_sdf(C.byref(S), 32, 32, dummy, 32, None) == -5


def test_torch_ops_refuse_operands_on_different_devices():
    """every device tensor of one operator call must live on one GPU (the launch then goes to THAT GPU's
    current stream).  The check itself needs no GPU: any two distinct torch devices exercise it."""
    import torch
    from mrirt import torch_ops
    a, b = torch.empty(1, device="meta"), torch.empty(1)
    assert torch_ops._one_device([("x", a), ("y", None), ("z", a)]) == a.device
    with pytest.raises(ValueError, match="same GPU"):
        torch_ops._one_device([("gIntensity0", a), ("gLabels", b)])
    with pytest.raises(ValueError):
        torch_ops._one_device([("x", None)])


def test_inline_asm_gathers_are_not_touched_before_their_wait():
    """The pipelined march kernels issue their gathers as inline asm, invisible to the compiler's wait insertion (and to its
    notion of "this register is still being loaded").  tools/check_async_loads.py walks the control-flow graph of every such
    kernel in the BUILT library and fails if any instruction reads or writes a gather destination that may be in flight."""
    import pathlib
    import subprocess
    import sys
    root = pathlib.Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "tools" / "check_async_loads.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-500:]
    assert "0 kernels failing" in r.stdout


def test_kernel_family_choices_incl_the_4gib_fallbacks():
    """mrirt_brats_kernel_family (host-only): the launches of the BASELINE configs take the kernels DESIGN.md names, and the
    configurations real volumes can reach beyond 32-bit offsets drop to the generic kernel: VG / QUAD grids
    >= 4 GiB (a 645^3 channel; 1024 x 1024 x 272), label grids >= 2^30 elements with an overlay shown, LINEAR grids >= 2^30
    voxels.  Skipping never applies to those."""
    from mrirt import render, synth
    fam = render.kernel_family
    c3 = synth.brats_scene(512, 1024, 512, channels=1, intensity_alpha=16.0)
    assert fam(c3, dict(synth.SHADE_EXT, layout="vga")) == {"family": "pipelined", "skipping": False, "label_cells": False}
    assert fam(c3, dict(synth.SHADE_EXT, layout="vga"), skip=True)["skipping"]
    assert fam(c3, dict(synth.SHADE_EXT, layout="vga", kernelVariant=64))["family"] == "slab"
    assert fam(c3, dict(synth.SHADE_EXT, layout="vga", kernelVariant=2048))["family"] == "ring"
    assert fam(c3, dict(synth.SHADE_EXT, layout="brick"))["family"] == "generic"
    c2 = synth.brats_scene(256, 512, 256, channels=4, show_seg=True, intensity_alpha=0.4)
    assert fam(c2, dict(layout="quad", labelLayout="labcell")) == {"family": "pipelined", "skipping": False, "label_cells": True}
    assert fam(c2, dict(layout="quad", labelLayout="brick"), skip=True) == {"family": "pipelined", "skipping": True, "label_cells": False}
    assert fam(c2, dict(layout="linear"))["family"] == "pipelined"                 # the plain ABI's own buffers
    # the four modalities as one float4 grid (MOD4): the pipelined march, with label cells, with skipping — whatever is enabled
    assert fam(c2, dict(layout="mod4", labelLayout="labcell")) == {"family": "pipelined", "skipping": False, "label_cells": True}
    assert fam(c2, dict(layout="mod4", labelLayout="brick"), skip=True) == {"family": "pipelined", "skipping": True, "label_cells": False}
    assert fam(dict(c2, volEnabled=(0, 0, 0, 0)), dict(layout="mod4"))["family"] == "pipelined"
    four = synth.brats_scene(256, 512, 256, channels=4)
    assert fam(four, dict(synth.SHADE_EXT, layout="vga"))["family"] == "rolling"
    assert fam(four, dict(synth.SHADE_EXT, layout="vga"), skip=True) == {"family": "rolling", "skipping": True, "label_cells": False}
    # FAST skips whatever gamma is; STRICT only at gamma == 1 (the skipping kernels specialise it)
    g08 = dict(c3, gamma=0.8)
    assert fam(g08, dict(synth.SHADE_EXT, layout="vg", math="fast"), skip=True) == {"family": "pipelined", "skipping": True, "label_cells": False}
    assert fam(g08, dict(synth.SHADE_EXT, layout="vg"), skip=True) == {"family": "pipelined", "skipping": False, "label_cells": False}
    assert fam(c2, dict(layout="quad", labelLayout="labcell", math="fast")) == {"family": "pipelined", "skipping": False, "label_cells": True}
    # a tile rank that owns no tile launches nothing
    tiles = synth.brats_scene(64, 64, 64, channels=1)
    assert fam(tiles, dict(layout="vg", tileSize=64, tileRank=1, tileWorld=2))["family"] == "none"
    assert fam(tiles, dict(layout="vg", tileSize=64, tileRank=0, tileWorld=2))["family"] == "pipelined"
    assert fam(dict(four, showSeg=1), dict(synth.SHADE_EXT, layout="vga"))["family"] == "generic"      # overlays: the generic kernel measured faster
    # ---- beyond 32-bit byte offsets ----
    wide = synth.brats_scene(0, 256, 200, dims=(1024, 1024, 272), channels=1)
    assert fam(wide, dict(synth.SHADE_EXT, layout="vg")) == {"family": "generic", "skipping": False, "label_cells": False}
    assert fam(wide, dict(synth.SHADE_EXT, layout="vg"), skip=True) == {"family": "generic", "skipping": False, "label_cells": False}
    assert fam(synth.brats_scene(645, 256, 200, channels=1), dict(layout="quad"))["family"] == "generic"
    assert fam(synth.brats_scene(644, 256, 200, channels=1), dict(layout="quad"))["family"] == "pipelined"     # 3.98 GiB: still 32-bit
    big = synth.brats_scene(1024, 128, 200, channels=1, show_seg=True)
    assert fam(big, dict(layout="linear"))["family"] == "generic"                  # 2^30 voxels, 2^30 label words
    huge_labels = synth.brats_scene(0, 128, 200, dims=(1024, 1024, 1020), channels=1, show_seg=True)
    assert fam(huge_labels, dict(layout="quad", labelLayout="brick"))["family"] == "generic"
    # ... so no map is built for them either: mrirt_brats_skip_applicable asks the launch's own plan
    for layout in ("quad", "vg"):
        assert _skip_applicable(huge_labels, dict(layout=layout, labelLayout="brick")) == 0
    assert _skip_applicable(c2, dict(layout="quad", labelLayout="brick")) == 1
    # VGA copies past 2^28 elements are refused outright (32-bit byte offsets inside a copy): an error, not a fault
    import pytest as _pt
    with _pt.raises(_lib_error()):
        fam(synth.brats_scene(0, 64, 64, dims=(1024, 1024, 272), channels=1), dict(synth.SHADE_EXT, layout="vga"))
    # MOD4 has the pipelined kernels only: shading, and grids from 4 GiB upwards, are refused (MRIRT_ERR_LAYOUT)
    with _pt.raises(_lib_error()):
        fam(c2, dict(synth.SHADE_EXT, layout="mod4"))
    with _pt.raises(_lib_error()):
        fam(synth.brats_scene(0, 64, 64, dims=(1024, 1024, 272), channels=4), dict(layout="mod4"))


def _skip_applicable(p, ext):
    """mrirt_brats_skip_applicable with every summary offered, placeholder addresses for the grids (as render.kernel_family)."""
    P, E = params.brats_params(p), params.render_ext(ext)
    fake = C.c_void_p(0x1000)
    vp = (C.c_void_p * 4)(*[fake if P.volEnabled[m] != 0 else None for m in range(4)])
    S = _lib.Skip()
    for m in range(4):
        S.macroUb[m] = 0x1000 if P.volEnabled[m] != 0 else None
    S.macroSeg = S.macroPred = 0x1000
    return int(_lib.lib().mrirt_brats_skip_applicable(C.byref(P), C.byref(E), vp, fake, fake, C.byref(S)))


def _lib_error():
    from mrirt import _lib
    return _lib.MrirtError
