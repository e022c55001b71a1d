"""Class surfaces of label volumes (naive surface nets) without a GPU: the NumPy restatement against the values the definition
gives, the properties of every output, the kernels' per-thread text on the CPU under AddressSanitizer + UBSan
(tests/native/surface_harness.hip, built as test_hausdorff_host.py builds the distance transform's harness), the argument
checks of the C ABI (made before any HIP call) and the scratch formula."""
import ctypes as C
import inspect
import os
import pathlib
import shutil
import struct
import subprocess

import numpy as np
import pytest

import surface_cases as sc
import surface_ref as sr
import mrirt
from mrirt import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
CASES = sc.all_cases()
IDS = [c[0] for c in CASES]
f32 = np.float32


def _extract(case):
    name, lab, mask, sp, org, _ = case
    return sr.extract(lab, mask, sp, org)


def _by_name(name):
    return next(c for c in CASES if c[0] == name)


# --- the values the definition gives ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[5] is not None], ids=[c[0] for c in CASES if c[5] is not None])
def test_restatement_gives_the_listed_counts(case):
    v, t = _extract(case)
    print(case[0], len(v), len(t))
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape[1:] == (3,) and t.shape[1:] == (3,)
    assert (len(v), len(t)) == case[5]


def test_single_voxel_coordinates():
    v, t = _extract(_by_name("single_voxel"))
    lo, hi = f32(-1) + f32(5) / f32(6), f32(1) / f32(6)
    assert set(v.ravel().tolist()) == {float(lo), float(hi)}
    assert sorted(map(tuple, v.tolist())) == sorted((float(a), float(b), float(c)) for a in (lo, hi) for b in (lo, hi) for c in (lo, hi))


def test_all_inside_bounds():
    v, t = _extract(_by_name("all_inside_3x4x5"))
    assert v.min(axis=0).tolist() == [-0.5, -0.5, -0.5] and v.max(axis=0).tolist() == [2.5, 3.5, 4.5]


def test_ball_volume_and_voxel_count():
    lab = _by_name("ball_24x22x20")[1]
    assert int((lab == 1).sum()) == 1640
    v, t = sr.extract(lab, 0b10)
    assert round(sr.signed_volume(v, t) / 1640, 3) == 0.981
    v, t = sr.extract(lab, 0b10, sc.BALL_SPACING)
    assert round(sr.signed_volume(v, t) / (1640 * 1.25), 3) == 0.981


def test_large_case_has_the_listed_cells():
    assert sr.num_cells(sc.LARGE_SHAPE) == sc.LARGE_CELLS == 1204224
    assert sc.LARGE_CELLS > 1024 * 1024            # more than one chunk of chunk sums: the scan recurses


def test_cases_cover_what_they_should():
    odd = _by_name("odd_labels_0b10")[1]
    assert {-1, 32, 1000} <= set(odd.ravel().tolist())
    v1, t1 = sr.extract(odd, 0xFFFFFFFF)
    v2, t2 = sr.extract(np.where((odd >= 0) & (odd < 32), 1, 0).astype(np.int16), 0b10)
    assert np.array_equal(v1, v2) and np.array_equal(t1, t2)          # -1, 32 and 1000 are outside under every mask
    assert _by_name("thin_1x7x1")[1].shape == (1, 7, 1) and _by_name("thin_5x1x1")[1].shape == (5, 1, 1)
    six = sr.inside(_by_name("six_faces")[1], 0b100)
    assert all(six.take(i, axis=k).any() for k in range(3) for i in (0, -1))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_properties_of_every_output(case):
    v, t = _extract(case)
    assert sr.is_closed(t)
    if len(t):
        assert t.min() >= 0 and t.max() < len(v) and len(np.unique(t)) == len(v)
        assert sr.signed_volume(v, t) > 0
    else:
        assert len(v) == 0
    if case[0].startswith("ball"):
        assert sr.euler(v, t) == 2


# --- the Python names ---------------------------------------------------------------------------------------------------
def test_python_names_have_the_documented_signatures():
    sig = inspect.signature(mrirt.mesh.extract_surface)
    assert list(sig.parameters) == ["labels", "classes", "spacing", "origin", "stream"]
    assert sig.parameters["spacing"].default == (1, 1, 1) and sig.parameters["origin"].default == (0, 0, 0)
    assert sig.parameters["stream"].default is None
    sig = inspect.signature(mrirt.mesh.surface_mesh)
    assert list(sig.parameters) == ["labels", "classes", "spacing", "origin", "max_leaf_tris"]
    assert sig.parameters["max_leaf_tris"].default == 4
    assert mrirt.extract_surface is mrirt.mesh.extract_surface and mrirt.surface_mesh is mrirt.mesh.surface_mesh
    for s in ("mrirt_surface_scratch_bytes", "mrirt_surface_count", "mrirt_surface_extract"):
        assert s in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), s)
    assert "surface.hip" in _lib.HIP_SOURCES and _lib.lib().mrirt_abi_version() == 4
    assert mrirt.mesh.class_mask(3) == 8 and mrirt.mesh.class_mask((1, 2, 3)) == 0b1110 and mrirt.mesh.class_mask([0, 31]) == 0x80000001
    for bad in (-1, 32, (1, 40)):
        with pytest.raises(ValueError):
            mrirt.mesh.class_mask(bad)


def test_torch_operators_have_static_shapes_from_their_ints():
    import torch
    from mrirt import torch_ops  # noqa: F401  (registers torch.ops.mrirt.*)
    lab = torch.empty((5, 6, 7), dtype=torch.int16, device="meta")
    assert tuple(torch.ops.mrirt.surface_count(lab, 2).shape) == (2,) and torch.ops.mrirt.surface_count(lab, 2).dtype == torch.int64
    v, t = torch.ops.mrirt.surface_extract(lab, 2, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], 11, 22)
    assert (tuple(v.shape), v.dtype, tuple(t.shape), t.dtype) == ((11, 3), torch.float32, (22, 3), torch.int32)


# --- the C ABI without a device -------------------------------------------------------------------------------------------
def _hwd(*v):
    return (C.c_uint32 * 3)(*v)


def _f3(*v):
    return (C.c_float * 3)(*v)


def test_abi_rejects_malformed_arguments_before_any_hip_call():
    """Host memory stands in for the device buffers: every call below must return before anything is launched or read."""
    l = _lib.lib()
    buf = C.create_string_buffer(8192)
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)
    ok_hwd, ok_sp, ok_org = _hwd(4, 4, 4), _f3(1, 1, 1), _f3(0, 0, 0)
    big = 1 << 40

    def count(lab=p, hwd=ok_hwd, scratch=p, nbytes=big, counts=p):
        return l.mrirt_surface_count(lab, hwd, 2, scratch, nbytes, counts, None)

    def extract(lab=p, hwd=ok_hwd, sp=ok_sp, org=ok_org, verts=p, vcap=8, tris=p, tcap=8, scratch=p, nbytes=big, counts=p):
        return l.mrirt_surface_extract(lab, hwd, 2, sp, org, verts, vcap, tris, tcap, scratch, nbytes, counts, None)

    NULL, DIMS, ARG = -1, -2, -5
    for kw in ("lab", "hwd", "scratch", "counts"):
        assert count(**{kw: None}) == NULL, kw
    for kw in ("lab", "hwd", "sp", "org", "verts", "tris", "scratch", "counts"):
        assert extract(**{kw: None}) == NULL, kw
    for bad in (_hwd(0, 4, 4), _hwd(4, 0, 4), _hwd(4, 4, 0)):
        assert count(hwd=bad) == DIMS and extract(hwd=bad) == DIMS, list(bad)
        assert l.mrirt_surface_scratch_bytes(bad) == 0
    # (n0+1)(n1+1)(n2+1) must stay below 2^31
    for bad in (_hwd(2047, 1023, 1023), _hwd(0xFFFFFFFF, 1, 1), _hwd(1, 0xFFFFFFFF, 0xFFFFFFFF), _hwd(1 << 30, 1, 1), _hwd(1290, 1290, 1290)):
        assert count(hwd=bad) == ARG and extract(hwd=bad) == ARG, list(bad)
        assert l.mrirt_surface_scratch_bytes(bad) == 0
    assert l.mrirt_surface_scratch_bytes(_hwd(2046, 1023, 1023)) > 0 and l.mrirt_surface_scratch_bytes(_hwd(1289, 1289, 1289)) > 0
    for bad in (_f3(float("nan"), 1, 1), _f3(1, float("inf"), 1), _f3(1, 1, float("-inf")), _f3(0, 1, 1), _f3(1, -1, 1), _f3(1, 1, -0.0)):
        assert extract(sp=bad) == ARG, list(bad)
    for bad in (_f3(float("nan"), 0, 0), _f3(0, float("inf"), 0), _f3(0, 0, float("-inf"))):
        assert extract(org=bad) == ARG, list(bad)
    need = l.mrirt_surface_scratch_bytes(ok_hwd)
    for fn in (count, extract):
        assert fn(nbytes=need - 1) == ARG and fn(nbytes=0) == ARG and fn(nbytes=-1) == ARG
        assert fn(scratch=C.c_void_p(p.value + 4)) == ARG                   # the scratch must be 16-byte aligned
    assert extract(vcap=-1) == ARG and extract(tcap=-1) == ARG
    assert l.mrirt_surface_scratch_bytes(None) == 0


def _scratch_formula(shape, chunk=1024):
    """code: one byte per cell in whole chunks; vidx: 4 B per cell; 16 B per chunk at every level until one chunk holds a
    level; every part rounded up to 256 B."""
    def al(x):
        return (x + 255) // 256 * 256
    cells = sr.num_cells(shape)
    n = -(-cells // chunk)
    total = al(n * chunk) + al(4 * cells) + al(16 * n)
    while n > chunk:
        n = -(-n // chunk)
        total += al(16 * n)
    return total


def test_scratch_bytes_formula():
    l = _lib.lib()
    shapes = [(1, 1, 1), (1, 7, 1), (5, 1, 1), (9, 6, 5), (24, 22, 20), (31, 31, 31), (127, 97, 95), (240, 240, 155), (1023, 1023, 1023),
              (2046, 1023, 1023)]
    sizes = [l.mrirt_surface_scratch_bytes(_hwd(*s)) for s in shapes]
    for s, v in zip(shapes, sizes):
        assert v == _scratch_formula(s) and v >= 5 * sr.num_cells(s), s
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))


# --- the per-thread text under the sanitizers -----------------------------------------------------------------------------
def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "surface_harness"
    src = ROOT / "tests" / "native" / "surface_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "surface_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "surface_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


def _fnv(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_cell_text_under_asan_and_ubsan_equals_the_restatement(tmp_path):
    exe = build_harness()
    blob = struct.pack("<I", len(CASES))
    for name, lab, mask, sp, org, _ in CASES:
        blob += struct.pack("<4I6f", *lab.shape, mask, *sp, *org) + np.ascontiguousarray(lab, dtype=np.int16).tobytes()
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "FAILED" not in out, out[-6000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"surface_harness: {len(CASES)} cases done" and len(lines) == 3 * len(CASES) + 1
    l = _lib.lib()
    for k, case in enumerate(CASES):
        name, lab = case[0], case[1]
        head, vline, tline = (ln.split() for ln in lines[3 * k:3 * k + 3])
        want_v, want_t = _extract(case)
        # the buffer the harness ran in (ASan-checked, exactly this long) is what the ABI tells callers to allocate
        assert int(head[3]) == l.mrirt_surface_scratch_bytes(_hwd(*lab.shape)), name
        assert (int(head[7]), int(head[9])) == (len(want_v), len(want_t)), name
        if vline[0] == "v":
            got_v = np.array([int(w, 16) for w in vline[1:]], dtype=np.uint32).view(np.float32).reshape(-1, 3)
            got_t = np.array([int(w) for w in tline[1:]], dtype=np.int32).reshape(-1, 3)
            assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), f"{name}: harness vertices differ from the restatement"
            assert np.array_equal(got_t, want_t), f"{name}: harness triangles differ from the restatement"
        else:
            assert name == "ball_127x97x95" and int(head[5]) == 2              # sums of chunk sums: the scan recursed
            assert int(vline[1], 16) == _fnv(np.ascontiguousarray(want_v).tobytes()), f"{name}: harness vertices differ"
            assert int(tline[1], 16) == _fnv(np.ascontiguousarray(want_t).tobytes()), f"{name}: harness triangles differ"
