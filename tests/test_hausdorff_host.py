"""Hausdorff distance / exact distance transform without a GPU: the definition against the reference's recorded values, the
argument checks of the C ABI (made before any HIP call), the scratch formula, and the kernels' per-thread text on the CPU
under AddressSanitizer + UBSan (tests/native/edt_harness.hip, built as test_mesh_sanitizers.py builds the mesh harness)."""
import ctypes as C
import inspect
import os
import pathlib
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hausdorff_cases as hc
import hausdorff_ref as href
from mrirt import _lib, inr

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
CASES = hc.load_cases()
MAX_LINE = 4096


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_the_reference(case):
    name, pred, true, spacing, nc, want = case
    got = href.hausdorff(pred, true, spacing, nc)
    print(name, [got[c] for c in range(nc)], list(want))
    for c in range(nc):
        assert hc.same(got[c], want[c]), f"{name} class {c}: restatement {got[c]!r}, reference {float(want[c])!r}"


def test_fixture_covers_what_it_should():
    by = {c[0]: c for c in CASES}
    assert len(CASES) >= 12 and all(max(c[1].shape) <= 40 for c in CASES if c[0] != "medium_blob")
    assert by["medium_blob"][1].shape == (96, 96, 62)
    assert {c[3] for c in CASES} >= {(1.0, 1.0, 1.0), (1.0, 1.0, 2.5), (0.9375, 1.1, 1.3), (0.7, 0.7, 3.3)}
    assert np.isnan(by["absent_in_pred_only"][5][3]) and (by["absent_in_pred_only"][2] == 3).any()
    assert list(by["identical"][5][:4]) == [0.0] * 4
    assert int((by["one_voxel_class"][2] == 3).sum()) == 1
    assert 1 in by["thin_axis1"][1].shape
    assert by["labels_outside_classes"][1].max() >= by["labels_outside_classes"][4] and by["labels_outside_classes"][1].min() < 0


def test_large_case_volumes_rebuild_to_their_crc():
    shape, spacing, nc, crc_p, crc_t, want = hc.load_large()
    assert shape[0] >= 128 and shape[1] >= 128 and shape[2] >= 96
    pred, true = hc.large_pair(shape)
    assert (hc.crc(pred), hc.crc(true)) == (crc_p, crc_t)
    assert all(np.isfinite(want)) and len(want) == nc


def test_python_names_have_the_reference_signatures():
    sig = inspect.signature(inr.hausdorff_distance)
    assert list(sig.parameters) == ["pred", "true", "spacing", "num_classes"]
    assert sig.parameters["spacing"].default == (1.0, 1.0, 1.0) and sig.parameters["num_classes"].default == 4
    assert list(inspect.signature(inr.evaluate_single_case).parameters) == ["case_idx", "case_data", "params", "num_classes", "fourier_freqs"]
    assert list(inspect.signature(inr.distance_transform).parameters) == ["mask_or_labels", "cls", "spacing"]
    for s in ("mrirt_edt_scratch_bytes", "mrirt_edt_squared", "mrirt_hausdorff"):
        assert s in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), s)
    assert _lib.lib().mrirt_abi_version() == 4


def _hwd(*v):
    return (C.c_uint32 * 3)(*v)


def _sp(*v):
    return (C.c_float * 3)(*v)


def test_abi_rejects_malformed_arguments_before_any_hip_call():
    """Host memory stands in for the device buffers: every call below must return before anything is launched or read."""
    l = _lib.lib()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    ok_hwd, ok_sp = _hwd(4, 4, 4), _sp(1, 1, 1)
    big = 1 << 40

    def hd(pred=p, truth=p, hwd=ok_hwd, sp=ok_sp, nc=4, out=p, scratch=p, nbytes=big):
        return l.mrirt_hausdorff(pred, truth, hwd, sp, nc, out, scratch, nbytes, None)

    def edt(lab=p, hwd=ok_hwd, sp=ok_sp, out=p, scratch=p, nbytes=big):
        return l.mrirt_edt_squared(lab, hwd, 1, sp, out, scratch, nbytes, None)

    NULL, DIMS, ARG = -1, -2, -5
    for kw in ("pred", "truth", "hwd", "sp", "out", "scratch"):
        assert hd(**{kw: None}) == NULL, kw
    for kw in ("lab", "hwd", "sp", "out", "scratch"):
        assert edt(**{kw: None}) == NULL, kw
    for bad in (_hwd(0, 4, 4), _hwd(4, 0, 4), _hwd(4, 4, 0), _hwd(2048, 1024, 1024), _hwd(4096, 4096, 128), _hwd(MAX_LINE + 1, 1, 1),
                _hwd(1, 1, MAX_LINE + 1), _hwd(1, 0xFFFFFFFF, 1)):
        assert hd(hwd=bad) == DIMS and edt(hwd=bad) == DIMS, list(bad)
        assert l.mrirt_edt_scratch_bytes(bad, 4) == 0
    for nc in (0, 33, 1 << 20):
        assert hd(nc=nc) == ARG, nc
    assert l.mrirt_edt_scratch_bytes(ok_hwd, 33) == 0
    for bad in (_sp(float("nan"), 1, 1), _sp(1, float("inf"), 1), _sp(1, 1, float("-inf")), _sp(3e38, 1, 1)):
        assert hd(sp=bad) == ARG and edt(sp=bad) == ARG, list(bad)
    need = l.mrirt_edt_scratch_bytes(ok_hwd, 4)
    assert hd(nbytes=need - 1) == ARG and hd(nbytes=0) == ARG and hd(nbytes=-1) == ARG
    assert edt(nbytes=l.mrirt_edt_scratch_bytes(ok_hwd, 0) - 1) == ARG
    assert l.mrirt_edt_scratch_bytes(None, 4) == 0


def test_scratch_bytes_is_monotone_in_the_volume_size():
    l = _lib.lib()
    shapes = [(1, 1, 1), (1, 1, 17), (2, 3, 4), (24, 1, 20), (40, 36, 30), (96, 96, 62), (240, 240, 155), (512, 512, 512),
              (4096, 1, 1), (4096, 4096, 127)]
    shapes.sort(key=lambda s: s[0] * s[1] * s[2])
    for nc in (1, 4, 32):
        sizes = [l.mrirt_edt_scratch_bytes(_hwd(*s), nc) for s in shapes]
        assert all(v > 0 for v in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), (nc, sizes)
        for s, v in zip(shapes, sizes):                       # two fp64 fields and the per-class accumulators
            assert v >= 16 * s[0] * s[1] * s[2] + 32 * nc
    for s in shapes:
        assert l.mrirt_edt_scratch_bytes(_hwd(*s), 1) <= l.mrirt_edt_scratch_bytes(_hwd(*s), 32)
        assert 0 < l.mrirt_edt_scratch_bytes(_hwd(*s), 0) <= 64           # mrirt_edt_squared runs in place in its output


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "edt_harness"
    src = ROOT / "tests" / "native" / "edt_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "edt_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "edt_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


def _longest_line_case():
    """One line of the longest supported length (4096 x 1 x 1) and the same along the last axis, sparse labels."""
    rng = np.random.default_rng(4096)
    out = []
    for shape, sp in (((MAX_LINE, 1, 1), (0.7, 1.0, 1.0)), ((1, 1, MAX_LINE), (1.0, 1.0, 1.3)), ((1, MAX_LINE, 2), (1.0, 0.9375, 1.0))):
        a, b = (np.where(rng.random(shape) < 0.98, 0, rng.integers(1, 3, shape)).astype(np.int16) for _ in range(2))
        out.append((f"line{shape}", a, b, sp, 3, None))
    return out


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_line_pass_under_asan_and_ubsan(tmp_path):
    exe = build_harness()
    cases = [c for c in CASES if c[0] != "medium_blob"] + _longest_line_case()
    blob = struct.pack("<I", len(cases))
    for name, pred, true, sp, nc, _ in cases:
        blob += struct.pack("<4I3f", *pred.shape, nc, *sp)
        blob += np.ascontiguousarray(pred, dtype=np.int16).tobytes() + np.ascontiguousarray(true, dtype=np.int16).tobytes()
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, env=env, timeout=900)
    out = r.stdout + r.stderr
    print(out[-6000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "FAILED" not in out, out[-6000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert len(lines) == len(cases) and f"edt_harness: {len(cases)} cases done" in r.stdout
    l = _lib.lib()
    for ln, (name, pred, true, sp, nc, want) in zip(lines, cases):
        # the buffer the harness ran in (ASan-checked, exactly this long) is what the ABI tells callers to allocate
        assert int(ln[3]) == l.mrirt_edt_scratch_bytes(_hwd(*pred.shape), nc), name
        if want is None:
            ref = href.hausdorff(pred, true, sp, nc)
            want = [ref[c] for c in range(nc)]
        got = [float("nan") if tok == "nan" else struct.unpack("<d", struct.pack("<Q", int(tok, 16)))[0] for tok in ln[5:]]
        assert len(got) == nc
        for c in range(nc):
            assert hc.same(got[c], want[c]), f"{name} class {c}: harness {got[c]!r}, expected {float(want[c])!r}"
