"""Muon's index arithmetic on the CPU under AddressSanitizer + UBSan (as test_inr_loop_sanitizers.py for the training loop).

csrc/inr_muon.h holds the per-layer table, the strided operand views of the three Newton-Schulz products, the element -> layer
lookup and the scratch layout as ``MRIRT_HD`` functions; ``tests/native/inr_muon_harness.hip`` compiles it host-only as a
stand-alone program and replays mrirt_muon_orthogonalize for network shapes of inr_muon_cases.py over buffers of exactly the
real sizes, comparing the result with plain loops over explicit (transposed) matrices.  No sanitizer is loaded into Python."""
import os
import pathlib
import shutil
import subprocess

import pytest

import inr_muon_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "inr_muon_harness"
    src = ROOT / "tests" / "native" / "inr_muon_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "inr_muon_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "inr_muon_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_index_arithmetic_under_asan_and_ubsan():
    exe = build_harness()
    # every exact shape but the widest (one step each: the indices do not depend on the step), the smaller tolerance shapes in
    # full, and the widest hidden layer once
    shapes = [(c["dims"], 1) for c in cases.EXACT if max(c["dims"]) < 256]
    shapes += [(cases.TOL_NETS["103x64x64x4"], 5), (cases.TOL_NETS["65x32x32x32x16"], 2), ([7, 256, 256, 4], 1), ([128, 256, 1], 2)]
    args = []
    for dims, steps in shapes:
        args += ["n", dims[0], dims[1], len(dims) - 1, dims[-1], steps]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert f"inr_muon_harness: {len(shapes)} items, 0 failed" in r.stdout, out[-6000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("item done")]
    assert len(rows) == len(shapes) and all(row[-1] == "0" for row in rows)
