"""The INR training kernels' index arithmetic on the CPU under AddressSanitizer + UBSan (as test_brats_grad_sanitizers.py for
the K1 backward pass).

csrc/inr_train.h holds the tile, tail and slab arithmetic and the scratch layout as ``MRIRT_HD`` functions;
``tests/native/inr_train_harness.hip`` compiles it host-only as a stand-alone program and replays the launches of one step
for every shape of inr_train_cases.py over buffers of exactly the real sizes.  The exact shapes are also computed (integer
data, the MFMA as its definition) and compared with a plain triple loop; the end-to-end shapes walk the addresses only."""
import os
import pathlib
import shutil
import subprocess

import pytest

import inr_train_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "inr_train_harness"
    src = ROOT / "tests" / "native" / "inr_train_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "inr_train_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "inr_train_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_index_arithmetic_under_asan_and_ubsan():
    exe = build_harness()
    shapes = [(ind, hid, depth, out, n, 1) for ind, hid, depth, out, n, _ in cases.EXACT]
    shapes += [(3 + 6 * K + M, hid, nh + 1, nc, n, 0) for K, M, hid, nh, nc, n in cases.E2E.values()]
    shapes += [(31, 64, 5, 4, 4096, 0), (7, 32, 2, 1, 16385, 0)]          # the timing tool's small shape; the first n with longer slabs
    shapes += [(ind, hid, depth, out, n, 0) for ind, hid, depth, out, n, _ in cases.BATCH if ind == 7]     # every slab length up to 4096
    args = [str(v) for s in shapes for v in s]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert f"inr_train_harness: {len(shapes)} shapes, 0 failed" in r.stdout, out[-6000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("shape ")]
    assert len(rows) == len(shapes) and all(row[-1] == "0" for row in rows)
