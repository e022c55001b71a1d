"""The index arithmetic of the extended loss, the tumour index and the mixed sampler on the CPU under AddressSanitizer + UBSan
(as test_inr_muon_sanitizers.py for Muon).

csrc/inr_lossx.h holds the partial-sum layout, the chunking of the compaction, the voxel decode and the mixed draw as
``MRIRT_HD`` functions; ``tests/native/inr_lossx_harness.hip`` compiles it host-only as a stand-alone program and replays the
launches over buffers of exactly the real sizes: n on both sides of 256 x 256 points, volumes that are no multiple of the
4096-voxel chunk, and (arithmetic only) volumes with H W D just below 2^32.  No sanitizer is loaded into Python."""
import os
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]

ITEMS = [["l", 1], ["l", 255], ["l", 257], ["l", 65535], ["l", 65536], ["l", 65537], ["l", 65836], ["l", 131073],
         ["t", 4, 5, 7, 9], ["t", 4, 17, 16, 17], ["t", 5, 67, 66, 65], ["t", 3, 16, 16, 16], ["t", 1, 2, 2, 2], ["t", 4, 64, 64, 257],
         ["m", 4, 5, 7, 9, 1000, 500], ["m", 4, 17, 16, 17, 1000, 1000], ["m", 5, 67, 66, 65, 255, 1], ["m", 1, 2, 2, 2, 300, 300], ["big"]]


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "inr_lossx_harness"
    src = ROOT / "tests" / "native" / "inr_lossx_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "inr_lossx_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "inr_lossx_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_index_arithmetic_under_asan_and_ubsan():
    exe = build_harness()
    args = [str(a) for item in ITEMS for a in item]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert f"inr_lossx_harness: {len(ITEMS)} items, 0 failed" in r.stdout, out[-6000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("item ")]
    assert len(rows) == len(ITEMS) and all(row[-1] == "0" for row in rows)
    used = [int(ln.split()[ln.split().index("index") + 1]) for ln in r.stdout.splitlines() if ln.startswith("item m")]
    assert all(u > 0 for u in used[:3]) and used[3] == 0          # the last cache is one empty case: every tumour draw falls back
