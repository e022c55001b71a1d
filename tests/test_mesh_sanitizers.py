"""The K4 traversal's index and stack handling on the CPU under AddressSanitizer + UBSan (as test_index_sanitizers.py for K1).

csrc/mesh_trace.h holds the traversal the kernel runs as ``MRIRT_HD`` functions; ``tests/native/mesh_harness.hip`` compiles
it host-only and walks it over the reference's BVH of the 1 280-triangle icosphere and over malformed copies of it (child
out of range, negative and huge leaf counts, a triangle index >= vertCount, cycles, a stack shallower than the tree, NaN
boxes and indices), with every buffer exactly its count long.  No invalid access, every ray ends, and on malformed buffers
the fault status is raised.  Malformed buffers never reach the GPU."""
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from mesh_cases import fixture
from mrirt import mesh

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "mesh_harness"
    src = ROOT / "tests" / "native" / "mesh_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "mesh_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "mesh_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_mesh_traversal_under_asan_and_ubsan(tmp_path):
    exe = build_harness()
    f = fixture("ico3")
    tris, verts = mesh.pack_tris(f["bvh_tris"]), mesh.pack_verts(f["bvh_verts"])
    depth = mesh.validate_bvh(f["nodes"], tris, len(verts))
    paths = []
    for name, arr in (("nodes", f["nodes"].astype(np.float32)), ("tris", tris.astype(np.uint32)), ("verts", verts)):
        p = tmp_path / f"{name}.bin"
        p.write_bytes(np.ascontiguousarray(arr).tobytes())
        paths.append(str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), *paths, str(depth)], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert "mesh_harness:" in r.stdout and " 0 failed" in r.stdout, out[-6000:]
