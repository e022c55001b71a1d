"""The index arithmetic of the K1 march on the CPU under AddressSanitizer + UBSan (VERDICT r3 #1b).

GPU sanitizers are not available on the pool, so the part of the kernels that can fault — which element, byte, pixel or map
cell an id turns into — is compiled for the host as well (``MRIRT_HD`` functions in csrc/mrirt_device.h / skip_map.h) and
``tests/native/index_harness.hip`` walks it against buffers of exactly the sizes the host wrappers allocate: every tap of every
layout for every admissible base cell, the workgroup/lane -> pixel map of frames and tile shards, the skipping pre-pass with
its ballot words and byte maps, MapWindow's window moves, and the host halves of ``mrirt_render_brats_skip`` / ``_ex`` for the
launch whose synchronisation aborted once in round 3 (72^3, QUAD, 3 channels, 160^2, both showSeg values).  The harness
includes the library's headers (csrc/brats_host.h, csrc/skip_map.h) and links the library's own sources, compiled host-only
(``hipcc --offload-host-only``) under the same sanitizers, so it checks the product's code, not a copy."""
import os
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "mri-raytracer_amd" / "csrc"
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "index_harness"
    srcs = [ROOT / "tests" / "native" / "index_harness.hip"] + [
        CSRC / s for s in ("brats_march.hip", "brats_skip.hip", "brats_c5.hip", "brats_slab.hip", "brats_ring.hip", "grid_ops.hip", "inr_mlp.hip", "inr_stream.hip",
                             "inr_ws.hip", "inr_refine.hip")]
    deps = srcs + list(CSRC.glob("*.h")) + [ROOT / "include" / "mrirt.h"]
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    objs = []
    procs = []
    for s in srcs:
        o = OUT / (s.name + ".o")
        objs.append(o)
        procs.append(subprocess.Popen([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                                       "-c", str(s), "-o", str(o)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, out[-4000:]
    # A host-only object still refers to the device image of its translation unit (`__hip_fatbin_<id>`, registered by a
    # constructor).  There is none: give each an empty one, so the program links and the runtime finds no kernels — the
    # harness never launches successfully (it has no GPU), it only runs the host code.
    syms = []
    for o in objs:
        nm = subprocess.run(["nm", str(o)], capture_output=True, text=True, check=True).stdout
        syms += [ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln]
    stub = OUT / "no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in sorted(set(syms))))
    r = subprocess.run([HIPCC, *SAN, "-w", *map(str, objs), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_index_arithmetic_under_asan_and_ubsan():
    exe = build_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=900)
    tail = (r.stdout + r.stderr)[-6000:]
    assert r.returncode == 0, tail
    assert "runtime error" not in tail and "AddressSanitizer" not in tail, tail
    assert "index_harness:" in r.stdout and " 0 failed" in r.stdout, tail
