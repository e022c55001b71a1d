"""The SIREN training step's index arithmetic and its sine on the CPU under AddressSanitizer + UBSan (the pattern of
test_inr_train_sanitizers.py).

``tests/native/inr_siren_harness.hip`` compiles csrc/inr_train.h and csrc/siren_sincos.h host-only as a stand-alone program
and replays the launches of one SIREN step for the shapes of inr_siren_cases.py over buffers of exactly the real sizes — the
scratch is exactly ``mrirt_siren_train_scratch_bytes``, cosines included.  Small shapes are also computed on selection nets and
compared bit for bit with the plain definition; then the sine runs over the edges of its domain and beyond under UBSan."""
import os
import pathlib
import shutil
import subprocess

import pytest

import inr_siren_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "inr_siren_harness"
    src = ROOT / "tests" / "native" / "inr_siren_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "inr_siren_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "inr_siren_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_siren_step_and_sine_under_asan_and_ubsan():
    exe = build_harness()
    raw = cases.KIND_RAW_SIREN
    # (in, hidden, layers, out, n, raw, compute): the exact cases' shapes at a small n, computed; the tolerance tier's shapes and
    # the timing tool's, addresses only; a slab length above the minimum
    shapes = sorted({(c["ind"], c["hidden"], c["layers"], c["out"], 65, int(c["kind"] == raw), 1) for c in cases.EXACT if c["hidden"] <= 64})
    shapes += sorted({(c["ind"], c["hidden"], c["layers"], c["out"], 65, int(c["kind"] == raw), 0) for c in cases.EXACT if c["hidden"] > 64})
    shapes += [(7, 32, 3, 4, cases.N, 0, 1), (65, 32, 2, 1, cases.N, 1, 1)]
    shapes += [(ind, hid, nh + 1, nc, n, int(kind == raw), 0) for kind, ind, hid, nh, nc, n in cases.E2E.values()]
    shapes += [(7, 256, 5, 4, 4096, 0, 0), (7, 32, 2, 4, 16385, 0, 0)]
    # the batch sweep's (shape, n) pairs, the head-coverage shapes and the beyond-the-domain net: addresses only
    shapes += [s for s in ((ind, hid, depth, out, n, int(kind == raw), 0) for kind, ind, hid, depth, out, _, n, _ in cases.BATCH) if s not in shapes]
    shapes += sorted({(c["ind"], c["hidden"], c["layers"], c["out"], cases.HEAD_N, 1, 0) for c in cases.HEAD_COVER})
    shapes += [(17, 64, 3, 4, cases.N, 1, 0)]
    args = [str(v) for s in shapes for v in s]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, env=env, timeout=900)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert f"inr_siren_harness: {len(shapes)} shapes, 0 failed, 0 sincos edges bad" in r.stdout, out[-6000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("shape ")]
    assert len(rows) == len(shapes) and all(row[-1] == "0" for row in rows)
