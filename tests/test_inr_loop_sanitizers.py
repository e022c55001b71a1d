"""The INR training loop's index arithmetic on the CPU under AddressSanitizer + UBSan (as test_inr_train_sanitizers.py for the
training step).

csrc/inr_optim.h holds the Philox draw, mulhi32, the 64-bit voxel offsets, the norm pass's block-to-range assignment, the
update's float4 / scalar units and the scratch layout of a run as ``MRIRT_HD`` functions; ``tests/native/inr_loop_harness.hip``
compiles it host-only as a stand-alone program and replays the sampler, the norm pass and the update for every case of
inr_loop_cases.py over buffers of exactly the real sizes, walks the offsets of volumes just under 2^31 elements, and
compares Philox with its known answers.  No sanitizer is loaded into Python."""
import os
import pathlib
import shutil
import subprocess

import pytest

import inr_loop_cases as cases

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "inr_loop_harness"
    src = ROOT / "tests" / "native" / "inr_loop_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "inr_loop_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "inr_loop_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_index_arithmetic_under_asan_and_ubsan():
    exe = build_harness()
    args, items = [], 0
    for name in cases.SAMPLER_CACHES + ["run"]:
        ncases, M, (H, W, D) = cases.cache_shape(name)
        for n in cases.BATCH_SIZES + ([cases.RUN_NET["micro"]] if name == "run" else []):
            args += ["s", ncases, M, H, W, D, n]
            items += 1
    args += ["s", 2, 4, 16, 16, 16, cases.E2E_CONFIG["MICRO_BATCH_SIZE"]]
    items += 1
    for n in cases.ADAMW_SIZES + [cases.ADAMW_FLOAT_N]:
        args += ["o", *cases.adamw_split(n)]
        items += 1
    args += ["o", 1, 0, "o", 4, 0, "o", 1000, 3]
    net = cases.RUN_NET
    args += ["r", 3 + 6 * net["K"] + net["M"], net["hidden"], net["hidden_layers"] + 1, net["classes"], net["micro"], net["M"]]
    args += ["r", 31, 64, 5, 4, 4096, 4, "r", 15, 32, 3, 4, 1, 0, "big"]                  # the timing tool's small shape; one point, no modality
    items += 7
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert "philox known answers: mismatches 0" in r.stdout
    assert f"inr_loop_harness: {items} items, 0 failed" in r.stdout, out[-6000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("item ")]
    assert len(rows) == items and all(row[-1] == "0" for row in rows)
