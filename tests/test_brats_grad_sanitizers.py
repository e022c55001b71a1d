"""The K1 backward pass's per-sample math on the CPU under AddressSanitizer + UBSan (as test_mesh_sanitizers.py for K4).

csrc/brats_grad.h holds what one sample contributes — the derivative chain, the eight corner weights, the corner indices with
their clamps — as ``MRIRT_HD`` functions; ``tests/native/brats_grad_harness.hip`` compiles it host-only as a stand-alone program
and walks every sample of every case of brats_grad_cases.py, with every gradient buffer exactly the grid's size.  No invalid
access, and the per-case sums it prints equal the fp64 reference's closed form."""
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import brats_grad_cases as bc
import brats_grad_ref as ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "brats_grad_harness"
    src = ROOT / "tests" / "native" / "brats_grad_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "brats_grad_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "brats_grad_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_per_sample_math_under_asan_and_ubsan(tmp_path):
    exe = build_harness()
    paths, want = [], []
    for c in bc.CASES:
        d = bc.data(c["name"])
        cf = ref.closed_form(c, d)
        p = c["params"]
        hdr = [*c["dims"], len(cf.samples), *p["volEnabled"], *[np.float32(w) for w in p["volWeight"]],
               *[np.float32(p[k]) for k in ("ww", "wl", "intensityAlpha", "gamma", "stepSize")], np.float32(cf.rec.wsum)]
        f = tmp_path / f"{c['name']}.bin"
        f.write_bytes(np.concatenate([np.asarray(hdr, np.float64), cf.samples.reshape(-1)]).tobytes())
        paths.append(str(f))
        want.append(cf)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), *paths], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert f"brats_grad_harness: {len(bc.CASES)} cases, 0 failed" in r.stdout, out[-6000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert len(rows) == len(bc.CASES)
    for c, cf, row in zip(bc.CASES, want, rows):
        assert int(row[3]) == len(cf.samples), c["name"]
        for m in range(4):
            got = [float(x) for x in row[7 + 4 * m: 10 + 4 * m]]
            g = cf.grad_vols[m]
            if g is None:
                assert got == [0.0, 0.0, 0.0], (c["name"], m)
                continue
            key = (np.arange(g.size, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1021)
            scale = cf.A_vols[m].sum()
            # the harness rounds the corner weights to fp32 (as the kernel does): 8 products of three fp32 factors, 2^-22 of A
            assert abs(got[0] - g.sum()) <= 1e-6 * scale, (c["name"], m, got[0], g.sum())
            assert abs(got[1] - np.abs(g).sum()) <= 1e-6 * scale, (c["name"], m)
            assert abs(got[2] - float((g * key.astype(np.float64)).sum())) <= 1e-6 * scale * 1021, (c["name"], m)
        got_tf = np.array([float(x) for x in row[-4:]])
        # (v and T reach the chain as the forward's fp32 values: 2^-24 relative per sample)
        assert np.all(np.abs(got_tf - cf.grad_tf) <= 1e-6 * cf.A_tf + 1e-300), (c["name"], got_tf, cf.grad_tf)
