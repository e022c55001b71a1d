"""The soft prediction overlay's per-sample chain on the CPU under AddressSanitizer + UBSan (as test_brats_grad_sanitizers.py).

csrc/brats_soft.h holds what one sample contributes — softmax, sigma, E, alpha, c and the four derivative lines — as ``MRIRT_HD``
functions; ``tests/native/brats_soft_harness.hip`` compiles it host-only as a stand-alone program and walks every logits row and
every recorded event of every case of brats_soft_cases.py, each row in a buffer of exactly C floats.  No invalid access, and
the per-case sums it prints equal the fp64 reference's.  Nothing is loaded into Python."""
import os
import pathlib
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

import brats_soft_cases as sc
import brats_soft_ref as ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]

warnings.filterwarnings("ignore", message="The given NumPy array is not writable")


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "brats_soft_harness"
    src = ROOT / "tests" / "native" / "brats_soft_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "brats_soft_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "brats_soft_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_per_sample_chain_under_asan_and_ubsan(tmp_path):
    exe = build_harness()
    paths, want = [], []
    for c in sc.CASES:
        d = sc.data(c["name"])
        cf = ref.closed_form(c, d, geo=sc.geo(c["name"]))
        lut = np.asarray(c["params"]["lutColorAlpha"], np.float32).reshape(8, 4)
        hdr = [c["classes"], d["logits"].shape[0], len(cf.samples), cf.rec.Dp, *lut.reshape(-1)]
        f = tmp_path / f"{c['name']}.bin"
        f.write_bytes(np.concatenate([np.asarray(hdr, np.float64), d["logits"].astype(np.float64).reshape(-1), cf.samples.reshape(-1)]).tobytes())
        paths.append(str(f))
        _, _, has, alpha, col = ref.soft_event(torch.from_numpy(d["logits"].astype(np.float64)), lut, cf.rec.Dp)
        want.append((cf, int(has.sum()), float(alpha.numpy().astype(np.float32).astype(np.float64).sum()),
                     float(col.numpy().astype(np.float32).astype(np.float64).sum())))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), *paths], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
    assert f"brats_soft_harness: {len(sc.CASES)} cases, 0 failed" in r.stdout, out[-6000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert len(rows) == len(sc.CASES)
    for c, (cf, events, alpha, col), row in zip(sc.CASES, want, rows):
        name = c["name"]
        assert int(row[3]) == c["classes"] and int(row[5]) == sc.data(name)["logits"].shape[0], name
        assert int(row[7]) == events, name
        # alpha and c are rounded once to fp32 on both sides; their fp64 values agree to a few ulp, so a sum of n of them to n 2^-24
        assert abs(float(row[9]) - alpha) <= 1e-6 * max(events, 1) and abs(float(row[11]) - col) <= 1e-6 * max(events, 1), name
        g, scale = cf.dlogits, cf.A.sum()
        key = ((np.arange(g.size, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1021)).astype(np.float64).reshape(g.shape)
        got = [float(x) for x in row[13:16]]
        # the harness rounds dlogits to fp32 as the kernel does: 2^-24 of each element, far inside 1e-6 of the sum of A
        assert abs(got[0] - g.sum()) <= 1e-6 * scale + 1e-300, (name, got[0], g.sum())
        assert abs(got[1] - np.abs(g).sum()) <= 1e-6 * scale + 1e-300, name
        assert abs(got[2] - float((g * key).sum())) <= 1e-6 * scale * 1021 + 1e-300, name
