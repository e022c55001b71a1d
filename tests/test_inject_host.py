"""The coordinate-injection INR's C ABI without a GPU: header, symbols and struct sizes, every refusal (made before any HIP
call), the scratch formula, and the kernels' index arithmetic on the CPU under AddressSanitizer + UBSan
(tests/native/inject_harness.hip, built and run as a program the way test_hausdorff_host.py builds the distance-transform
harness)."""
import ctypes as C
import inspect
import os
import pathlib
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import inject_cases as ic
import inject_ref as ref
from mrirt import _lib, inr

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
SYMBOLS = ["mrirt_inject_scratch_bytes", "mrirt_inject_forward", "mrirt_inject_uncertainty", "mrirt_inject_predict_volume",
           "mrirt_boundary_weights_scratch_bytes", "mrirt_boundary_weights"]
NULL, ARG = -1, -5


def test_header_symbols_and_struct_sizes():
    l = _lib.lib()
    header = (ROOT / "include" / "mrirt.h").read_text()
    for s in SYMBOLS:
        assert s in _lib.ABI_SYMBOLS and hasattr(l, s) and re.search(rf"\b{s}\(", header), s
    assert "typedef struct MrirtInjectDesc" in header and "typedef struct MrirtInjectDropout" in header
    assert l.mrirt_sizeof(17) == C.sizeof(_lib.InjectDesc) == 52
    assert l.mrirt_sizeof(18) == C.sizeof(_lib.InjectDropout) == 32
    assert l.mrirt_sizeof(12) == 0 and l.mrirt_sizeof(16) == 0 and l.mrirt_sizeof(19) == 0 and l.mrirt_abi_version() == 4
    assert "inr_inject.hip" in _lib.HIP_SOURCES


def test_python_names_have_the_notebook_signatures():
    sig = inspect.signature(inr.predict_full_volume)
    assert list(sig.parameters)[:3] == ["params", "case_data", "chunk_size"] and sig.parameters["chunk_size"].default == 50000
    sig = inspect.signature(inr.compute_uncertainty_mc_dropout)
    assert list(sig.parameters)[:6] == ["params", "coords", "mods", "n_samples", "seed", "dropout_rate"]
    assert sig.parameters["n_samples"].default == 5 and sig.parameters["dropout_rate"].default == 0.3
    assert inspect.signature(inr.boundary_weights).parameters["num_classes"].default == 4
    sig = inspect.signature(inr.inject_desc)
    assert sig.parameters["coord_layers"].default == (1, 2, 3) and sig.parameters["mod_layers"].default == (2,)


def test_inject_load_round_trip_and_desc(tmp_path):
    g = ic.load_golden()
    path = tmp_path / "model_final.npz"
    np.savez_compressed(path, **{k: v for k, v in g.items() if k == "fourier_B" or k.startswith("mlp_")})
    p = inr.inject_load(path)
    assert ref.same_bits(p["fourier"]["B"], g["fourier_B"]) and len(p["mlp"]) == 4
    for i, layer in enumerate(p["mlp"]):
        assert ref.same_bits(layer["W"], g[f"mlp_W_{i}"]) and ref.same_bits(layer["b"], g[f"mlp_b_{i}"])
    d = inr.inject_desc(p)                                        # the notebook's own lists: index 3 names the head and is dropped
    assert (d.numLayers, d.fourierDim, d.numMods, list(d.width)[:4], d.coordLayers, d.modLayers) == (4, 128, 4, [64, 64, 64, 4], 0b110, 0b100)
    with pytest.raises(ValueError):
        inr.inject_desc(p, coord_layers=(1,), mod_layers=(2,))   # the weights do not have that shape


def _desc(L=4, F=128, M=4, widths=(64, 64, 64, 4), cl=0b110, ml=0b100):
    d = _lib.InjectDesc()
    d.numLayers, d.fourierDim, d.numMods, d.coordLayers, d.modLayers = L, F, M, cl, ml
    for i, w in enumerate(widths):
        d.width[i] = w
    return d


def _drop(seed=1, keep=0.5, samples=1, sample0=0, reserved=0, index0=0):
    d = _lib.InjectDropout()
    d.seed, d.keep, d.samples, d.sample0, d.reserved, d.index0 = seed, keep, samples, sample0, reserved, index0
    return d


BAD_DESCS = {
    "one layer": dict(L=1), "nine layers": dict(L=9), "F odd": dict(F=127), "F zero": dict(F=0), "F 258": dict(F=258),
    "nine mods": dict(M=9), "width zero": dict(widths=(64, 0, 64, 4)), "width 257": dict(widths=(257, 64, 64, 4)),
    "17 classes": dict(widths=(64, 64, 64, 17)), "coords at 0": dict(cl=0b111), "coords at the head": dict(cl=0b1110),
    "mods at the head": dict(ml=0b1100), "mods at 0": dict(ml=0b101), "bit beyond": dict(cl=1 << 9),
}


def test_abi_rejects_malformed_arguments_before_any_hip_call():
    """Host memory stands in for the device buffers: every call below must return before anything is launched or read."""
    l = _lib.lib()
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    big = 1 << 40
    ok, hwd = _desc(), (C.c_uint32 * 3)(4, 4, 4)

    def fwd(desc=ok, B=p, w=p, b=p, coords=p, mods=p, n=8, drop=None, logits=p, am=p, scratch=p, nbytes=big):
        return l.mrirt_inject_forward(C.byref(desc) if desc is not None else None, B, w, b, coords, mods, n,
                                      C.byref(drop) if drop is not None else None, logits, am, scratch, nbytes, None)

    def unc(desc=ok, B=p, w=p, b=p, coords=p, mods=p, n=8, drop=_drop(samples=5), ent=p, mean=p, scratch=p, nbytes=big):
        return l.mrirt_inject_uncertainty(C.byref(desc) if desc is not None else None, B, w, b, coords, mods, n,
                                          C.byref(drop) if drop is not None else None, ent, mean, scratch, nbytes, None)

    def vol(desc=ok, B=p, w=p, b=p, mods=p, hwd=hwd, chunk=16, drop=None, pred=p, ent=None, scratch=p, nbytes=big):
        return l.mrirt_inject_predict_volume(C.byref(desc) if desc is not None else None, B, w, b, mods, hwd, chunk,
                                             C.byref(drop) if drop is not None else None, pred, ent, scratch, nbytes, None)

    def bw(lab=p, hwd=hwd, nc=4, out=p, scratch=p, nbytes=big):
        return l.mrirt_boundary_weights(lab, hwd, nc, out, scratch, nbytes, None)

    for kw in ("desc", "B", "w", "b", "coords", "mods", "scratch"):
        assert fwd(**{kw: None}) == NULL and unc(**{kw: None}) == NULL, kw
    assert fwd(logits=None, am=None) == NULL and unc(drop=None) == NULL and unc(ent=None) == NULL
    for kw in ("desc", "B", "w", "b", "mods", "hwd", "pred", "scratch"):
        assert vol(**{kw: None}) == NULL, kw
    assert vol(ent=p) == NULL                                    # entropy without a dropout
    assert vol(drop=_drop(samples=5)) == ARG                     # a dropout without entropy
    for kw in ("lab", "hwd", "out", "scratch"):
        assert bw(**{kw: None}) == NULL, kw
    for name, kw in BAD_DESCS.items():
        d = _desc(**kw)
        assert fwd(desc=d) == ARG and unc(desc=d) == ARG and vol(desc=d) == ARG, name
        assert l.mrirt_inject_scratch_bytes(C.byref(d), 8) == 0, name
    for n in (0, -1, 1 << 31):
        assert fwd(n=n) == ARG and unc(n=n) == ARG and l.mrirt_inject_scratch_bytes(C.byref(ok), n) == 0
        assert vol(chunk=n) == ARG
    for bad in (_drop(keep=0.0), _drop(keep=-0.5), _drop(keep=1.5), _drop(keep=float("nan")), _drop(keep=1e-45), _drop(samples=0),
                _drop(samples=2), _drop(sample0=1 << 24), _drop(reserved=1)):
        assert fwd(drop=bad) == ARG, (bad.keep, bad.samples, bad.sample0)
    for bad in (_drop(keep=0.0, samples=5), _drop(samples=0), _drop(samples=65), _drop(samples=5, sample0=(1 << 24) - 4), _drop(keep=2.0, samples=5)):
        assert unc(drop=bad) == ARG and vol(drop=bad, ent=p) == ARG, (bad.keep, bad.samples, bad.sample0)
    assert vol(drop=_drop(samples=5, index0=1), ent=p) == ARG
    for bad in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (2048, 1024, 1024)):
        assert vol(hwd=(C.c_uint32 * 3)(*bad)) == ARG, bad
    need = l.mrirt_inject_scratch_bytes(C.byref(ok), 8)
    assert need > 0
    for call in (fwd, unc):
        assert call(nbytes=need - 1) == ARG and call(nbytes=0) == ARG and call(nbytes=-1) == ARG
        assert call(scratch=C.c_void_p(p.value + 4)) == ARG      # misaligned
    need = l.mrirt_inject_scratch_bytes(C.byref(ok), 16)
    assert vol(nbytes=need - 1) == ARG and vol(scratch=C.c_void_p(p.value + 8)) == ARG
    assert l.mrirt_inject_scratch_bytes(None, 8) == 0
    # a net without modalities needs no mods pointer: the call gets as far as the scratch check
    assert fwd(desc=_desc(M=0, ml=0), mods=None, nbytes=0) == ARG
    for nc in (0, 33):
        assert bw(nc=nc) == ARG
    for bad in ((0, 4, 4), (4097, 1, 1), (2048, 1024, 1024)):
        assert bw(hwd=(C.c_uint32 * 3)(*bad)) == ARG and l.mrirt_boundary_weights_scratch_bytes((C.c_uint32 * 3)(*bad)) == 0
    need = l.mrirt_boundary_weights_scratch_bytes(hwd)
    assert need >= 8 * 64 and bw(nbytes=need - 1) == ARG and bw(scratch=C.c_void_p(p.value + 4)) == ARG
    assert l.mrirt_boundary_weights_scratch_bytes(None) == 0


def test_scratch_bytes_is_monotone_in_n():
    l = _lib.lib()
    ns = [1, 2, 63, 64, 65, 100, 257, 4096, 50000, 50001, 1 << 20, 8928000, (1 << 31) - 1]
    for d in (_desc(), _desc(L=2, F=2, M=0, widths=(1, 1), cl=0, ml=0), _desc(L=3, F=256, M=8, widths=(256, 256, 16), cl=2, ml=2)):
        sizes = [l.mrirt_inject_scratch_bytes(C.byref(d), n) for n in ns]
        assert all(v > 0 and v % 256 == 0 for v in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        C_out = d.width[d.numLayers - 1]
        hid = max(d.width[i] for i in range(d.numLayers - 1))
        for n, v in zip(ns, sizes):                               # coords, features, two activations, logits, probability sums
            assert v >= 4 * n * (3 + d.fourierDim + 2 * hid + 2 * C_out)


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "inject_harness"
    src = ROOT / "tests" / "native" / "inject_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "inject_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "inject_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


def _blob(params, F, M, widths, cl, ml, n, hwd, chunk, coords, mods, drop=None):
    cbits, mbits = ref.bits(cl, ml, len(widths))
    w, b = ref.flat(params)
    hd = [len(widths), F, M, *widths, *([0] * (8 - len(widths))), cbits, mbits, n, *hwd, chunk, 1 if drop else 0, drop["s"] if drop else 0]
    out = struct.pack("<20I", *hd) + struct.pack("<Qf", drop["seed"] if drop else 0, drop["keep"] if drop else 1.0)
    out += np.asarray(params["fourier"]["B"], np.float32).tobytes() + w.tobytes() + b.tobytes()
    if coords is not None:
        out += np.ascontiguousarray(coords, np.float32).tobytes()
    return out + np.ascontiguousarray(mods, np.float32).tobytes()


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_index_arithmetic_under_asan_and_ubsan(tmp_path):
    exe = build_harness()
    l = _lib.lib()
    cases, blob = [], b""
    for case in ic.EXACT:
        name, n, F, M, widths, cl, ml, _ = case
        params, _, coords, mods = ic.exact_case(case)
        for drop in (None, dict(seed=77, keep=0.5, s=3)):
            if drop and n > 65:
                continue
            blob += _blob(params, F, M, widths, cl, ml, n, (0, 0, 0), 0, coords, mods, drop)
            cases.append((name, params, F, M, widths, cl, ml, n, None, coords, mods, drop, n))
    for hwd, chunk in (((2, 2, 2), 3), ((7, 33, 5), 100), ((7, 33, 5), 64), ((3, 4, 5), 60)):
        n = hwd[0] * hwd[1] * hwd[2]
        rng = np.random.default_rng(n)
        params, _ = ref.selection_net(rng, 16, 4, (17, 64, 13, 4), (1, 2), (2,), 5)
        mods = rng.normal(0, 1, (4, *hwd)).astype(np.float32)
        blob += _blob(params, 16, 4, (17, 64, 13, 4), (1, 2), (2,), n, hwd, chunk, None, mods)
        cases.append((f"volume{hwd}x{chunk}", params, 16, 4, (17, 64, 13, 4), (1, 2), (2,), n, hwd, ref.grid_coords(hwd), ref.volume_mods(mods), None, chunk))
    path, outp = tmp_path / "cases.bin", tmp_path / "out.bin"
    path.write_bytes(struct.pack("<I", len(cases)) + blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(path), str(outp)], capture_output=True, text=True, env=env, timeout=900)
    out = r.stdout + r.stderr
    print(out[-6000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "FAILED" not in out, out[-6000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert len(lines) == len(cases) and f"inject_harness: {len(cases)} cases done" in r.stdout
    raw, at = outp.read_bytes(), 0
    for ln, (name, params, F, M, widths, cl, ml, n, hwd, coords, mods, drop, per) in zip(lines, cases):
        cbits, mbits = ref.bits(cl, ml, len(widths))
        d = _desc(len(widths), F, M, widths, cbits, mbits)
        # the buffer the harness ran in (ASan-checked, exactly this long) is what the ABI tells callers to allocate
        assert int(ln[3]) == l.mrirt_inject_scratch_bytes(C.byref(d), per), name
        Cn = widths[-1]
        got = np.frombuffer(raw, np.float32, n * Cn, at).reshape(n, Cn); at += 4 * n * Cn
        am = np.frombuffer(raw, np.int16, n, at); at += 2 * n
        want = ref.forward32(params, coords, mods, cl, ml, drop)
        assert ref.same_bits(got, want), name
        assert np.array_equal(am, ref.argmax(want)), name
    assert at == len(raw)
