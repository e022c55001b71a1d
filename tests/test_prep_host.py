"""Case preparation without a GPU: the NumPy restatements of tests/prep_ref.py pinned to their sources
(np.percentile, volume.normalize_intensity, scipy.ndimage.gaussian_filter and its stored outputs, an fp64 z-score), the index
arithmetic of csrc/prep_index.h on the CPU under AddressSanitizer + UBSan (tests/native/prep_harness.hip, a stand-alone
program), the argument checks of the C ABI (made before any HIP call) and the scratch formula."""
import ctypes as C
import inspect
import os
import pathlib
import shutil
import struct
import subprocess

import numpy as np
import pytest

import prep_ref as pr
import mrirt
from mrirt import _lib, volume

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
GOLDEN = ROOT / "tests" / "golden" / "prep_gauss.npz"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
f32 = np.float32
GAUSS_SHAPES = [(1, 1, 1), (2, 3, 1), (5, 1, 7), (9, 8, 7), (33, 17, 20)]
NAMED_SIZES = [131802, 8928000, 8928001]


def _mri_like(rng, shape):
    return (rng.integers(0, 4096, size=shape) * (rng.random(shape) < 0.6)).astype(np.float32)


# --- the percentile -------------------------------------------------------------------------------------------------------
def test_percentile_restatement_equals_numpy_on_random_sizes():
    rng = np.random.default_rng(1)
    sizes = [1, 2, 3, 4, 5] + rng.integers(1, 5001, size=400).tolist()
    for n in sizes:
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)
        if n % 3 == 0:
            v = np.round(v)                       # ties
        for q in (1.0, 99.5, 0.0, 100.0, 50.0):
            want = np.percentile(v, q)
            assert want.dtype == np.float32
            got = pr.percentile(v, q)
            assert got.tobytes() == want.tobytes() or (got == want == 0), (n, q, got, want)


@pytest.mark.parametrize("n", NAMED_SIZES)
def test_percentile_restatement_equals_numpy_at_the_named_sizes(n):
    rng = np.random.default_rng(n)
    v = _mri_like(rng, n) + rng.random(n).astype(np.float32)
    for q in (1.0, 99.5):
        assert pr.percentile(v, q).tobytes() == np.percentile(v, q).tobytes(), (n, q)


def test_fp32_index_differs_from_the_exact_one_at_131802():
    k, g = pr.rank(131802, 99.5)
    assert k == 131142 and int(np.floor(131801 * 0.995)) == 131141
    k, g = pr.rank(8928000, 99.5)
    assert g == 0                                  # no fraction bits left at 8.88 M


def test_percentile_with_nan_is_nan_as_in_numpy():
    v = np.arange(100, dtype=np.float32)
    v[17] = np.nan
    with np.errstate(all="ignore"):
        assert np.isnan(np.percentile(v, 1.0)) and np.isnan(np.percentile(v, 99.5))
    assert np.isnan(pr.percentile(v, 1.0)) and np.isnan(pr.percentile(v, 99.5))


def _window_cases():
    rng = np.random.default_rng(7)
    yield "random_2x3x5", rng.standard_normal((2, 3, 5)).astype(np.float32)
    yield "one", np.array([[[3.5]]], dtype=np.float32)
    yield "two", np.array([[[3.5, -1.0]]], dtype=np.float32)
    yield "constant", np.full((4, 5, 6), 7.25, dtype=np.float32)
    yield "two_valued", np.where(rng.random((7, 6, 5)) < 0.3, 2.0, -1.0).astype(np.float32)
    yield "mri_like", _mri_like(rng, (17, 19, 23))
    yield "denormals", (rng.integers(-50, 50, size=(6, 7, 8)).astype(np.float32) * f32(1e-42)).astype(np.float32)
    yield "signed_zeros", np.where(rng.random((5, 6, 7)) < 0.5, 0.0, -0.0).astype(np.float32)
    v = rng.standard_normal((5, 6, 7)).astype(np.float32)
    v[2, 3, 4] = np.nan
    yield "one_nan", v
    v = rng.standard_normal((5, 6, 7)).astype(np.float32)
    v[0, 0, 0], v[1, 1, 1] = np.inf, -np.inf
    yield "infs", v


@pytest.mark.parametrize("name,vol", list(_window_cases()), ids=[c[0] for c in _window_cases()])
def test_window_and_normalisation_equal_the_host_function(name, vol):
    with np.errstate(all="ignore"):
        lin, norm, dims = volume.normalize_intensity(vol)
    rec = pr.window(vol)
    got = pr.normalize(vol, rec)
    assert pr.same(got, norm), name
    assert pr.same(pr.flatten_xyz(got), lin) and dims.tolist() == list(vol.shape)
    if name == "constant":
        assert rec[2] == f32(1e-6) and rec[0] == rec[1] == f32(7.25)


# --- the z-score ----------------------------------------------------------------------------------------------------------
def test_zscore_restatement_against_fp64_and_the_host():
    rng = np.random.default_rng(3)
    vol = _mri_like(rng, (20, 21, 22))
    mu, sg, cnt = pr.zscore_stats(vol)
    x = vol[vol != 0].astype(np.float64)
    assert cnt == x.size and mu == f32(x.mean()) and abs(float(sg) - x.std()) <= np.spacing(sg)
    z = pr.zscore_apply(vol, mu, sg, cnt)
    z64 = pr.zscore_f64(vol)
    host = volume.zscore_nonzero(vol)
    dev_host = np.abs(host - z64).max()
    dev_ref = np.abs(z - z64).max()
    print(f"host fp32 deviation from fp64 {dev_host:.3e}, restatement's {dev_ref:.3e}")
    assert dev_ref <= 8 * max(dev_host, np.finfo(np.float32).eps)
    zeros = np.zeros((3, 4, 5), np.float32)
    assert pr.zscore_stats(zeros) == (0, 0, 0) and pr.same(pr.zscore_apply(zeros, 0, 0, 0), zeros)
    one = zeros.copy()
    one[1, 2, 3] = 5
    mu, sg, cnt = pr.zscore_stats(one)
    assert (mu, sg, cnt) == (5, 0, 1) and pr.same(pr.zscore_apply(one, mu, sg, cnt), volume.zscore_nonzero(one))


# --- the Gaussian ---------------------------------------------------------------------------------------------------------
def _tag(shape):
    return "x".join(str(v) for v in shape)


def test_gaussian_restatement_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for shape in GAUSS_SHAPES + [(3, 3, 3)]:
        a = (rng.standard_normal(shape) * 100).astype(np.float32)
        for sigma in (0.5, 1.0, 2.3):
            assert np.array_equal(pr.gaussian_filter(a, sigma), ndimage.gaussian_filter(a, sigma)), (shape, sigma)
    a = rng.standard_normal((4, 5, 6)).astype(np.float32)
    assert np.array_equal(pr.gaussian_filter(a, 0.1), a) and len(pr.gaussian_weights(0.1)) == 1      # radius 0: the identity


@pytest.mark.parametrize("sigma", [0.5, 2.3])
@pytest.mark.parametrize("shape", GAUSS_SHAPES, ids=_tag)
def test_gaussian_restatement_equals_the_stored_scipy_outputs(shape, sigma):
    g = np.load(GOLDEN)
    a, w, want = g[f"in_{_tag(shape)}"], g[f"w_{sigma}"], g[f"out_{_tag(shape)}_{sigma}"]
    assert a.dtype == np.float32 and want.dtype == np.float32 and w.dtype == np.float64 and a.shape == shape
    assert np.array_equal(pr.gaussian_weights(sigma), w) and np.array_equal(volume.gaussian_weights(sigma), w)
    assert np.array_equal(pr.gaussian_filter(a, weights=w), want)


def test_golden_file_is_small():
    assert GOLDEN.stat().st_size < 256 * 1024


# --- the Python names -----------------------------------------------------------------------------------------------------
def test_python_names_and_abi_symbols():
    sig = inspect.signature(volume.normalize_intensity_device)
    assert list(sig.parameters)[:2] == ["data", "percentiles"] and sig.parameters["percentiles"].default == (1.0, 99.5)
    assert list(inspect.signature(volume.zscore_nonzero_device).parameters)[0] == "mods"
    assert list(inspect.signature(volume.gaussian_filter_device).parameters)[:2] == ["vol", "sigma"]
    for s in ("mrirt_prep_scratch_bytes", "mrirt_prep_window", "mrirt_prep_normalize", "mrirt_prep_zscore_scratch_bytes",
              "mrirt_prep_zscore_stats", "mrirt_prep_zscore_apply", "mrirt_prep_gaussian3d"):
        assert s in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), s)
    assert "prep.hip" in _lib.HIP_SOURCES and _lib.lib().mrirt_abi_version() == 4
    with pytest.raises(ValueError):
        volume.gaussian_weights(4.2)               # radius 17
    with pytest.raises(ValueError):
        volume.gaussian_weights(0.0)
    assert len(volume.gaussian_weights(4.1)) == 33


# --- the C ABI without a device -------------------------------------------------------------------------------------------
def _d3(*v):
    return (C.c_uint32 * 3)(*v)


def test_abi_rejects_malformed_arguments_before_any_hip_call():
    """Host memory stands in for the device buffers: every call below must return before anything is launched or read."""
    l = _lib.lib()
    buf = C.create_string_buffer(8192)
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)
    q = C.c_void_p(p.value + 4096)
    NULL, DIMS, ARG = -1, -2, -5
    big = 1 << 40

    def window(vol=p, n=100, qlo=1.0, qhi=99.5, rec=p, scratch=p, nbytes=big):
        return l.mrirt_prep_window(vol, n, qlo, qhi, rec, scratch, nbytes, None)

    for kw in ("vol", "rec", "scratch"):
        assert window(**{kw: None}) == NULL, kw
    for n in (0, -1, 1 << 31, 1 << 40):
        assert window(n=n) == ARG and l.mrirt_prep_scratch_bytes(n) == 0, n
    assert l.mrirt_prep_scratch_bytes((1 << 31) - 1) > 0
    need = l.mrirt_prep_scratch_bytes(100)
    assert window(nbytes=need - 1) == ARG and window(nbytes=0) == ARG and window(nbytes=-1) == ARG
    assert window(scratch=C.c_void_p(p.value + 4)) == ARG
    for bad in (-0.5, 100.5, float("nan"), float("inf")):
        assert window(qlo=bad) == ARG and window(qhi=bad) == ARG, bad

    def normalize(vol=p, dims=_d3(4, 4, 4), rec=p, norm=q, lin=q):
        return l.mrirt_prep_normalize(vol, dims, rec, norm, lin, None)

    for kw in ("vol", "dims", "rec"):
        assert normalize(**{kw: None}) == NULL, kw
    assert normalize(norm=None, lin=None) == NULL
    for bad in (_d3(0, 4, 4), _d3(4, 0, 4), _d3(4, 4, 0)):
        assert normalize(dims=bad) == DIMS
    assert normalize(dims=_d3(2048, 1024, 1024)) == ARG and normalize(dims=_d3(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)) == ARG
    assert normalize(lin=p) == ARG

    def stats(mods=p, n=100, M=4, st=p, scratch=p, nbytes=big):
        return l.mrirt_prep_zscore_stats(mods, n, M, st, scratch, nbytes, None)

    def apply(mods=p, n=100, M=4, st=p, out=p):
        return l.mrirt_prep_zscore_apply(mods, n, M, st, out, None)

    for kw in ("mods", "st", "scratch"):
        assert stats(**{kw: None}) == NULL, kw
    for kw in ("mods", "st", "out"):
        assert apply(**{kw: None}) == NULL, kw
    for fn in (stats, apply):
        assert fn(M=0) == ARG and fn(M=65) == ARG
        for n in (0, -1, 1 << 31):
            assert fn(n=n) == ARG, n
    zneed = l.mrirt_prep_zscore_scratch_bytes(100, 4)
    assert zneed > 0 and stats(nbytes=zneed - 1) == ARG and stats(scratch=C.c_void_p(p.value + 4)) == ARG
    assert l.mrirt_prep_zscore_scratch_bytes(100, 0) == 0 and l.mrirt_prep_zscore_scratch_bytes(0, 4) == 0

    w = (C.c_double * 33)(*([1.0 / 33] * 33))
    far = C.c_void_p(p.value + 2048)

    def gauss(vol=p, dims=_d3(4, 4, 4), wt=w, r=2, out=q, scratch=far):
        return l.mrirt_prep_gaussian3d(vol, dims, wt, r, out, scratch, None)

    for kw in ("vol", "dims", "wt", "out", "scratch"):
        assert gauss(**{kw: None}) == NULL, kw
    for bad in (_d3(0, 4, 4), _d3(4, 0, 4), _d3(4, 4, 0)):
        assert gauss(dims=bad) == DIMS
    assert gauss(r=17) == ARG and gauss(r=-1) == ARG and gauss(dims=_d3(2048, 1024, 1024)) == ARG
    assert gauss(scratch=p) == ARG and gauss(scratch=q) == ARG and gauss(out=C.c_void_p(p.value + 16)) == ARG     # overlaps


def test_scratch_bytes_formula():
    l = _lib.lib()
    sizes = [1, 2, 4095, 4096, 4097, 131802, 512 * 4096 - 1, 512 * 4096, 512 * 4096 + 1, 8928000, 2**31 - 1]
    got = [l.mrirt_prep_scratch_bytes(n) for n in sizes]
    assert got == [pr.window_scratch_bytes(n) for n in sizes]
    assert all(a <= b for a, b in zip(got, got[1:])) and got[-1] == got[-2] == 256 + 4096 + 4096 + 512 * 4096


# --- the index arithmetic under the sanitizers ----------------------------------------------------------------------------
def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "prep_harness"
    src = ROOT / "tests" / "native" / "prep_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "prep_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "prep_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


def _bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_index_arithmetic_under_asan_and_ubsan_equals_the_restatement(tmp_path):
    exe = build_harness()
    rng = np.random.default_rng(11)
    cmds, want = [], []
    # keys: every sign x exponent class with the mantissas at both ends and in the middle
    for sign in (0, 1):
        for e in range(256):
            for man in (0, 1, 0x400000, 0x7FFFFF):
                b = (sign << 31) | (e << 23) | man
                k = pr.key(b)
                cmds.append(f"K {b:08x}")
                want.append(f"K {k:08x} {pr.key_inverse(k):08x}")
    for n in [1, 2, 3, 100, 131802, 8928000, 8928001, 17000001, 2**31 - 1] + rng.integers(1, 5001, size=50).tolist():
        for q in (0.0, 1.0, 50.0, 99.5, 100.0):
            k, g = pr.rank(n, q)
            cmds.append(f"P {n} {_bits(q):08x}")
            want.append(f"P {k} {_bits(g):08x}")
    hists = [np.zeros(256, np.int64) for _ in range(4)]
    hists[0][0] = 10                                    # everything in the first bin
    hists[1][255] = 10                                  # ... in the last
    hists[2][[3, 4, 200]] = [1, 2, 3]                   # gaps
    hists[3][:] = rng.integers(0, 5, size=256)          # dense, with empty bins
    for h in hists:
        total = int(h.sum())
        for r in sorted({0, 1, total // 2, total - 2, total - 1} & set(range(total))):
            cmds.append(f"S {r} " + " ".join(str(int(c)) for c in h))
            b, rem = pr.select_bin(h.tolist(), r)
            want.append(f"S {b} {rem}")
            assert h[:b].sum() + rem == r and rem < h[b]
    for p, ans in (((0, 0, 0, 0), "1 0 0 0 0"), ((5, 5, 9, 9), "2 0 0 1 1"), ((1, 2, 3, 4), "4 0 1 2 3"), ((7, 8, 7, 8), "2 0 1 0 1"),
                   ((1, 2, 2, 3), "3 0 1 1 2")):
        cmds.append("A " + " ".join(map(str, p)))
        want.append("A " + ans)
    for n in range(1, 6):
        for i in range(-17, n + 17):                    # r up to 16, and one more
            cmds.append(f"R {i} {n}")
            want.append(f"R {pr.reflect(i, n)}")
    for n in (1, 4096, 4097, 8928000, 2**31 - 1, 0, 2**31):
        cmds.append(f"W {n}")
        blocks = min(max(-(-n // 4096), 1), 512) if pr.window_scratch_bytes(n) else 0
        want.append(f"W {blocks} {pr.window_scratch_bytes(n)}")
    for shape in [(1, 1, 1), (2, 3, 1), (5, 1, 7), (9, 8, 7), (33, 17, 20), (40, 33, 65), (3, 70, 2)]:
        for axis in range(3):
            for cfg in ((1, 32, 32), (4, 64, 1)):
                for r in (0, 2, 16):
                    cmds.append(f"T {shape[0]} {shape[1]} {shape[2]} {axis} {cfg[0]} {cfg[1]} {cfg[2]} {r}")
                    outer = int(np.prod(shape[:axis], dtype=np.int64))
                    inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
                    tiles = -(-outer // cfg[0]) * -(-shape[axis] // cfg[1]) * -(-inner // cfg[2])
                    want.append(f"T {tiles} ok")
    path = tmp_path / "commands.txt"
    path.write_text("\n".join(cmds) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "FAILED" not in out, out[-6000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"prep_harness: {len(cmds)} commands done" and len(lines) == len(cmds) + 1
    for c, got, exp in zip(cmds, lines, want):
        assert got == exp, (c[:60], got, exp)
