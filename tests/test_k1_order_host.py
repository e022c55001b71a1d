"""The dispatch order of the K1 march without a GPU: the builder's permutation logic (csrc/k1_order.h, through
``mrirt_order_build_host``) against a NumPy restatement for random step records, the sizes of its tables, which launches
take an order (``mrirt_brats_order_applicable``), and the same header under AddressSanitizer + UBSan
(tests/native/order_harness.cpp, a stand-alone program)."""
import ctypes as C
import os
import pathlib
import subprocess

import numpy as np
import pytest

from mrirt import _lib, params, synth

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
XCDS = 8
SIZES = [0, 1, 5, 8, 9, 13, 64, 100, 511, 512, 4096, 4100]      # workgroup counts: 0, below 8, no multiple of 8, the bench's 4096


def build_host(steps: np.ndarray, classes: int) -> np.ndarray:
    steps = np.ascontiguousarray(steps, dtype=np.uint32)
    order = np.full(steps.size, 0xDEADBEEF, dtype=np.uint32)
    rc = _lib.lib().mrirt_order_build_host(steps.ctypes.data if steps.size else None, steps.size, classes,
                                           order.ctypes.data if steps.size else None)
    assert rc == 0
    return order


def reference(steps: np.ndarray, classes: int) -> np.ndarray:
    """Per XCD (positions b % 8): thresholds at the values of rank j * n // C, class = thresholds reached, classes longest
    first, a stable sort inside — written with NumPy's own sort, nothing of the header's bitwise selection."""
    C_ = 4 if classes == 0 else min(classes, 16)
    order = np.zeros(steps.size, dtype=np.uint32)
    for x in range(XCDS):
        pos = np.arange(x, steps.size, XCDS, dtype=np.uint32)
        v = steps[pos].astype(np.int64)
        n = v.size
        if n == 0:
            continue
        srt = np.sort(v)
        thr = [srt[(j * n) // C_] for j in range(1, C_)]
        cls = np.zeros(n, dtype=np.int64)
        for t in thr:
            cls += v >= t
        order[pos] = pos[np.argsort(-cls, kind="stable")]
    return order


def records(words: int, seed: int):
    rng = np.random.default_rng(seed)
    yield "steps", rng.integers(0, 700, words, dtype=np.uint32)
    yield "ties", rng.integers(0, 3, words, dtype=np.uint32)
    yield "sparse", np.where(rng.random(words) < 0.25, rng.integers(1, 1000, words), 0).astype(np.uint32)
    yield "wide", rng.integers(0, 2 ** 32, words, dtype=np.uint64).astype(np.uint32)
    yield "ramp", np.arange(words, dtype=np.uint32)[::-1].copy()


@pytest.mark.parametrize("classes", [0, 1, 2, 4, 8, 16, 40])
@pytest.mark.parametrize("words", SIZES)
def test_builder_equals_the_numpy_reference(words, classes):
    for name, steps in records(words, 1000 * words + classes):
        got, want = build_host(steps, classes), reference(steps, classes)
        assert np.array_equal(got, want), (name, words, classes)


@pytest.mark.parametrize("words", SIZES)
def test_tables_are_stable_descending_permutations_inside_each_xcd(words):
    for classes in (2, 4, 16):
        for name, steps in records(words, 77 + words):
            order = build_host(steps, classes)
            assert np.array_equal(np.sort(order), np.arange(words, dtype=np.uint32)), name            # a permutation ...
            assert np.array_equal(order % XCDS, np.arange(words, dtype=np.uint32) % XCDS), name        # ... inside each XCD
            for x in range(XCDS):
                e = order[x::XCDS].astype(np.int64)
                v = steps[e].astype(np.int64)
                n = v.size
                if n == 0:
                    continue
                srt = np.sort(steps[x::XCDS].astype(np.int64))
                cls = sum((v >= srt[(j * n) // classes]).astype(np.int64) for j in range(1, classes))
                assert np.all(np.diff(cls) <= 0), (name, x)                                             # classes descending
                same = np.diff(cls) == 0
                assert np.all(np.diff(e)[same] > 0), (name, x)                                          # launch order inside a class


@pytest.mark.parametrize("words", SIZES)
def test_a_zero_record_gives_the_identity(words):
    for classes in (0, 1, 4, 16):
        assert np.array_equal(build_host(np.zeros(words, dtype=np.uint32), classes), np.arange(words, dtype=np.uint32))
    # ... and so does one class, whatever the record
    steps = np.random.default_rng(5).integers(0, 500, words, dtype=np.uint32)
    assert np.array_equal(build_host(steps, 1), np.arange(words, dtype=np.uint32))


def test_null_tables_are_refused_and_an_empty_launch_is_not():
    l = _lib.lib()
    assert l.mrirt_order_build_host(None, 0, 4, None) == 0
    assert l.mrirt_order_build_host(None, 8, 4, None) == -1


def _words(w, h, ext):
    size = (C.c_uint32 * 2)(w, h)
    return int(_lib.lib().mrirt_order_words(size, C.byref(params.render_ext(ext)) if ext is not None else None))


def test_table_sizes_follow_the_launch():
    # the bench's frame: VGA grids at 1024^2 march in 16-px workgroups, 4096 of them; other layouts in 8-px ones
    assert _words(1024, 1024, {"layout": "vga"}) == 4096
    assert _words(1024, 1024, {"layout": "vga", "kernelVariant": 2}) == 16384
    assert _words(1024, 1024, {"layout": "vg"}) == 16384
    # ragged frames: whole bands per XCD, so the launch (and the tables) are padded to 8 bands' worth
    assert _words(136, 120, {"layout": "quad"}) == 17 * 16          # 15 band rows of 17 workgroups -> 2 bands per XCD
    assert _words(136, 120, {"layout": "vga", "kernelVariant": 2}) == 9 * 8
    assert _words(128, 128, None) == 256
    # no ordering: tiled launches, an empty image
    assert _words(1024, 1024, {"layout": "vga", "tileSize": 64, "tileRank": 0, "tileWorld": 2}) == 0
    assert _words(0, 16, None) == 0


def _applicable(p, ext, skip=False):
    P, E = params.brats_params(p), params.render_ext(ext)
    fake = C.c_void_p(0x1000)
    vp = (C.c_void_p * 4)(*[fake if P.volEnabled[m] != 0 else None for m in range(4)])
    S = None
    if skip:
        S = _lib.Skip()
        for m in range(4):
            S.macroUb[m] = 0x1000 if P.volEnabled[m] != 0 else None
        S.macroSeg = S.macroPred = S.mask = 0x1000
        S.maskWords = 0xFFFFFFFF
    return int(_lib.lib().mrirt_brats_order_applicable(C.byref(P), C.byref(E), vp, fake, fake, C.byref(S) if S is not None else None))


def test_which_launches_take_an_order():
    dims = (64, 64, 64)
    p1 = synth.brats_scene(0, 0, 96, dims=dims, image_hw=(120, 136), channels=1, intensity_alpha=16.0)
    p4 = synth.brats_scene(0, 0, 96, dims=dims, image_hw=(120, 136), channels=4)
    shade = dict(synth.SHADE_EXT)
    assert _applicable(p1, dict(shade, layout="vga")) == 1                         # the benched kernel (pipelined)
    assert _applicable(p1, dict(shade, layout="vga", kernelVariant=1 << 15)) == 1  # its tagged twin
    assert _applicable(p4, dict(shade, layout="vga")) == 1                         # rolling
    assert _applicable(p4, dict(layout="quad")) == 1                               # pipelined, unshaded
    assert _applicable(p1, dict(shade, layout="vga"), skip=True) == 0              # marches with an empty-radius map
    assert _applicable(p1, dict(shade, layout="vga", kernelVariant=4)) == 0        # the generic kernel
    assert _applicable(p1, dict(shade, layout="vga", tileSize=64, tileRank=0, tileWorld=2)) == 0
    assert _applicable(p1, dict(layout="brick")) == 0                              # generic
    assert _applicable(dict(p1, stepSize=0.0), dict(shade, layout="vga")) < 0      # the render call's own refusal


def test_header_under_sanitizers():
    """tests/native/order_harness.cpp: the header's own code on random records in exactly-sized heap buffers, ASan + UBSan."""
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "order_harness"
    src = ROOT / "tests" / "native" / "order_harness.cpp"
    hdr = ROOT / "mri-raytracer_amd" / "csrc" / "k1_order.h"
    if not exe.exists() or exe.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        # (the compiler of the other sanitizer harnesses: clang links the sanitizer runtimes statically.  Host code only:
        # the source is plain C++ and -fno-gpu-sanitize keeps the sanitizers off any device code whatever the driver does)
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++", "-std=c++17", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-g", "-O1", f"-I{hdr.parent}", str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    print(out[-3000:])
    assert r.returncode == 0 and "cases ok" in r.stdout, out[-3000:]
