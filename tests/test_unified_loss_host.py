"""The unified loss and the samplers' field gather without a GPU: header, symbols and the struct's size, every refusal and
their order (made before any HIP call, on host memory), the scratch formula restated, the Python names that need no device, and
the kernels' index arithmetic on the CPU under AddressSanitizer + UBSan (tests/native/unified_loss_harness.hip, built and run as
a program the way test_inject_train_host.py builds its harness)."""
import ctypes as C
import inspect
import os
import pathlib
import re
import shutil
import subprocess

import pytest

from mrirt import _lib, inr
from test_inr_loop_host import BAD, ERR_ARG, ERR_DIMS, ERR_NULL, INF, NAN, P, cache

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
SYMBOLS = ["mrirt_unified_loss_scratch_bytes", "mrirt_unified_loss", "mrirt_inr_sample_field"]


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def cfg(gamma=0.5, lam=0.5, alpha=0.3, beta=0.7, ufl=0.5, dice=0.5, tv=0.02, bd=0.1, flags=0, cw=1.0):
    x = _lib.UnifiedLoss()
    for k in range(16):
        x.classWeights[k] = cw[k] if isinstance(cw, (list, tuple)) else cw
    x.gamma, x.lambda_, x.tverskyAlpha, x.tverskyBeta = gamma, lam, alpha, beta
    x.uflWeight, x.diceWeight, x.tvWeight, x.boundaryWeight, x.flags = ufl, dice, tv, bd, flags
    return x


def test_header_symbols_and_struct_size(lib):
    header = (ROOT / "include" / "mrirt.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in SYMBOLS:
        assert s in _lib.ABI_SYMBOLS and hasattr(lib, s) and re.search(rf"\b{s}\s*\(", code), s
    assert "typedef struct MrirtUnifiedLoss" in code and header.count("typedef struct MrirtInject") == 2
    assert lib.mrirt_sizeof(20) == C.sizeof(_lib.UnifiedLoss) == 16 * 4 + 8 * 4 + 4
    assert lib.mrirt_sizeof(19) == 0 and lib.mrirt_sizeof(12) == 0 and lib.mrirt_sizeof(16) == 0 and lib.mrirt_sizeof(21) == 0
    assert lib.mrirt_abi_version() == 4
    assert "inr_unified.hip" in _lib.HIP_SOURCES and (_lib.CSRC / "inr_unified.h").exists()
    assert [f[0] for f in _lib.UnifiedLoss._fields_] == ["classWeights", "gamma", "lambda_", "tverskyAlpha", "tverskyBeta", "uflWeight", "diceWeight",
                                                         "tvWeight", "boundaryWeight", "flags"]


def test_no_torch_operator_was_added():
    src = (_lib.CSRC / "torch_binding.cpp").read_text()
    assert len(re.findall(r"\bm\.def\(", src)) == 19 and "unified" not in src


def test_scratch_bytes_is_the_stated_layout_and_monotone_in_n(lib):
    f = lib.mrirt_unified_loss_scratch_bytes
    ns = [1, 2, 255, 256, 257, 4000, 65536, 65537, 1 << 20, 2 ** 31 - 1]
    sizes = [f(n) for n in ns]
    for n, v in zip(ns, sizes):
        assert v == ((min((n + 255) // 256, 256) + 2) * 83 * 8 + 255) & ~255, n
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and all(v % 256 == 0 for v in sizes)
    assert all(a <= b for a, b in zip([f(n) for n in range(250, 1030)], [f(n) for n in range(251, 1031)]))
    for n in (0, -1, 2 ** 31, 2 ** 40):
        assert f(n) == 0
    # the loss has a scratch of its own: it does not fit the loss prefix of the injection step's scratch
    assert f(4000) > lib.mrirt_inr_loss_scratch_bytes(4000)


def test_unified_loss_refusals_and_their_order(lib):
    """Host memory stands in for the device buffers: every call below must return before anything is launched or read."""
    f = lib.mrirt_unified_loss
    n, nc = 1000, 4
    nbytes = lib.mrirt_unified_loss_scratch_bytes(n)
    ok = [P, P, P, n, nc, C.byref(cfg()), P, P, P, P, nbytes, None]
    for i in (0, 1, 5, 6, 7, 9):                         # logits, labels, cfg, loss, aux, scratch; boundary_w and dlogits may be NULL
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for i, v in ((3, 0), (3, -1), (3, 2 ** 31), (4, 0), (4, 17), (10, nbytes - 1), (10, 0), (10, -1), (9, BAD)):
        a = list(ok); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)
    bad = [dict(gamma=0.2499), dict(gamma=0.0), dict(gamma=1.0001), dict(gamma=2.0), dict(gamma=-0.5), dict(gamma=NAN), dict(gamma=INF),
           dict(lam=-0.001), dict(lam=1.001), dict(lam=NAN), dict(lam=INF), dict(alpha=-0.1), dict(alpha=NAN), dict(alpha=INF), dict(beta=-0.1),
           dict(beta=NAN), dict(beta=INF), dict(ufl=-1.0), dict(ufl=NAN), dict(ufl=INF), dict(dice=-1.0), dict(dice=NAN), dict(dice=INF),
           dict(tv=-0.01), dict(tv=NAN), dict(tv=INF), dict(bd=-0.1), dict(bd=NAN), dict(bd=INF), dict(flags=1), dict(flags=1 << 31),
           dict(cw=-1.0), dict(cw=NAN), dict(cw=INF), dict(cw=[1.0, 1.0, 1.0, -0.5] + [1.0] * 12)]
    for kw in bad:
        a = list(ok); a[5] = C.byref(cfg(**kw))
        assert f(*a) == ERR_ARG, kw
    # what is accepted gets as far as the scratch check (nothing here may reach a launch: the pointers are not real)
    good = [dict(), dict(gamma=0.25), dict(gamma=1.0), dict(lam=0.0), dict(lam=1.0), dict(alpha=0.0, beta=0.0), dict(ufl=0.0, dice=0.0, tv=0.0, bd=0.0),
            dict(alpha=5.0), dict(cw=0.0), dict(cw=[1.0, 1.0, 1.0, 1.0] + [NAN] * 12)]      # only the first C class weights are read
    for kw in good:
        a = list(ok); a[5] = C.byref(cfg(**kw)); a[10] = nbytes - 1
        assert f(*a) == ERR_ARG, kw
        a[9] = None
        assert f(*a) == ERR_NULL, kw
    # the order: a NULL pointer (the scratch included) before any bad argument; n, C, gamma, lambda, the weights, the flags, the scratch
    a = list(ok); a[9] = None; a[3] = 0
    assert f(*a) == ERR_NULL
    a = list(ok); a[0] = None; a[5] = C.byref(cfg(gamma=5.0)); a[10] = 0
    assert f(*a) == ERR_NULL
    # ... and each ARG check before the later ones cannot be told apart by the code alone: every one of them precedes the
    # scratch check, which the `good` loop above shows is reached last
    a = list(ok); a[5] = C.byref(cfg(flags=2)); a[9] = BAD
    assert f(*a) == ERR_ARG
    a = list(ok); a[2] = None; a[8] = None; a[10] = nbytes - 1      # boundary_w and dlogits NULL: still only the scratch is wrong
    assert f(*a) == ERR_ARG


def test_sample_field_refusals(lib):
    f = lib.mrirt_inr_sample_field
    t = _lib.InrTumourIndex(0x1000, 0x1000)
    ok = [C.byref(cache()), C.byref(t), P, 1, 0, 100, 40, P, None]
    for i in (0, 1, 2, 7):                                # cache, index (n_tumour > 0), fields, out
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for bad in (_lib.InrTumourIndex(None, 0x1000), _lib.InrTumourIndex(0x1000, None)):
        a = list(ok); a[1] = C.byref(bad)
        assert f(*a) == ERR_NULL
    for n, nt in ((100, 101), (100, -1), (0, 0), (2 ** 31, 0), (1, 2)):
        a = list(ok); a[5], a[6] = n, nt
        assert f(*a) == ERR_ARG, (n, nt)
    assert f(C.byref(cache(hwd=(1, 5, 7))), C.byref(t), P, 1, 0, 100, 40, P, None) == ERR_DIMS
    assert f(C.byref(cache(ncases=0)), C.byref(t), P, 1, 0, 100, 40, P, None) == ERR_ARG
    # the mixed sampler's own refusals, in its order: the same arguments give the same code
    mix = lib.mrirt_inr_sample_batch_mix
    for c, tt, n, nt in ((cache(hwd=(1, 5, 7)), t, 100, 40), (cache(), None, 100, 40), (cache(), t, 0, 0), (cache(seg=None), t, 100, 0)):
        tp = C.byref(tt) if tt is not None else None
        assert f(C.byref(c), tp, P, 1, 0, n, nt, P, None) == mix(C.byref(c), tp, 1, 0, n, nt, P, P, P, None) != 0


def test_python_names_and_defaults():
    sig = inspect.signature(inr.unified_loss)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [("gamma", 0.5), ("lam", 0.5), ("alpha", 0.3), ("beta", 0.7), ("ufl_weight", 0.5),
                                                                               ("dice_weight", 0.5), ("tv_weight", 0.02), ("boundary_weight", 0.1)]
    x = inr.unified_loss([0.1, 1.5, 1.0, 2.0])
    assert isinstance(x, _lib.UnifiedLoss) and x.flags == 0 and x.gamma == 0.5 and x.lambda_ == 0.5 and abs(x.tverskyAlpha - 0.3) < 1e-7
    assert [x.classWeights[k] for k in range(5)] == [C.c_float(v).value for v in (0.1, 1.5, 1.0, 2.0, 0.0)]
    with pytest.raises(ValueError):
        inr.unified_loss([1.0] * 17)
    assert list(inspect.signature(inr.unified_loss_and_dlogits).parameters) == ["logits", "labels", "cfg", "boundary_w", "scratch", "want_grad"]
    assert list(inspect.signature(inr.VoxelCache.sample_field).parameters) == ["self", "seed", "batch_index", "n", "n_tumour"]
    assert list(inspect.signature(inr.VoxelCache.set_boundary).parameters) == ["self", "maps"]
    doc = inr.train_inject.__doc__
    assert "UNIFIED_FOCAL_GAMMA" in doc and "TV_WEIGHT_STAGE2" in doc and "unified loss, hybrid sampler" not in doc


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "unified_loss_harness"
    src = ROOT / "tests" / "native" / "unified_loss_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "unified_loss_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "unified_loss_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_index_arithmetic_under_asan_and_ubsan(lib):
    exe = build_harness()
    loss = [(1, 1), (1, 16), (255, 3), (256, 4), (257, 4), (4000, 4), (65536, 4), (65537, 16), (70001, 1)]
    field = [(2, 5, 4, 3, 300, 0), (2, 5, 4, 3, 300, 120), (3, 5, 4, 3, 257, 257), (4, 9, 7, 6, 1000, 600), (1, 2, 2, 2, 64, 64)]
    args = [str(v) for item in loss for v in ("l", *item)] + [str(v) for item in field for v in ("f", *item)] + ["big"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert r.returncode == 0, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("item ")]
    assert len(lines) == len(loss) + len(field) + 1 and all(ln[-1] == "0" for ln in lines)
    assert f"unified_loss_harness: {len(lines)} items, 0 failed" in r.stdout
    for ln, (n, c) in zip(lines, loss):
        # the buffer the harness ran in (ASan-checked, exactly this long) is what the ABI tells callers to allocate
        assert int(ln[10]) == lib.mrirt_unified_loss_scratch_bytes(n) and int(ln[5]) == min((n + 255) // 256, 256), (n, c)
    used = [(int(ln[11]), int(ln[13])) for ln in lines if ln[1] == "f"]
    assert used[0] == (0, 0) and all(a > 0 and b > 0 for a, b in used[1:4])      # points from the index, and the fallback fill fired
    assert used[4] == (0, 4 * 64)                                                # one case without tumour: nothing but the fallback
