"""The coordinate-injection INR's training step without a GPU: header, symbols, every refusal (made before any HIP call), the
scratch formula, the Python names that need no device (two_stage_schedule, inject_init), and the new index arithmetic on the
CPU under AddressSanitizer + UBSan (tests/native/inject_train_harness.hip, built and run as a program the way
test_inject_host.py builds inject_harness.hip)."""
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
import inject_train_cases as tc
import inject_train_ref as tref
from mrirt import _lib, inr
from test_inject_host import BAD_DESCS, HIPCC, OUT, ROOT, SAN, _desc, _drop

SYMBOLS = ["mrirt_inject_train_scratch_bytes", "mrirt_inject_forward_train", "mrirt_inject_backward"]
NULL, ARG = -1, -5


def test_header_symbols_and_no_new_struct():
    l = _lib.lib()
    header = (ROOT / "include" / "mrirt.h").read_text()
    for s in SYMBOLS:
        assert s in _lib.ABI_SYMBOLS and hasattr(l, s) and re.search(rf"\b{s}\(", header), s
    assert l.mrirt_sizeof(19) == 0 and l.mrirt_abi_version() == 4
    assert "inr_inject_train.hip" in _lib.HIP_SOURCES
    assert header.count("typedef struct MrirtInject") == 2


def test_abi_rejects_malformed_arguments_before_any_hip_call():
    """Host memory stands in for the device buffers: every call below must return before anything is launched or read."""
    l = _lib.lib()
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    big = 1 << 40
    ok = _desc()

    def fwd(desc=ok, B=p, w=p, b=p, coords=p, mods=p, n=8, drop=None, logits=p, scratch=p, nbytes=big):
        return l.mrirt_inject_forward_train(C.byref(desc) if desc is not None else None, B, w, b, coords, mods, n,
                                            C.byref(drop) if drop is not None else None, logits, scratch, nbytes, None)

    def bwd(desc=ok, B=p, w=p, coords=p, mods=p, n=8, drop=None, dl=p, gB=p, gw=p, gb=p, flags=0, scratch=p, nbytes=big):
        return l.mrirt_inject_backward(C.byref(desc) if desc is not None else None, B, w, coords, mods, n,
                                       C.byref(drop) if drop is not None else None, dl, gB, gw, gb, flags, scratch, nbytes, None)

    for kw in ("desc", "B", "w", "b", "coords", "mods", "logits", "scratch"):
        assert fwd(**{kw: None}) == NULL, kw
    for kw in ("desc", "B", "w", "coords", "mods", "dl", "gB", "gw", "gb", "scratch"):
        assert bwd(**{kw: None}) == NULL, kw
    for name, kw in BAD_DESCS.items():
        d = _desc(**kw)
        assert fwd(desc=d) == ARG and bwd(desc=d) == ARG, name
        assert l.mrirt_inject_train_scratch_bytes(C.byref(d), 8) == 0, name
    for n in (0, -1, 1 << 31):
        assert fwd(n=n) == ARG and bwd(n=n) == ARG and l.mrirt_inject_train_scratch_bytes(C.byref(ok), n) == 0
    for bad in (_drop(keep=0.0), _drop(keep=-0.5), _drop(keep=1.5), _drop(keep=float("nan")), _drop(keep=1e-45), _drop(samples=0),
                _drop(samples=2), _drop(sample0=1 << 24), _drop(reserved=1)):
        assert fwd(drop=bad) == ARG and bwd(drop=bad) == ARG, (bad.keep, bad.samples, bad.sample0)
    for flags in (2, 3, 4, 1 << 31):
        assert bwd(flags=flags) == ARG, flags
    need = l.mrirt_inject_train_scratch_bytes(C.byref(ok), 8)
    assert need > 0
    for call in (fwd, bwd):
        assert call(nbytes=need - 1) == ARG and call(nbytes=0) == ARG and call(nbytes=-1) == ARG
        assert call(scratch=C.c_void_p(p.value + 4)) == ARG      # misaligned
        assert call(drop=_drop(keep=1.0), nbytes=0) == ARG and call(drop=_drop(keep=0.5), nbytes=0) == ARG      # a good dropout gets as far as the scratch
    assert bwd(flags=1, nbytes=0) == ARG
    assert l.mrirt_inject_train_scratch_bytes(None, 8) == 0
    # a net without modalities needs no mods pointer: the call gets as far as the scratch check
    d0 = _desc(M=0, ml=0)
    assert fwd(desc=d0, mods=None, nbytes=0) == ARG and bwd(desc=d0, mods=None, nbytes=0) == ARG
    # the order of the checks: a NULL pointer before a bad n, a bad n before a bad dropout, a bad flag before the scratch
    assert fwd(B=None, n=0) == NULL and bwd(B=None, n=0) == NULL
    assert bwd(gB=None, flags=2) == NULL and bwd(flags=2, scratch=None) == ARG


def _layout(d, n):
    """The scratch layout of include/mrirt.h, restated."""
    al = lambda v: (v + 255) & ~255
    L, F, M = d.numLayers, d.fourierDim, d.numMods
    widths = [d.width[i] for i in range(L)]
    shapes = ref.net_shape(F, M, widths, [l for l in range(L) if d.coordLayers >> l & 1], [l for l in range(L) if d.modLayers >> l & 1])
    loss = _lib.lib().mrirt_inr_loss_scratch_bytes(n)
    total = loss + al(4 * n * F) + sum(al(4 * n * w) for w in widths[:-1]) + 2 * al(4 * n * max(widths[:-1])) + al(4 * n * F) + al(4 * n * 3)
    elems = max(max((s[0] + 1) * s[3] for s in shapes), 3 * F // 2)
    return total + al(4 * min((n + 255) // 256, 64) * elems)


def test_scratch_bytes_is_the_stated_layout_and_monotone_in_n():
    l = _lib.lib()
    ns = [1, 2, 63, 64, 65, 100, 256, 257, 4000, 4096, 16384, 16385, 50000, 65536, 1 << 20, (1 << 31) - 1]
    for d in (_desc(), _desc(L=2, F=2, M=0, widths=(1, 1), cl=0, ml=0), _desc(L=2, F=256, M=0, widths=(1, 1), cl=0, ml=0),
              _desc(L=3, F=256, M=8, widths=(256, 256, 16), cl=2, ml=2), _desc(L=8, F=18, M=8, widths=(64, 256, 16, 1, 65, 17, 13, 16), cl=0b1000010, ml=0b1000000)):
        sizes = [l.mrirt_inject_train_scratch_bytes(C.byref(d), n) for n in ns]
        assert all(v > 0 and v % 256 == 0 for v in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        for n, v in zip(ns, sizes):
            assert v == _layout(d, n), n
            assert v >= l.mrirt_inr_loss_scratch_bytes(n) > 0
    # every n in a range that crosses the first doubling of the slab length (64 slabs of 256 -> 33 of 512)
    d = _desc()
    sizes = [l.mrirt_inject_train_scratch_bytes(C.byref(d), n) for n in range(16380, 16390)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))


def test_two_stage_schedule_matches_cell_11():
    sig = inspect.signature(inr.two_stage_schedule)
    assert list(sig.parameters) == ["stage1_steps", "stage2_steps", "lr_stage1", "lr_stage2", "warmup_steps", "min_lr"]
    for s1, s2, lr1, lr2, warm, lo in ((5000, 5000, 2e-3, 5e-4, 300, 1e-5), (10, 7, 1e-2, 1e-3, 3, 1e-4), (4, 0, 1e-3, 5e-4, 1, 1e-5), (6, 2, 1.0, 0.5, 0, 0.25)):
        f = inr.two_stage_schedule(s1, s2, lr1, lr2, warm, lo)
        for t in sorted({0, 1, warm - 1, warm, warm + 1, s1 - 1, s1, s1 + 1, s1 + s2 - 1, s1 + s2} - {-1}):
            if s2 == 0 and t >= s1:
                assert f(t) == lo                               # the notebook's last branch would divide by zero; it never gets there
                continue
            got, want = f(t), tref.two_stage_lr(t, s1, s2, lr1, lr2, warm, lo)
            assert isinstance(got, float) and got == want, (t, got, want)
    f = inr.two_stage_schedule(5000, 5000, 2e-3, 5e-4, 300, 1e-5)
    assert f(0) == 0.0 and f(300) == 2e-3 and f(5000) == 5e-4 and f(10000) == 1e-5


def test_inject_init_shapes_and_limits():
    sig = inspect.signature(inr.inject_init)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("fourier_dim", 128), ("num_mods", 4), ("hidden_dims", (64, 64, 64)), ("out_dim", 4), ("coord_layers", (1, 2, 3)), ("mod_layers", (2,)),
        ("sigma", 5.0), ("voxel_spacing", (1, 1, 1))]
    p = inr.inject_init(3)
    assert p["fourier"]["B"].shape == (64, 3) and p["fourier"]["B"].dtype == np.float32
    assert [q["W"].shape for q in p["mlp"]] == [(132, 64), (67, 64), (71, 64), (64, 4)]          # index 3 of the notebook's list names the head
    d = inr.inject_desc(p)
    assert (d.numLayers, d.fourierDim, d.numMods, d.coordLayers, d.modLayers) == (4, 128, 4, 0b110, 0b100)
    for q in p["mlp"]:
        lim = np.sqrt(6.0 / sum(q["W"].shape))
        assert q["W"].dtype == np.float32 and np.abs(q["W"]).max() <= np.float32(lim) and np.abs(q["W"]).max() > 0.9 * lim
        assert abs(float(q["W"].mean())) < 0.1 * lim
        assert q["b"].dtype == np.float32 and q["b"].shape == (q["W"].shape[1],) and not q["b"].any()
    big = inr.inject_init(3, fourier_dim=256, sigma=5.0)["fourier"]["B"]
    assert 4.5 < big.std() < 5.5 and abs(big.mean()) < 0.6
    an = inr.inject_init(3, fourier_dim=256, voxel_spacing=(1.0, 2.0, 4.0))["fourier"]["B"]
    assert np.allclose(an * np.float32([1, 2, 4]), big, rtol=1e-6)
    assert ref.same_bits(inr.inject_init(3)["mlp"][1]["W"], p["mlp"][1]["W"]) and not ref.same_bits(inr.inject_init(4)["mlp"][1]["W"], p["mlp"][1]["W"])
    q = inr.inject_init(1, 16, 0, (17, 13), 3, (1,), ())
    assert [x["W"].shape for x in q["mlp"]] == [(16, 17), (20, 13), (13, 3)]
    sig = inspect.signature(inr.make_inject_loss_and_grad)
    assert list(sig.parameters) == ["num_classes", "class_weights", "dice_weight", "coord_layers", "mod_layers", "ext"]
    assert list(inspect.signature(inr.train_inject).parameters) == ["config", "cases_or_cache", "params", "log", "save_path"]
    assert list(inspect.signature(inr.inject_autograd).parameters) == ["B", "Ws", "bs", "coords", "mods", "coord_layers", "mod_layers", "dropout"]


def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "inject_train_harness"
    src = ROOT / "tests" / "native" / "inject_train_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "inject_train_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "inject_train_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


def _blob(params, F, M, widths, cl, ml, n, coords, mods, dl, drop, old):
    cbits, mbits = ref.bits(cl, ml, len(widths))
    w, b = ref.flat(params)
    hd = [len(widths), F, M, *widths, *([0] * (8 - len(widths))), cbits, mbits, n, 1 if drop else 0, drop["s"] if drop else 0]
    out = struct.pack("<16I", *hd) + struct.pack("<QfI", drop["seed"] if drop else 0, drop["keep"] if drop else 1.0, 1 if old else 0)
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    out += f32(params["fourier"]["B"]) + w.tobytes() + b.tobytes() + f32(coords) + f32(mods) + f32(dl)
    if old:
        out += f32(old["B"]) + b"".join(f32(x) for x in old["W"]) + b"".join(f32(x) for x in old["b"])
    return out


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_index_arithmetic_under_asan_and_ubsan(tmp_path):
    exe = build_harness()
    l = _lib.lib()
    cases, blob = [], b""
    for k, case in enumerate(ic.EXACT):                        # the selection nets: real sines, special inputs, every split
        name, n, F, M, widths, cl, ml, _ = case
        params, _, coords, mods = tc.selection_case(case)
        rng = np.random.default_rng(k)
        drop = tc.dropout_of(0.5) if k % 2 == 0 else None
        dl = tc.one_row_per_slab(rng, n, widths[-1], tc.SELECTION_ROWS[k % len(tc.SELECTION_ROWS)])
        want = tref.backward32(params, coords, mods, cl, ml, dl, drop)
        blob += _blob(params, F, M, widths, cl, ml, n, coords, mods, dl, drop, None)
        cases.append((name, params, F, M, widths, cl, ml, n, coords, mods, drop, want))
    for case in tc.INTEGER:                                    # the integer nets up to 321 points: 64 and 65 rows, accumulation
        name, n, F, M, widths, cl, ml, _, _, _ = case
        if n > 321:
            continue
        params, c8, mods, dl, drop, old = tc.integer_case(case)
        coords = (c8 / 8.0).astype(np.float32)
        want = tref.backward32(params, coords, mods, cl, ml, dl.astype(np.float32), drop, old=old)
        blob += _blob(params, F, M, widths, cl, ml, n, coords, mods, dl, drop, old)
        cases.append((name, params, F, M, widths, cl, ml, n, coords, mods, drop, want))
    path, outp = tmp_path / "cases.bin", tmp_path / "out.bin"
    path.write_bytes(struct.pack("<I", len(cases)) + blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(path), str(outp)], capture_output=True, text=True, env=env, timeout=900)
    out = r.stdout + r.stderr
    print(out[-6000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "FAILED" not in out, out[-6000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert len(lines) == len(cases) and f"inject_train_harness: {len(cases)} cases done" in r.stdout
    raw, at = outp.read_bytes(), 0
    for ln, (name, params, F, M, widths, cl, ml, n, coords, mods, drop, want) in zip(lines, cases):
        cbits, mbits = ref.bits(cl, ml, len(widths))
        d = _desc(len(widths), F, M, widths, cbits, mbits)
        # the buffer the harness ran in (ASan-checked, exactly this long) is what the ABI tells callers to allocate
        assert int(ln[3]) == l.mrirt_inject_train_scratch_bytes(C.byref(d), n), name
        assert int(ln[5]) == (n + tref.slab_len(n) - 1) // tref.slab_len(n), name
        w, b = ref.flat(params)
        sizes = [n * widths[-1], 3 * F // 2, w.size, b.size]
        logits, gB, gw, gb = [np.frombuffer(raw, np.float32, s, at + 4 * sum(sizes[:i])) for i, s in enumerate(sizes)]
        at += 4 * sum(sizes)
        assert ref.same_bits(logits.reshape(n, -1), ref.forward32(params, coords, mods, cl, ml, drop)), name
        assert ref.same_bits(gB.reshape(-1, 3), want["B"]), name
        assert ref.same_bits(gw, np.concatenate([x.reshape(-1) for x in want["W"]])), name
        assert ref.same_bits(gb, np.concatenate(want["b"])), name
    assert at == len(raw)
