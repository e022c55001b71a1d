"""The fused forward of the coordinate-injection INR and the render driven by it, without a GPU: header, symbols, the LDS layout
(restated here) and the fit rule, every refusal (made before any HIP call), the Python names, the margin proof of the decisive
net of tests/test_gpu_inject_render.py, and the kernel's index arithmetic on the CPU under AddressSanitizer + UBSan
(tests/native/inject_fused_harness.hip, built and run as a program)."""
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

import c5_cases as cc
import inject_cases as ic
import inject_ref as ref
from mrirt import _lib, inr

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
SYMBOLS = ["mrirt_inject_fused_lds_bytes", "mrirt_inject_classify", "mrirt_render_brats_inject"]
NULL, ARG = -1, -5
BUDGET = 160 * 1024
WAVES, WAVE_ROWS = 4, 16
REQUIRED = ["n1_F2_M0_L2", "n63_F14_M1_L3_coords", "n64_F16_M4_L5_both_first_mods_last", "n65_F16_M1_L4_coords_last", "n257_F16_M4_L3_none",
            "int_small", "int_wide", "notebook_shape", "n257_F128_M4_notebook"]
DECISIVE_SCENE = "brick_inside_37x29"


def all_cases():
    """(name, n, F, M, widths, coord layers, mod layers) of every case of EXACT, INTEGER and TOLERANCE."""
    return [c[:7] for c in ic.EXACT + ic.TOLERANCE + ic.INTEGER]


def _desc(F, M, widths, cl, ml):
    d = _lib.InjectDesc()
    d.numLayers, d.fourierDim, d.numMods = len(widths), F, M
    for i, w in enumerate(widths):
        d.width[i] = w
    d.coordLayers, d.modLayers = ref.bits(cl, ml, len(widths))
    return d


def _round(x, to):
    return (x + to - 1) // to * to


def layout(F, M, widths, cl, ml):
    """inj_fused_layout restated: regions as (name, first float, floats) in LDS order, and the total in bytes."""
    shapes = ref.net_shape(F, M, widths, cl, ml)
    L = len(widths)
    k_pad = [_round(s[0], 4) for s in shapes]
    out_pad = [_round(s[3], 16) for s in shapes]
    pitch = [o if o % 32 == 16 else o + 16 for o in out_pad]
    regions, at = [], 0
    for l in range(L):
        regions.append((f"W{l}", at, k_pad[l] * pitch[l]))
        at += k_pad[l] * pitch[l]
    for l in range(L):
        regions.append((f"b{l}", at, out_pad[l]))
        at += out_pad[l]
    regions.append(("B", at, _round(F // 2 * 3, 4)))
    at += _round(F // 2 * 3, 4)
    buf = [0, 0]
    for l in range(L + 1):
        buf[l & 1] = max(buf[l & 1], (k_pad[l] if l < L else 16) * WAVE_ROWS)
    for v in range(WAVES):
        for i in (0, 1):
            regions.append((f"wave{v}buf{i}", at, buf[i]))
            at += buf[i]
    return regions, 4 * at, dict(k_pad=k_pad, out_pad=out_pad, pitch=pitch)


def test_header_symbols_and_sources():
    l = _lib.lib()
    header = (ROOT / "include" / "mrirt.h").read_text()
    for s in SYMBOLS:
        assert s in _lib.ABI_SYMBOLS and hasattr(l, s) and re.search(rf"\b{s}\(", header), s
    assert l.mrirt_abi_version() == 4 and "inr_inject_fused.hip" in _lib.HIP_SOURCES
    assert all(l.mrirt_sizeof(i) == 0 for i in (12, 16, 19, 21, 24, 25))      # no new struct


def test_python_names_and_signatures():
    sig = inspect.signature(inr.inject_fused_ok)
    assert list(sig.parameters) == ["params", "coord_layers", "mod_layers"]
    assert sig.parameters["coord_layers"].default == (1, 2, 3) and sig.parameters["mod_layers"].default == (2,)
    sig = inspect.signature(inr.inject_classify)
    assert list(sig.parameters) == ["params", "coords", "mods", "count", "want_logits", "coord_layers", "mod_layers"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("count", "want_logits", "coord_layers", "mod_layers"))
    assert sig.parameters["count"].default is None and sig.parameters["want_logits"].default is False
    sig, base = inspect.signature(inr.render_brats_inject), inspect.signature(inr.render_brats_inr)
    assert list(sig.parameters) == ["params", "intensities", "net_params", "zmu", "zsigma", "labels", "out", "ext", "return_aux", "chunk_steps",
                                    "one_pass", "coord_layers", "mod_layers"]
    for k in ("labels", "out", "ext", "return_aux", "chunk_steps", "one_pass"):
        assert sig.parameters[k].default == base.parameters[k].default, k


def test_fit_rule_equals_its_restatement_and_takes_the_required_cases():
    l = _lib.lib()
    seen = set()
    for name, n, F, M, widths, cl, ml in all_cases():
        regions, nbytes, _ = layout(F, M, widths, cl, ml)
        got = l.mrirt_inject_fused_lds_bytes(C.byref(_desc(F, M, widths, cl, ml)))
        assert got == (nbytes if nbytes <= BUDGET else 0), (name, got, nbytes)
        at = 0
        for what, first, floats in regions:                       # disjoint, in order, no gaps, 16-byte aligned
            assert first == at and first % 4 == 0 and floats > 0 and floats % 4 == 0, (name, what)
            at += floats
        assert 4 * at == nbytes
        if name in REQUIRED:
            assert 0 < got <= BUDGET, name
            seen.add(name)
        params = ref.glorot_net(np.random.default_rng(0), F, M, widths, cl, ml)
        assert inr.inject_fused_ok(params, cl, ml) == (got > 0), name
    assert seen == set(REQUIRED)
    assert l.mrirt_inject_fused_lds_bytes(C.byref(_desc(128, 4, (64, 64, 64, 4), (1, 2), (2,)))) == 143936      # what the documents state
    refused = [c for c in all_cases() if l.mrirt_inject_fused_lds_bytes(C.byref(_desc(*c[2:7]))) == 0]
    assert "n65_F18_M8_L8_coords_first_both_last" in {c[0] for c in refused} and all(256 in c[4] for c in refused), refused      # only 256-wide nets
    assert l.mrirt_inject_fused_lds_bytes(None) == 0
    assert l.mrirt_inject_fused_lds_bytes(C.byref(_desc(127, 4, (64, 64, 64, 4), (1, 2), (2,)))) == 0            # a shape inj_check_shape refuses


def test_classify_refuses_before_any_hip_call():
    """Host memory stands in for the device buffers: every call below must return before anything is launched or read."""
    l = _lib.lib()
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    ok = _desc(128, 4, (64, 64, 64, 4), (1, 2), (2,))

    def cls(desc=ok, B=p, w=p, b=p, coords=p, mods=p, n=8, count=None, am=p, logits=p):
        return l.mrirt_inject_classify(C.byref(desc) if desc is not None else None, B, w, b, coords, mods, n, count, am, logits, None)

    for kw in ("desc", "B", "w", "b", "coords", "mods"):
        assert cls(**{kw: None}) == NULL, kw
    assert cls(am=None, logits=None) == NULL
    for n in (0, -1, 1 << 31, 1 << 40):
        assert cls(n=n) == ARG, n
    for bad in (dict(F=127), dict(widths=(64, 64, 64, 17)), dict(cl=(0, 1)), dict(M=9)):
        kw = dict(F=128, M=4, widths=(64, 64, 64, 4), cl=(1, 2), ml=(2,))
        kw.update(bad)
        d = _desc(**kw)
        if "cl" in bad:
            d.coordLayers = 0b11                                  # bit 0: ref.bits drops it, the ABI must refuse it
        assert cls(desc=d) == ARG and l.mrirt_inject_fused_lds_bytes(C.byref(d)) == 0, bad
    for name in ("n65_F18_M8_L8_coords_first_both_last", "n257_F256_M8_L3_mods"):      # shapes the chain takes and the fit rule refuses
        case = next(c for c in ic.EXACT if c[0] == name)
        assert cls(desc=_desc(*case[2:7])) == ARG, name
    assert cls(desc=_desc(2, 0, (13, 4), (), ()), mods=None, n=0) == ARG      # no modalities: no mods pointer needed, n is looked at


def test_render_refuses_its_network_before_any_hip_call():
    l = _lib.lib()
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    ok = _desc(128, 4, (64, 64, 64, 4), (1, 2), (2,))
    P, E = _lib.BratsParams(), _lib.RenderExt()
    vols = (C.c_void_p * 4)(p, p, p, p)
    z = (C.c_float * 4)(0, 0, 0, 0)
    one = (C.c_float * 4)(1, 1, 1, 1)

    def rnd(P=P, E=E, vp=vols, lab=None, desc=ok, B=p, w=p, b=p, mu=z, sg=one, chunk=4, scratch=p, nbytes=1 << 40, out=p, pitch=64):
        return l.mrirt_render_brats_inject(C.byref(P) if P is not None else None, C.byref(E), vp, lab, C.byref(desc) if desc is not None else None,
                                           B, w, b, mu, sg, chunk, scratch, nbytes, out, pitch, None, None)

    for kw in ("desc", "B", "w", "b", "vp", "mu", "sg", "scratch", "out"):
        assert rnd(**{kw: None}) == NULL, kw
    holed = (C.c_void_p * 4)(p, p, None, p)
    assert rnd(vp=holed) == NULL
    tiled = _lib.RenderExt()
    tiled.tileSize = 8
    assert rnd(E=tiled) == ARG
    assert rnd(desc=_desc(128, 3, (64, 64, 64, 4), (1, 2), (2,))) == ARG        # three modalities
    assert rnd(desc=_desc(128, 4, (64, 64, 64, 17), (1, 2), (2,))) == ARG       # a shape inj_check_shape refuses
    wide = next(c for c in ic.TOLERANCE if c[0] == "widths_256_32_96")
    assert l.mrirt_inject_fused_lds_bytes(C.byref(_desc(*wide[2:7]))) == 0 and rnd(desc=_desc(*wide[2:7])) == ARG
    assert rnd(P=None) == NULL                                   # prepare()'s refusal, still before any HIP call
    assert rnd() == -2                                           # a zeroed params block: MRIRT_ERR_DIMS


# ---- the decisive net of tests/test_gpu_inject_render.py ------------------------------------------------------------------------
def decisive_inject(net: cc.Net, seed=77):
    """An injection net of the notebook's shape (F 128, widths 64 / 64 / 64 / 4, coordinates into layers 1 and 2, modalities into
    layer 2) whose class is cc.rule(net): `a` where the z-scored modality x_f > 0, `b` where x_f < 0.  Unit 0 of layer 0 is
    relu(+x_f), unit 1 relu(-x_f), each through ONE weight of +-1; layers 1 and 2 copy the two with weight 1; the head gives
    class a unit 0 and class b unit 1, every other class a bias of -4.  Every other weight of columns 0 and 1 is zero, so each
    of their sums holds one non-zero term and zeros times finite values: exact in any order.  The other hidden units carry
    seeded junk (Fourier rows, coordinates and modalities included) that the head does not read."""
    assert net.f >= 3 and net.out == 4
    F, M, widths, cl, ml = 128, 4, (64, 64, 64, 4), (1, 2), (2,)
    params = ref.glorot_net(np.random.default_rng(seed), F, M, widths, cl, ml)
    mlp = params["mlp"]
    for l in range(3):
        mlp[l]["W"][:, :2] = 0.0
        mlp[l]["b"][:2] = 0.0
    mlp[0]["W"][F + net.f - 3, 0] = 1.0
    mlp[0]["W"][F + net.f - 3, 1] = -1.0
    for l in (1, 2):
        mlp[l]["W"][0, 0] = mlp[l]["W"][1, 1] = 1.0
    mlp[3]["W"][:] = 0.0
    mlp[3]["b"][:] = -4.0
    mlp[3]["W"][0, net.a] = mlp[3]["W"][1, net.b] = 1.0
    mlp[3]["b"][[net.a, net.b]] = 0.0
    return params, cl, ml


def test_the_decisive_net_has_an_exact_margin():
    """Over every sample of the scene the logits are EXACTLY (relu(x) at a, relu(-x) at b, -4 elsewhere) with |x| >= 2^-20
    (tests/test_c5_cases_host.py holds the scene to that), so the class is the rule's whatever order the sums take."""
    import c5_ref as cr
    case, r = cc.CASES[DECISIVE_SCENE], cr.reference(DECISIVE_SCENE)
    params, cl, ml = decisive_inject(case.net)
    coords, feats = r["coords"][::7], r["feats"][::7]             # every seventh sample: the sums do not depend on the row
    x = cc.feature(case.net, coords, feats)
    assert x.size > 1000 and float(np.abs(x).min()) >= cc.MARGIN and (x > 0).any() and (x < 0).any()
    z = ref.forward32(params, coords, feats, cl, ml)
    want = np.full_like(z, -4.0)
    want[:, case.net.a] = np.maximum(x, 0)
    want[:, case.net.b] = np.maximum(-x, 0)
    assert ref.same_bits(z, want)
    assert np.array_equal(ref.argmax(z), cc.rule(case.net, coords, feats))
    for l in range(3):                                            # columns 0 and 1: one non-zero weight each
        assert (np.count_nonzero(params["mlp"][l]["W"][:, :2], axis=0) == 1).all()


# ---- the index arithmetic under the sanitizers --------------------------------------------------------------------------------
def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "inject_fused_harness"
    src = ROOT / "tests" / "native" / "inject_fused_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "inject_fused_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", *SAN, "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "inject_fused_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


def _blob(params, F, M, widths, cl, ml, n_max, count, coords, mods):
    cbits, mbits = ref.bits(cl, ml, len(widths))
    w, b = ref.flat(params)
    rows = n_max if count is None else min(count, n_max)
    hd = [len(widths), F, M, *widths, *([0] * (8 - len(widths))), cbits, mbits, n_max, 0 if count is None else 1, count or 0]
    out = struct.pack("<16I", *hd) + np.asarray(params["fourier"]["B"], np.float32).tobytes() + w.tobytes() + b.tobytes()
    out += np.ascontiguousarray(coords[:rows], np.float32).tobytes()
    return out + np.ascontiguousarray(np.asarray(mods, np.float32).reshape(len(coords), M)[:rows], np.float32).tobytes(), rows


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_index_arithmetic_under_asan_and_ubsan(tmp_path):
    exe = build_harness()
    l = _lib.lib()
    cases, blob = [], b""

    def add(name, params, F, M, widths, cl, ml, coords, mods, counts):
        nonlocal blob
        if l.mrirt_inject_fused_lds_bytes(C.byref(_desc(F, M, widths, cl, ml))) == 0:
            return
        for count in counts:
            piece, rows = _blob(params, F, M, widths, cl, ml, len(coords), count, coords, mods)
            blob += piece
            cases.append((name, params, F, M, widths, cl, ml, coords[:rows], np.asarray(mods, np.float32).reshape(len(coords), M)[:rows], rows))

    for case in ic.EXACT:                                         # every accepted case; counts on both sides of a wave's and a tile's edge
        name, n, F, M, widths, cl, ml, _ = case
        params, _, coords, mods = ic.exact_case(case)
        add(name, params, F, M, widths, cl, ml, coords, mods, [None] + [c for c in (0, 15, 16, 17, 63, 64, 65, 1000) if n >= 64])
    for case in ic.INTEGER:
        name, n, F, M, widths, cl, ml, _ = case
        params, coords8, mods = ic.integer_case(case)
        add(name, params, F, M, widths, cl, ml, (coords8 / 8.0).astype(np.float32), mods.astype(np.float32), [None, 64, 65])
    assert {c[0] for c in cases} >= {"n1_F2_M0_L2", "n63_F14_M1_L3_coords", "n64_F16_M4_L5_both_first_mods_last", "n65_F16_M1_L4_coords_last",
                                     "n257_F16_M4_L3_none", "n257_F128_M4_notebook", "int_small", "int_wide"}
    path, outp = tmp_path / "cases.bin", tmp_path / "out.bin"
    path.write_bytes(struct.pack("<I", len(cases)) + blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(path), str(outp)], capture_output=True, text=True, env=env, timeout=900)
    out = r.stdout + r.stderr
    print(out[-6000:])
    assert r.returncode == 0, out[-6000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "FAILED" not in out, out[-6000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert len(lines) == len(cases) and f"inject_fused_harness: {len(cases)} cases done" in r.stdout
    raw, at = outp.read_bytes(), 0
    for ln, (name, params, F, M, widths, cl, ml, coords, mods, rows) in zip(lines, cases):
        # the LDS block the harness ran in (ASan-checked, exactly this long) is what the launch asks for
        assert int(ln[3]) == l.mrirt_inject_fused_lds_bytes(C.byref(_desc(F, M, widths, cl, ml))) and int(ln[5]) == rows, name
        Cn = widths[-1]
        got = np.frombuffer(raw, np.float32, rows * Cn, at).reshape(rows, Cn); at += 4 * rows * Cn
        am = np.frombuffer(raw, np.int16, rows, at); at += 2 * rows
        if rows:
            want = ref.forward32(params, coords, mods, cl, ml)
            assert ref.same_bits(got, want), name
            assert np.array_equal(am, ref.argmax(want)), name
    assert at == len(raw)
