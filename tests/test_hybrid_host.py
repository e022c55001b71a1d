"""The hybrid sampler and the coordinate noise without a GPU: the NumPy / Python-int restatement pinned on
the CPU (tests/hybrid_ref.py), header, symbols and struct sizes, every refusal and their order (made before any HIP call, on host
memory), the scratch formula restated, the Python names that need no device, and the kernels' index arithmetic and draws on the
CPU under AddressSanitizer + UBSan (tests/native/hybrid_harness.hip, built and run as a program the way
test_unified_loss_host.py builds its harness)."""
import ctypes as C
import inspect
import os
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import hybrid_cases as hc
import hybrid_ref as ref
import inr_loop_ref as lp
import inr_lossx_ref as lx
from mrirt import _lib, inr
from test_inr_loop_host import BAD, ERR_ARG, ERR_DIMS, ERR_NULL, INF, NAN, P, cache

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "native" / "_build"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
SYMBOLS = ["mrirt_inr_class_count", "mrirt_inr_class_index_scratch_bytes", "mrirt_inr_class_index", "mrirt_select_largest", "mrirt_inr_normal3",
           "mrirt_inr_sample_candidates", "mrirt_inr_sample_batch_hybrid"]


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


# ---- the restatement, pinned ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hwd,ncases,nc", [((5, 4, 3), 1, 1), ((5, 4, 3), 3, 4), ((17, 16, 16), 2, 16), ((9, 7, 6), 2, 4)])
def test_class_index_is_a_stable_sort_of_label_case_offset(hwd, ncases, nc):
    cases = hc.index_cases(hwd, ncases, nc)
    index, offsets = ref.class_index(cases, nc)
    rows = [(int(lab), c, v) for c, case in enumerate(cases) for v, lab in enumerate(case["seg"].reshape(-1)) if 0 <= lab < nc]
    rows.sort()                                          # tuples: by label, then case, then offset
    assert [v for _, _, v in rows] == index.tolist() and offsets[-1] == len(rows) and len(offsets) == nc * ncases + 1
    for k in range(nc):
        for c in range(ncases):
            lo, hi = offsets[k * ncases + c], offsets[k * ncases + c + 1]
            assert all(r[0] == k and r[1] == c for r in rows[lo:hi]) and hi - lo == int((cases[c]["seg"] == k).sum())
    if nc > 1 and ncases > 1:
        assert offsets[(nc - 1) * ncases] == offsets[(nc - 1) * ncases + 1]          # class C - 1 is absent from case 0
    if nc > 2:
        assert offsets[ncases] == offsets[2 * ncases]                                # class 1 is absent from every case


def test_class_lists_above_zero_are_the_tumour_index_when_no_label_exceeds_the_range():
    rng = np.random.default_rng(3)
    cases = [{"seg": rng.integers(0, 4, (9, 7, 6)).astype(np.int16)} for _ in range(3)]
    index, offsets = ref.class_index(cases, 4)
    t_index, t_offsets = lx.tumour_index(cases)
    for c in range(3):
        mine = np.sort(np.concatenate([index[offsets[k * 3 + c]:offsets[k * 3 + c + 1]] for k in (1, 2, 3)]))
        assert np.array_equal(mine, t_index[t_offsets[c]:t_offsets[c + 1]])
    assert offsets[-1] - offsets[3] == t_offsets[-1]


def test_key_order_and_the_selection_rule():
    v = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0x7F7FFFFF, 0x3F800000, 0x00000001, 0x00000000, 0x80000000, 0x80000001, 0xBF800000,
                  0xFF7FFFFF, 0xFF800000], np.uint32).view(np.float32)
    k = ref.key(v)
    assert k[0] == k[1] == 0xFFFFFFFF and (np.diff(k[1:].astype(np.int64)) < 0).all()      # NaN, +inf, ..., +0, -0, ..., -inf
    assert ref.key(np.float32(-0.0)) == 0x7FFFFFFF and ref.key(np.float32(0.0)) == 0x80000000
    x = np.array([1.0, 3.0, 3.0, np.nan, 2.0, 3.0, np.nan, -0.0, 0.0], np.float32)
    assert ref.select_largest(x, 1).tolist() == [6]                  # the higher-indexed NaN
    assert ref.select_largest(x, 2).tolist() == [3, 6]
    assert ref.select_largest(x, 4).tolist() == [2, 3, 5, 6]         # of the three 3.0 the two highest-indexed
    assert ref.select_largest(x, 8).tolist() == [0, 1, 2, 3, 4, 5, 6, 8] and ref.select_largest(x, 9).tolist() == list(range(9))
    # without ties it is what NumPy's own sort gives (NaN last)
    y = hc.select_values("distinct", 1000)
    assert np.array_equal(ref.select_largest(y, 300), np.sort(np.argsort(y)[-300:]))


def test_mulhi64_and_the_balanced_draw_lands_in_its_class():
    assert ref.mulhi64(2 ** 64 - 1, 2 ** 64 - 1) == 2 ** 64 - 2 and ref.mulhi64(2 ** 64 - 1, 7) == 6 and ref.mulhi64(2 ** 63, 2) == 1
    hwd, ncases, nc = (9, 7, 6), 3, 4
    cases = hc.sampler_cases(hwd, ncases, 2, seed=5, empty_class=2)
    index, offsets = ref.class_index(cases, nc)
    n, U, Pc = 400, 10, 60
    picks = np.arange(U, dtype=np.uint32)
    cs, x, y, z, kind = ref.hybrid_rows(11, 3, n, U, Pc, nc, picks, index, offsets, ncases, hwd)
    seg = np.stack([c["seg"] for c in cases])
    lab = seg[cs, x, y, z]
    for i in range(U, U + nc * Pc):
        k = (i - U) // Pc
        assert (kind[i] == 1 and lab[i] == k) or (kind[i] == 2 and k == 2), i
    assert (kind[U + 2 * Pc:U + 3 * Pc] == 2).all() and (kind[:U] == 0).all() and (kind[U + nc * Pc:] == 3).all()
    u = lp.draw(11, 3, n, ncases, hwd)
    for got, want in zip((cs, x, y, z), u):
        assert np.array_equal(got[kind >= 2], want[kind >= 2])        # fallback and uniform rows: the plain sampler's
    # class 3 is absent from case 0: no row of class 3 comes from it, and both other cases occur
    rows3 = np.arange(U + 3 * Pc, U + 4 * Pc)
    assert set(cs[rows3]) == {1, 2}
    # the candidates are another stream than the batch's own
    cc = ref.candidates(11, 3, np.arange(50), ncases, hwd)
    assert any(not np.array_equal(a, b[:50]) for a, b in zip(cc, u))


def test_normal3_restatement_moments_and_edges():
    z = ref.normal3(7, 2, 60000).astype(np.float64)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02 and np.abs(np.corrcoef(z.T) - np.eye(3)).max() < 0.02
    full = 0xFFFFFFFF
    e = ref.normal_of_words(([0, full, 0, 0], [0, 0, 1 << 31, full], [full, 0, 5, 5], [0, 0, 0, 0]))
    R0 = np.sqrt(64 * np.log(2.0))
    assert e[0, 0] == R0 and e[0, 1] == 0.0 and e[0, 2] == 0.0                 # r0 = 0: the longest normal; r2 = 2^32 - 1: R' = 0
    assert e[1, 0] == 0.0 and e[1, 1] == 0.0 and e[1, 2] == R0                  # r0 = 2^32 - 1: u1 = 1, R = 0
    assert abs(e[2, 0] + R0) < 1e-12 and abs(e[2, 1]) < 1e-14                   # r1 = 2^31: the angle is pi
    assert np.isfinite(e).all() and np.abs(e).max() <= R0


def test_hybrid_counts_are_the_notebooks_truncations():
    assert inr.hybrid_counts(4000, 0.5, 0.3, 4, True) == ref.hybrid_counts(4000, 0.5, 0.3, 4, True) == (2000, 300, 10000)
    assert inr.hybrid_counts(4000, 0.75, 0.3, 4, True) == (3000, 300, 10000)
    assert inr.hybrid_counts(4000, 0.5, 0.3, 4, False) == (0, 300, 0)
    assert inr.hybrid_counts(256, 0.5, 0.3, 4, True) == (128, 19, 1280)          # int(76.8) // 4
    assert inr.hybrid_counts(1001, 0.3, 0.3, 3, True, max_candidates=2000) == (300, 100, 2000)
    for micro in (1, 7, 255, 4001):
        for ur in (0.0, 0.1, 0.5, 0.75):
            assert inr.hybrid_counts(micro, ur, 0.3, 4, True) == ref.hybrid_counts(micro, ur, 0.3, 4, True)


# ---- ABI surface -----------------------------------------------------------------------------------------------------------------------
def test_header_symbols_and_struct_sizes(lib):
    header = (ROOT / "include" / "mrirt.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in SYMBOLS:
        assert s in _lib.ABI_SYMBOLS and hasattr(lib, s) and re.search(rf"\b{s}\s*\(", code), s
    assert "typedef struct MrirtInrClassIndex" in code and "typedef struct MrirtInrHybrid" in code
    assert header.count("typedef struct MrirtInject") == 2
    assert lib.mrirt_sizeof(22) == C.sizeof(_lib.InrClassIndex) == 24 and lib.mrirt_sizeof(23) == C.sizeof(_lib.InrHybrid) == 32
    assert lib.mrirt_sizeof(21) == 0 and lib.mrirt_sizeof(24) == 0 and lib.mrirt_abi_version() == 4
    assert "inr_hybrid.hip" in _lib.HIP_SOURCES and (_lib.CSRC / "inr_hybrid.h").exists()
    assert [f[0] for f in _lib.InrClassIndex._fields_] == ["index", "offsets", "numClasses", "reserved"]
    assert [f[0] for f in _lib.InrHybrid._fields_] == ["nUncertain", "nPerClass", "picks", "noiseSigma", "reserved"]
    src = (_lib.CSRC / "torch_binding.cpp").read_text()
    assert len(re.findall(r"\bm\.def\(", src)) == 19 and "hybrid" not in src


def test_class_index_scratch_is_the_stated_layout_and_monotone(lib):
    f = lib.mrirt_inr_class_index_scratch_bytes
    for hwd in [(2, 2, 2), (5, 4, 3), (16, 16, 16), (17, 16, 16), (2, 3, 683), (2, 17, 241), (240, 240, 155)]:
        for ncases in (1, 2, 3):
            sizes = [f(C.byref(cache(ncases=ncases, hwd=hwd)), nc) for nc in range(1, 17)]
            assert sizes == [ref.scratch_bytes(ncases, hwd, nc) for nc in range(1, 17)], (hwd, ncases)
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and all(v % 256 == 0 and v > 0 for v in sizes)
    by_voxels = [f(C.byref(cache(hwd=(2, 2, d))), 4) for d in range(2, 3000, 37)]
    assert all(a <= b for a, b in zip(by_voxels, by_voxels[1:]))
    assert f(C.byref(cache()), 0) == 0 and f(C.byref(cache()), 17) == 0 and f(None, 4) == 0
    assert f(C.byref(cache(hwd=(1, 5, 7))), 4) == 0 and f(C.byref(cache(hwd=(65536, 65536, 2))), 4) == 0


def test_class_index_refusals_and_their_order(lib):
    count, index = lib.mrirt_inr_class_count, lib.mrirt_inr_class_index
    c = cache()
    nbytes = lib.mrirt_inr_class_index_scratch_bytes(C.byref(c), 4)
    assert count(None, 4, P, None) == ERR_NULL and count(C.byref(c), 4, None, None) == ERR_NULL
    assert count(None, 0, P, None) == ERR_NULL                                   # NULL before ARG
    for nc in (0, 17, 2 ** 32 - 1):
        assert count(C.byref(c), nc, P, None) == ERR_ARG and index(C.byref(c), nc, P, P, P, nbytes, None) == ERR_ARG
    assert count(C.byref(cache(hwd=(65536, 65536, 2))), 4, P, None) == ERR_ARG    # H W D >= 2^32
    assert count(C.byref(cache(hwd=(1, 5, 7))), 4, P, None) == ERR_DIMS and count(C.byref(cache(ncases=0)), 4, P, None) == ERR_ARG
    assert count(C.byref(cache(seg=None)), 4, P, None) == ERR_NULL
    ok = [C.byref(c), 4, P, P, P, nbytes, None]
    for i in (0, 2, 3, 4):                                   # cache, offsets, index, scratch
        a = list(ok); a[i] = None
        assert index(*a) == ERR_NULL, i
    for i, v in ((5, nbytes - 1), (5, 0), (5, -1), (4, BAD)):
        a = list(ok); a[i] = v
        assert index(*a) == ERR_ARG, (i, v)
    a = list(ok); a[2] = None; a[1] = 0
    assert index(*a) == ERR_NULL
    assert index(C.byref(cache(hwd=(65536, 65536, 2))), 4, P, P, P, 1 << 40, None) == ERR_ARG


def test_select_normal3_and_candidates_refusals(lib):
    sel = lib.mrirt_select_largest
    assert sel(None, 10, 3, P, None) == ERR_NULL and sel(P, 10, 3, None, None) == ERR_NULL and sel(None, 0, 0, P, None) == ERR_NULL
    for n, k in ((0, 0), (0, 1), (10, 0), (10, 11), (10, -1), (-1, 1), (65537, 1), (65537, 65537), (2 ** 40, 5)):
        assert sel(P, n, k, P, None) == ERR_ARG, (n, k)
    nrm = lib.mrirt_inr_normal3
    assert nrm(1, 0, 10, None, None) == ERR_NULL and nrm(1, 0, 0, None, None) == ERR_NULL
    for n in (0, -1, 2 ** 31):
        assert nrm(1, 0, n, P, None) == ERR_ARG
    cand, plain = lib.mrirt_inr_sample_candidates, lib.mrirt_inr_sample_batch
    ok = [C.byref(cache()), 1, 0, 100, P, P, P, None]
    for i in (0, 4, 5, 6):
        a = list(ok); a[i] = None
        assert cand(*a) == ERR_NULL, i
    a = list(ok); a[0] = C.byref(cache(M=0)); a[5] = None
    assert cand(*a[:3], 0, *a[4:]) == ERR_ARG                 # no modalities: feats may be NULL; then n_cand is looked at
    for n in (0, -1, 2 ** 31):
        a = list(ok); a[3] = n
        assert cand(*a) == ERR_ARG == plain(*a)
    for bad_cache in (cache(hwd=(1, 5, 7)), cache(ncases=0), cache(seg=None), cache(M=9)):
        a = list(ok); a[0] = C.byref(bad_cache)
        assert cand(*a) == plain(*a) != 0
    a = list(ok); a[4] = None; a[3] = 0
    assert cand(*a) == ERR_NULL


def hyb(U=0, Pc=0, picks=0x1000, sigma=0.0, reserved=0):
    h = _lib.InrHybrid()
    h.nUncertain, h.nPerClass, h.picks, h.noiseSigma, h.reserved = U, Pc, picks, sigma, reserved
    return h


def test_sample_batch_hybrid_refusals_and_their_order(lib):
    f = lib.mrirt_inr_sample_batch_hybrid
    ci = _lib.InrClassIndex(0x1000, 0x1000, 4, 0)
    ok = [C.byref(cache()), C.byref(ci), C.byref(hyb(7, 3)), P, 1, 0, 100, P, P, P, P, None]
    for i in (0, 1, 2, 3, 7, 8, 9, 10):                      # cache, classes (P > 0), hybrid, fields (field_out given), coords, feats, labels, field_out
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    a = list(ok); a[3] = None; a[10] = None                  # no field at all is fine: the next check is n
    a[6] = 0
    assert f(*a) == ERR_ARG
    for bad in (_lib.InrClassIndex(None, 0x1000, 4, 0), _lib.InrClassIndex(0x1000, None, 4, 0)):
        a = list(ok); a[1] = C.byref(bad)
        assert f(*a) == ERR_NULL
    a = list(ok); a[2] = C.byref(hyb(7, 3, picks=None))
    assert f(*a) == ERR_NULL
    # picks and classes may be NULL when their segment is empty: the call then gets as far as the ARG checks
    a = list(ok); a[1] = None; a[2] = C.byref(hyb(0, 0, picks=None, sigma=-1.0))
    assert f(*a) == ERR_ARG
    a = list(ok); a[0] = C.byref(cache(seg=None))
    assert f(*a) == ERR_NULL
    assert f(C.byref(cache(hwd=(1, 5, 7))), *ok[1:]) == ERR_DIMS and f(C.byref(cache(ncases=0)), *ok[1:]) == ERR_ARG
    bad = [dict(U=-1), dict(Pc=-1), dict(U=101), dict(Pc=101), dict(U=89, Pc=3), dict(U=0, Pc=26), dict(U=2 ** 62, Pc=2 ** 62), dict(sigma=-0.001),
           dict(sigma=NAN), dict(sigma=INF), dict(reserved=1)]
    for kw in bad:
        a = list(ok); a[2] = C.byref(hyb(**{**dict(U=7, Pc=3), **kw}))
        assert f(*a) == ERR_ARG, kw
    for n in (0, -1, 2 ** 31):
        a = list(ok); a[6] = n
        assert f(*a) == ERR_ARG, n
    for nc, res in ((0, 0), (17, 0), (4, 1)):
        a = list(ok); a[1] = C.byref(_lib.InrClassIndex(0x1000, 0x1000, nc, res))
        assert f(*a) == ERR_ARG, (nc, res)
    # NULL before ARG: a NULL labels with every argument wrong
    a = list(ok); a[9] = None; a[6] = 0; a[2] = C.byref(hyb(-1, -1, sigma=NAN, reserved=3))
    assert f(*a) == ERR_NULL


def test_python_names_and_pinned_signatures():
    assert list(inspect.signature(inr.VoxelCache.class_index).parameters) == ["self", "num_classes"]
    assert list(inspect.signature(inr.VoxelCache.sample_candidates).parameters) == ["self", "seed", "batch_index", "n_cand"]
    sig = inspect.signature(inr.VoxelCache.sample_hybrid)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[4:]] == [("n_uncertain", 0), ("picks", None), ("n_per_class", 0), ("num_classes", 4),
                                                                               ("noise_sigma", 0.0), ("with_field", False)]
    assert list(inspect.signature(inr.select_largest).parameters) == ["values", "k"]
    assert list(inspect.signature(inr.normal3).parameters) == ["seed", "batch_index", "n"]
    assert list(inspect.signature(inr.hybrid_counts).parameters) == ["micro", "uncertainty_ratio", "balanced_ratio", "num_classes", "use_uncertainty",
                                                                     "max_candidates"]
    assert list(inspect.signature(inr.train_inject).parameters) == ["config", "cases_or_cache", "params", "log", "save_path"]
    assert list(inspect.signature(inr.VoxelCache.sample_field).parameters) == ["self", "seed", "batch_index", "n", "n_tumour"]
    doc = inr.train_inject.__doc__
    for word in ("UNCERTAINTY_RATIO", "BALANCED_RATIO", "UNCERTAINTY_RATIO_STAGE2", "UNCERTAINTY_MC_SAMPLES", "COORD_NOISE_SIGMA_INIT",
                 "COORD_NOISE_SIGMA_FINAL", "UNIFORM_RATIO", "TUMOR_RATIO"):
        assert word in doc, word
    assert "are not part of it" not in doc


def test_train_inject_refuses_tumor_ratio_beside_the_new_keys_before_a_cache_is_built():
    base = dict(NUM_CLASSES=4, RNG_SEED=1, FOURIER_DIM=16, HIDDEN_DIMS=[16, 16], COORD_INJECTION_LAYERS=[1], MODALITY_INJECTION_LAYERS=[1],
                DROPOUT_RATE=0.3, MICRO_BATCH_SIZE=64, ACCUM_STEPS=1, STAGE1_STEPS=1, STAGE2_STEPS=1, LR_STAGE1=1e-3, LR_STAGE2=1e-4, MIN_LR=1e-5,
                WARMUP_STEPS=0, WEIGHT_DECAY=1e-4, CLIP_NORM=1.0, CLASS_WEIGHTS=[1.0] * 4, DICE_WEIGHT=0.5)

    class Never(list):                                   # building a cache from it would iterate it
        def __iter__(self):
            raise AssertionError("a cache was built")

        def __len__(self):
            raise AssertionError("a cache was built")

    for extra in (dict(UNCERTAINTY_RATIO=0.5, BALANCED_RATIO=0.3), dict(COORD_NOISE_SIGMA_INIT=0.01, COORD_NOISE_SIGMA_FINAL=0.0)):
        with pytest.raises(ValueError, match="TUMOR_RATIO"):
            inr.train_inject(dict(base, TUMOR_RATIO=0.25, **extra), Never())
    for half in (dict(UNCERTAINTY_RATIO=0.5), dict(BALANCED_RATIO=0.3), dict(COORD_NOISE_SIGMA_INIT=0.01), dict(COORD_NOISE_SIGMA_FINAL=0.01),
                 dict(COORD_NOISE_SIGMA_INIT=-1.0, COORD_NOISE_SIGMA_FINAL=0.0)):
        with pytest.raises(ValueError):
            inr.train_inject(dict(base, **half), Never())


# ---- harness ---------------------------------------------------------------------------------------------------------------------------
def build_harness() -> pathlib.Path:
    OUT.mkdir(parents=True, exist_ok=True)
    exe = OUT / "hybrid_harness"
    src = ROOT / "tests" / "native" / "hybrid_harness.hip"
    deps = [src] + list((ROOT / "mri-raytracer_amd" / "csrc").glob("*.h"))
    if exe.exists() and exe.stat().st_mtime >= max(p.stat().st_mtime for p in deps):
        return exe
    obj = OUT / "hybrid_harness.o"
    r = subprocess.run([HIPCC, "--offload-host-only", "-Xarch_host", SAN[0], *SAN[1:], "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-w",
                        "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # a host-only object may still name its translation unit's (absent) device image: give it an empty one
    nm = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if " U __hip_fatbin_" in ln})
    stub = OUT / "hybrid_no_device_images.c"
    stub.write_text("".join(f'const char {s}[16] __attribute__((section(".hip_fatbin"), aligned(4096))) = {{0}};\n' for s in syms))
    r = subprocess.run([HIPCC, *SAN, "-w", str(obj), str(stub), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


@pytest.mark.skipif(shutil.which(HIPCC) is None and not pathlib.Path(HIPCC).exists(), reason="hipcc not found")
def test_index_arithmetic_and_draws_under_asan_and_ubsan(lib):
    exe = build_harness()
    index = [(nc_cases, *hwd, nc) for hwd in hc.HARNESS_INDEX_SHAPES for nc_cases, nc in ((1, 1), (2, 4), (3, 16))] + [(2, 40, 30, 28, 4)]
    select = [(n, k, p) for n in (1, 2, 65, 1023, 1025, 10000) for k in hc.select_ks(n) for p in range(6)] + \
             [(n, k, p) for n in (16385, 65536) for k in (1, n // 3, n) for p in (0, 2, 5)]
    rows = [(2, 5, 4, 3, 4, 300, U, Pc) for U, Pc in hc.ROW_CONFIGS] + [(3, 9, 7, 6, 4, 1000, 100, 200), (1, 2, 2, 2, 16, 257, 1, 16)]
    args = [str(v) for item in index for v in ("c", *item)] + [str(v) for item in select for v in ("s", *item)] + \
           [str(v) for item in rows for v in ("r", *item)] + ["z"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert r.returncode == 0, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("item ")]
    assert len(lines) == len(index) + len(select) + len(rows) + 1 and all(ln[-1] == "0" for ln in lines)
    assert f"hybrid_harness: {len(lines)} items, 0 failed" in r.stdout
    for ln, (ncases, H, W, D, nc) in zip(lines, index):
        # the buffer the harness ran in (ASan-checked, exactly this long) is what the ABI tells callers to allocate
        assert int(ln[10]) == ref.scratch_bytes(ncases, (H, W, D), nc) and int(ln[8]) == (H * W * D + 4095) // 4096
        if min(H, W, D) >= 2:
            assert int(ln[10]) == lib.mrirt_inr_class_index_scratch_bytes(C.byref(cache(ncases=ncases, hwd=(H, W, D))), nc)
        assert int(ln[14]) > 0                               # the binary search ran at list ends
    row_lines = [ln for ln in lines if ln[1] == "r"]
    used = [(int(ln[13]), int(ln[15])) for ln in row_lines]
    assert used[0] == (0, 0) and used[2] == (0, 0)           # P == 0: no class rows
    assert all(a > 0 and b > 0 for a, b in (used[1], used[3], used[4], used[5]))      # class rows from the index, and the fallback of the absent class
