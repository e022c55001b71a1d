"""Inputs of the hybrid sampler's tests (tests/test_hybrid_host.py, tests/test_gpu_hybrid.py).  No GPU.

The shapes are the smallest at which the kernels can still go wrong: 5 x 4 x 3 (one partial chunk), 17 x 16 x 16 = 4352 voxels (one
voxel row past a 4096 chunk), and one and two chunks plus the least a cache can hold beyond them.  4097 = 17 x 241 and 8193 =
3 x 2731 have no three factors >= 2, and the library refuses a cache with an axis shorter than 2 (MRIRT_ERR_DIMS), so the GPU
runs 2 x 3 x 683 = 4098 and 2 x 17 x 241 = 8194 voxels; the host harness, which walks the same index functions without the
cache check, runs 4097 x 1 x 1 and 8193 x 1 x 1 exactly (HARNESS_INDEX_SHAPES).  Labels -1, C and 32767 are present in every
random volume; with C > 1 case 0 holds no voxel of class C - 1, with C > 2 class 1 is absent from every case.
"""
import numpy as np

INDEX_SHAPES = [(5, 4, 3), (17, 16, 16), (2, 3, 683), (2, 17, 241)]           # 60, 4352, 4098 and 8194 voxels
HARNESS_INDEX_SHAPES = INDEX_SHAPES + [(4097, 1, 1), (8193, 1, 1)]
INDEX_CLASSES = [1, 4, 16]
INDEX_NCASES = [1, 2, 3]

SELECT_N = [1, 2, 63, 64, 65, 1023, 1025, 10000, 16384, 16385, 65536]
SELECT_PATTERNS = ["equal", "distinct", "eight", "low_byte", "high_byte", "specials"]

# (U, P) of the row tests on n = 300 rows, C = 4: nothing, balanced only, picks only, all three kinds, and U + C P == n
ROW_CONFIGS = [(0, 0), (0, 3), (7, 0), (7, 3), (100, 50)]
ROW_N = 300


def select_ks(n):
    return sorted({1, max(1, n // 3), max(1, n - 1), n})


def label_volume(rng, hwd, C, cs):
    """Labels -1 .. C and 32767; class C - 1 absent from case 0 (C > 1); class 1 absent everywhere (C > 2)."""
    lab = rng.integers(-1, C + 2, hwd).astype(np.int16)
    lab[lab == C + 1] = 32767
    flat = lab.reshape(-1)
    flat[:3] = (-1, C, 32767)
    if C > 2:
        lab[lab == 1] = 0
    if C > 1 and cs == 0:
        lab[lab == C - 1] = 0
    return lab


def index_cases(hwd, ncases, C, seed=0):
    rng = np.random.default_rng(seed + 7 * ncases + C)
    return [{"seg": label_volume(rng, hwd, C, c)} for c in range(ncases)]


def select_values(pattern, n, seed=0):
    rng = np.random.default_rng(seed + n)
    if pattern == "equal":
        return np.full(n, 0.25, np.float32)
    if pattern == "distinct":
        return rng.permutation(n).astype(np.float32) * np.float32(0.5) - np.float32(n // 4)
    if pattern == "eight":
        return (rng.integers(0, 8, n) - 3).astype(np.float32)
    if pattern == "low_byte":
        return (np.uint32(0x40490F00) | rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    if pattern == "high_byte":
        return ((rng.integers(0, 0x80, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00345678)).view(np.float32)
    if pattern == "specials":
        sp = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0xBF800000, 0x3F800000,
                       0x007FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800001, 0xC0490FDB, 0x3EAAAAAB], np.uint32)
        return sp[rng.integers(0, len(sp), n)].view(np.float32)
    raise ValueError(pattern)


def sampler_cases(hwd, ncases, M, seed=0, C=4, empty_class=None):
    """Cases whose modality 0 names the case and the voxel (c * 100000 + offset); ``empty_class``: a class no case holds."""
    rng = np.random.default_rng(seed)
    vox = int(np.prod(hwd))
    cases = []
    for c in range(ncases):
        seg = rng.integers(-1, C + 1, hwd).astype(np.int16)
        if empty_class is not None:
            seg[seg == empty_class] = 0
        if ncases > 1 and c == 0:
            seg[seg == C - 1] = 0                                 # case 0 holds no voxel of the last class
        mods = np.zeros((M, *hwd), np.float32)
        if M:
            mods[0] = (c * 100000 + np.arange(vox)).reshape(hwd)
            mods[1:] = rng.normal(0, 1, (M - 1, *hwd))
        cases.append({"mods": mods, "seg": seg})
    return cases
