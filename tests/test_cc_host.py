"""Connected components of label volumes without a GPU: the NumPy restatement (cc_ref.py) against the counts the shapes give
by hand, against scipy.ndimage.label where SciPy imports and against its stored outputs everywhere; compute_multi_metrics on
NumPy inputs against the stored results of the notebook's own function; the argument checks of the C ABI (made before any HIP
call), the scratch formula and the documented names."""
import ctypes as C
import hashlib
import inspect
import json
import pathlib

import numpy as np
import pytest

import cc_cases as cc
import cc_ref as cr
import mrirt
from mrirt import _lib

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
CASES = cc.small_cases()
IDS = [c[0] for c in CASES]
CONNS = (1, 2, 3)


@pytest.fixture(scope="module")
def scipy_golden():
    return np.load(GOLDEN / "cc_scipy.npz")


# --- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[3] is not None], ids=[c[0] for c in CASES if c[3] is not None])
def test_restatement_gives_the_listed_counts(case):
    name, lab, mask, want = case
    got = {conn: cr.label(lab, mask, conn)[1] for conn in want}
    print(name, got)
    assert got == want


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_scipy(case):
    ndimage = pytest.importorskip("scipy.ndimage")
    name, lab, mask, _ = case
    for conn in CONNS:
        want, n = ndimage.label(cr.inside(lab, mask), ndimage.generate_binary_structure(3, conn))
        got, gn = cr.label(lab, mask, conn)
        assert got.dtype == want.dtype == np.int32 and gn == n and np.array_equal(got, want), (name, conn)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_the_stored_scipy_outputs(case, scipy_golden):
    name, lab, mask, _ = case
    for conn in CONNS:
        got, gn = cr.label(lab, mask, conn)
        want = scipy_golden[f"{name}_c{conn}"]
        assert got.dtype == want.dtype == np.int32 and got.shape == want.shape
        assert gn == int(scipy_golden[f"{name}_c{conn}_n"]) and np.array_equal(got, want), (name, conn)
        assert gn == 0 or cr.first_occurrences_increase(got, gn)


def test_large_checkerboard_restated(scipy_golden):
    name, lab, mask = cc.large_cases()[0]
    got, n = cr.label(lab, mask, 1)                       # no two voxels of a parity class share a face: no pair to unite
    assert n == cc.LARGE_CHECKER_ROOTS == int(scipy_golden[f"{name}_c1_n"]) and n > 1024 * 1024
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(scipy_golden[f"{name}_c1_sha256"])
    assert int(scipy_golden[f"{name}_c3_n"]) == 1


def test_large_ball_counts_are_stored(scipy_golden):
    name = cc.large_cases()[1][0]
    n6, n26 = int(scipy_golden[f"{name}_c1_n"]), int(scipy_golden[f"{name}_c3_n"])
    print(name, n6, n26)
    assert 1000 < n26 < n6 < int(np.prod(cc.BALL_SHAPE)) // 50
    assert (GOLDEN / "cc_scipy.npz").stat().st_size < 512 * 1024


def test_cases_cover_what_they_should():
    assert {-1, 32, 1000} <= set(cc.by_name("random_0.31_mask_0x3e")[1].ravel().tolist())
    lab = cc.by_name("random_0.31_mask_0xffffffff")[1]
    assert np.array_equal(cr.inside(lab, 0xFFFFFFFF), (lab >= 0) & (lab < 32))          # -1, 32 and 1000 are outside under every mask
    t0, t1, t2 = cc.TILE
    shapes = {c[1].shape for c in CASES if c[0].startswith("tile_")}
    for k, t in enumerate(cc.TILE):
        assert {t - 1, t, t + 1, 2 * t + 1} <= {s[k] for s in shapes}
    big = cc.by_name("tile_%dx%dx%d" % (2 * t0 + 1, 2 * t1 + 1, 2 * t2 + 1))
    n = [cr.label(big[1], big[2], c)[1] for c in CONNS]
    assert n[0] > n[1] > n[2] >= 1                      # pairs that touch only across an edge, only across a corner
    s = cc.by_name("serpentine")[1]
    assert s.shape == cc.SERPENTINE_SHAPE and int(s.sum()) > 17 * 9 * 70


def test_sizes_filter_and_keep_largest():
    lab = np.array([1, 1, 0, 2, 2, 0, 1, 0, 3, 3], np.int16).reshape(1, 1, 10)
    comp, n = cr.label(lab, 0b1110, 1)
    sz = cr.sizes(comp, n)
    assert n == 4 and sz.dtype == np.int32 and sz.tolist() == [2, 2, 1, 2]
    assert np.array_equal(cr.filter_small(lab, comp, sz, 0), lab)
    assert cr.filter_small(lab, comp, sz, 2).ravel().tolist() == [1, 1, 0, 2, 2, 0, 0, 0, 3, 3]
    assert cr.filter_small(lab, comp, sz, 3, fill=-7).ravel().tolist() == [-7, -7, 0, -7, -7, 0, -7, 0, -7, -7]
    assert cr.filter_small(lab, comp, sz, 0, keep_largest=True, fill=9).ravel().tolist() == [1, 1, 0, 9, 9, 0, 9, 0, 9, 9]   # the tie goes to number 1
    assert cr.filter_small(lab, comp, sz, 3, keep_largest=True).ravel().tolist() == [0] * 10
    empty = np.zeros((2, 2, 2), np.int16)
    comp, n = cr.label(empty, 0b10, 1)
    assert n == 0 and np.array_equal(cr.filter_small(empty, comp, cr.sizes(comp, n), 0, keep_largest=True), empty)


def test_slice_counts_restated():
    p = np.zeros((2, 2, 4), np.int16)
    p[:, :, 1] = [[1, 2], [0, -3]]
    p[:, :, 2] = [[1, 3], [4, -3]]
    assert cr.slice_counts(p).tolist() == [[0, 0, 0], [2, 0, 2], [3, 1, 3], [0, 0, 3]]


# --- compute_multi_metrics on the host ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", cc.metric_pairs(), ids=[p[0] for p in cc.metric_pairs()])
def test_compute_multi_metrics_on_numpy_equals_the_notebook(pair):
    name, pred, truth = pair
    want = json.loads((GOLDEN / "cc_metrics.json").read_text())[name]
    got = mrirt.inr.compute_multi_metrics(pred, truth)
    print(name, got)
    assert list(got) == [f"dice_class_{c}" for c in range(4)] + [f"n_components_class_{c}" for c in (1, 2, 3)] + ["slice_consistency"]
    assert got == want
    for c in (1, 2, 3):
        assert got[f"n_components_class_{c}"] == cr.label(pred, 1 << c, 1)[1]
        assert mrirt.components.count_components_host(pred == c, 3) == cr.label(pred, 1 << c, 3)[1]


def test_metric_pairs_cover_what_they_should():
    pairs = {p[0]: p for p in cc.metric_pairs()}
    _, p, t = pairs["absent_class"]
    assert not (p == 2).any() and not (t == 2).any() and (p == 1).any()
    assert not pairs["all_background"][1].any() and not pairs["all_background"][2].any()
    s = pairs["identical_slices"][1]
    assert np.array_equal(s[:, :, 2], s[:, :, 3]) and not s[:, :, 7].any() and s[:, :, 6].any() and s[:, :, 8].any()


# --- the names -----------------------------------------------------------------------------------------------------------------
def test_python_names_have_the_documented_signatures():
    sig = inspect.signature(mrirt.components.label_components)
    assert list(sig.parameters) == ["labels", "classes", "connectivity", "stream"]
    assert [sig.parameters[k].default for k in ("classes", "connectivity", "stream")] == [None, 1, None]
    sig = inspect.signature(mrirt.components.component_sizes)
    assert list(sig.parameters) == ["components", "n"]
    sig = inspect.signature(mrirt.components.remove_small_components)
    assert list(sig.parameters) == ["labels", "classes", "min_voxels", "connectivity", "keep_largest", "fill"]
    assert [p.default for p in sig.parameters.values()][1:] == [None, 0, 1, False, 0]
    assert list(inspect.signature(mrirt.components.slice_counts).parameters) == ["labels"]
    sig = inspect.signature(mrirt.inr.compute_multi_metrics)
    assert list(sig.parameters) == ["pred", "true", "num_classes"] and sig.parameters["num_classes"].default == 4
    for name in ("label_components", "component_sizes", "remove_small_components", "slice_counts"):
        assert getattr(mrirt, name) is getattr(mrirt.components, name)
    assert mrirt.compute_multi_metrics is mrirt.inr.compute_multi_metrics
    assert mrirt.components._mask(None) == 0xFFFFFFFE and mrirt.components._mask((1, 2, 3)) == 0b1110
    for bad in (0, 4, -1):
        with pytest.raises(ValueError):
            mrirt.components._connectivity(bad)


def test_symbols_are_declared_listed_and_exported():
    header = (_lib.INCLUDE / "mrirt.h").read_text()
    for s in ("mrirt_cc_scratch_bytes", "mrirt_cc_label", "mrirt_cc_sizes", "mrirt_cc_filter", "mrirt_slice_counts"):
        assert s + "(" in header and s in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), s), s
    assert "components.hip" in _lib.HIP_SOURCES and (_lib.CSRC / "cc_index.h").exists()
    assert _lib.lib().mrirt_abi_version() == 4


# --- the C ABI without a device -----------------------------------------------------------------------------------------------
def _hwd(*v):
    return (C.c_uint32 * 3)(*v)


NULL, DIMS, ARG = -1, -2, -5
TOO_LARGE = ((1 << 31, 1, 1), (1, 1 << 31, 1), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (1 << 16, 1 << 15, 1), (1291, 1291, 1291),
             (2048, 1024, 1024))
LARGEST = ((0x7FFFFFFF, 1, 1), (1, 1, 0x7FFFFFFF), (1290, 1290, 1290), (2047, 1024, 1024))


def test_abi_rejects_malformed_arguments_before_any_hip_call():
    """Host memory stands in for the device buffers: every call below must return before anything is launched or read."""
    l = _lib.lib()
    buf = C.create_string_buffer(8192)
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)
    ok = _hwd(4, 4, 4)
    big = 1 << 40

    def label(lab=p, hwd=ok, conn=1, comp=p, count=p, scratch=p, nbytes=big):
        return l.mrirt_cc_label(lab, hwd, 2, conn, comp, count, scratch, nbytes, None)

    def sizes(comp=p, hwd=ok, n=1, out=p):
        return l.mrirt_cc_sizes(comp, hwd, n, out, None)

    def filt(lab=p, comp=p, sz=p, n=1, hwd=ok, min_voxels=0, keep=0, out=p):
        return l.mrirt_cc_filter(lab, comp, sz, n, hwd, min_voxels, keep, 0, out, None)

    def counts(lab=p, hwd=ok, out=p):
        return l.mrirt_slice_counts(lab, hwd, out, None)

    for kw in ("lab", "hwd", "comp", "count", "scratch"):
        assert label(**{kw: None}) == NULL, kw
    for kw in ("comp", "hwd", "out"):
        assert sizes(**{kw: None}) == NULL, kw
    for kw in ("lab", "comp", "sz", "hwd", "out"):
        assert filt(**{kw: None}) == NULL, kw
    for kw in ("lab", "hwd", "out"):
        assert counts(**{kw: None}) == NULL, kw
    for bad in (_hwd(0, 4, 4), _hwd(4, 0, 4), _hwd(4, 4, 0)):
        assert label(hwd=bad) == DIMS and sizes(hwd=bad) == DIMS and filt(hwd=bad) == DIMS and counts(hwd=bad) == DIMS, list(bad)
        assert l.mrirt_cc_scratch_bytes(bad) == 0
    for shape in TOO_LARGE:                                   # n0 n1 n2 must stay below 2^31
        bad = _hwd(*shape)
        assert label(hwd=bad) == ARG and sizes(hwd=bad) == ARG and filt(hwd=bad) == ARG and counts(hwd=bad) == ARG, shape
        assert l.mrirt_cc_scratch_bytes(bad) == 0
    for shape in LARGEST:
        assert l.mrirt_cc_scratch_bytes(_hwd(*shape)) > 0, shape
    for conn in (0, 4, 26, 0xFFFFFFFF):
        assert label(conn=conn) == ARG, conn
    need = l.mrirt_cc_scratch_bytes(ok)
    assert need > 0
    assert label(nbytes=need - 1) == ARG and label(nbytes=0) == ARG and label(nbytes=-1) == ARG
    assert label(scratch=C.c_void_p(p.value + 4)) == ARG                    # the scratch must be 16-byte aligned
    assert sizes(n=-1) == ARG and sizes(n=65) == ARG                        # more components than voxels
    assert filt(n=-1) == ARG and filt(n=65) == ARG and filt(min_voxels=-1) == ARG
    assert filt(keep=2) == ARG and filt(keep=-1) == ARG
    assert l.mrirt_cc_scratch_bytes(None) == 0
    assert sizes(n=0, out=None) == 0                                        # nothing to count: nothing is launched


def _scratch_formula(shape, chunk=1024):
    """4 B per chunk of 1024 voxels, and per chunk of those until one chunk holds a level; every part rounded up to 256 B."""
    def al(x):
        return (x + 255) // 256 * 256
    n = -(-(shape[0] * shape[1] * shape[2]) // chunk)
    total = al(4 * n)
    while n > chunk:
        n = -(-n // chunk)
        total += al(4 * n)
    return total


def test_scratch_bytes_formula():
    l = _lib.lib()
    shapes = [(1, 1, 1), (1, 7, 1), (5, 1, 1), (9, 10, 11), (33, 17, 70), (128, 128, 130), (240, 240, 155), (1024, 1024, 1024),
              (1290, 1290, 1290), (0x7FFFFFFF, 1, 1)]
    got = [l.mrirt_cc_scratch_bytes(_hwd(*s)) for s in shapes]
    for s, v in zip(shapes, got):
        assert v == _scratch_formula(s), s
    assert got[0] == 256 and got[6] == _scratch_formula((240, 240, 155)) == 35072 + 256
    assert all(a <= b for a, b in zip(got, got[1:]))
    assert got[6] * 1000 < 4 * 240 * 240 * 155                               # the output volume is the parent array: the scratch stays small
