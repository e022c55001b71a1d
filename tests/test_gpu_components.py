"""Connected components of label volumes on the GPU (csrc/components.hip).  The contract is equality with the NumPy
restatement of the definition (tests/cc_ref.py, pinned by SciPy's stored outputs and the literals of cc_cases.py): component
numbers, counts, sizes, filtered volumes and slice counts, every comparison ``array_equal``, never a tolerance."""
import ctypes as C
import hashlib
import json
import pathlib

import numpy as np
import pytest

import cc_cases as cc
import cc_ref as cr

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
CASES = cc.small_cases()
IDS = [c[0] for c in CASES]
GUARD = 4096
_REF = {}


def _ref(case, conn):
    """The restatement's (components, N, sizes) of a case, computed once per session and never modified."""
    key = (case[0], conn)
    if key not in _REF:
        comp, n = cr.label(case[1], case[2], conn)
        sz = cr.sizes(comp, n)
        comp.setflags(write=False)
        sz.setflags(write=False)
        _REF[key] = (comp, n, sz)
    return _REF[key]


@pytest.fixture(scope="module")
def env():
    import torch
    import mrirt
    assert torch.cuda.is_available()
    return dict(torch=torch, mrirt=mrirt, lib=mrirt._lib.lib())


class Guarded:
    """`nbytes` of device memory between two guard blocks that must come back untouched."""

    def __init__(self, torch, nbytes):
        self.torch, self.nbytes = torch, nbytes
        self.buf = torch.full((GUARD + nbytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        self.ptr = C.c_void_p(self.buf.data_ptr() + GUARD)

    def check(self, what):
        assert bool((self.buf[:GUARD] == 0x5A).all()) and bool((self.buf[GUARD + self.nbytes:] == 0x5A).all()), f"{what}: guard overwritten"

    def array(self, dtype, shape):
        return self.buf[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype).reshape(shape)


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _abi_label(env, lab_dev, shape, mask, conn):
    """mrirt_cc_label with every buffer exactly its size between guards: (components, N), as NumPy / int."""
    torch, lib = env["torch"], env["lib"]
    hwd = (C.c_uint32 * 3)(*shape)
    nbytes = int(lib.mrirt_cc_scratch_bytes(hwd))
    total = int(np.prod(shape))
    comp, count, scratch = Guarded(torch, 4 * total), Guarded(torch, 8), Guarded(torch, nbytes)
    rc = lib.mrirt_cc_label(C.c_void_p(lab_dev.data_ptr()), hwd, mask, conn, comp.ptr, count.ptr, scratch.ptr, nbytes, _stream(torch))
    assert rc == 0
    torch.cuda.synchronize()
    for g, what in ((comp, "components"), (count, "count"), (scratch, "scratch")):
        g.check(what)
    return comp, int(count.array(np.int64, (1,))[0])


@pytest.mark.parametrize("conn", (1, 2, 3))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_stage_equals_the_restatement(env, case, conn):
    torch, lib = env["torch"], env["lib"]
    name, lab, mask, listed = case
    want, wn, wsz = _ref(case, conn)
    if listed is not None and conn in listed:
        assert wn == listed[conn]
    dev = torch.from_numpy(lab).cuda()
    hwd = (C.c_uint32 * 3)(*lab.shape)
    comp, n = _abi_label(env, dev, lab.shape, mask, conn)
    got = comp.array(np.int32, lab.shape)
    print(name, conn, "N", n, "want", wn)
    assert n == wn and np.array_equal(got, want), f"{name}/{conn}: components differ from the restatement"
    comp2, n2 = _abi_label(env, dev, lab.shape, mask, conn)
    assert n2 == n and np.array_equal(comp2.array(np.int32, lab.shape), got), f"{name}/{conn}: a second call gives other bits"

    # sizes
    sizes = Guarded(torch, 4 * n)
    assert lib.mrirt_cc_sizes(comp.ptr, hwd, n, sizes.ptr if n else None, _stream(torch)) == 0
    torch.cuda.synchronize()
    sizes.check("sizes")
    assert np.array_equal(sizes.array(np.int32, (n,)), wsz), f"{name}/{conn}: sizes differ"

    # the filter, out of place and in place
    largest = int(wsz.max()) if n else 0
    for min_voxels, keep, fill in ((0, 0, 0), (2, 0, -5), (largest, 0, 0), (largest + 1, 0, 9), (0, 1, 0), (2, 1, 77)):
        want_f = cr.filter_small(lab, want, wsz, min_voxels, bool(keep), fill)
        out = Guarded(torch, 2 * lab.size)
        assert lib.mrirt_cc_filter(C.c_void_p(dev.data_ptr()), comp.ptr, sizes.ptr if n else None, n, hwd, min_voxels, keep, fill, out.ptr,
                                   _stream(torch)) == 0
        torch.cuda.synchronize()
        out.check("filtered")
        assert np.array_equal(out.array(np.int16, lab.shape), want_f), f"{name}/{conn}: filter({min_voxels}, {keep}, {fill}) differs"
    inplace = dev.clone()
    assert lib.mrirt_cc_filter(C.c_void_p(inplace.data_ptr()), comp.ptr, sizes.ptr if n else None, n, hwd, 2, 0, -5,
                               C.c_void_p(inplace.data_ptr()), _stream(torch)) == 0
    assert np.array_equal(inplace.cpu().numpy(), cr.filter_small(lab, want, wsz, 2, False, -5)), f"{name}/{conn}: in-place filter differs"

    # slice counts (they do not depend on the connectivity: once per case)
    if conn == 1:
        counts = Guarded(torch, 24 * lab.shape[2])
        for _ in range(2):
            assert lib.mrirt_slice_counts(C.c_void_p(dev.data_ptr()), hwd, counts.ptr, _stream(torch)) == 0
            torch.cuda.synchronize()
            counts.check("slice counts")
            assert np.array_equal(counts.array(np.int64, (lab.shape[2], 3)), cr.slice_counts(lab)), f"{name}: slice counts differ"


def test_keep_largest_with_a_tie_keeps_the_lowest_number(env):
    torch, mrirt = env["torch"], env["mrirt"]
    lab = np.array([1, 1, 0, 2, 2, 0, 1, 0, 3, 3], np.int16).reshape(1, 1, 10)
    out = mrirt.remove_small_components(lab, (1, 2, 3), keep_largest=True, fill=9)
    assert out.dtype == torch.int16 and out.is_cuda and out.cpu().numpy().ravel().tolist() == [1, 1, 0, 9, 9, 0, 9, 0, 9, 9]
    comp, n = mrirt.label_components(lab)                  # classes=None: labels > 0
    assert n == 4 and comp.dtype == torch.int32 and comp.cpu().numpy().ravel().tolist() == [1, 1, 0, 2, 2, 0, 3, 0, 4, 4]
    sizes = mrirt.component_sizes(comp, n)
    assert sizes.dtype == torch.int32 and sizes.is_cuda and sizes.tolist() == [2, 2, 1, 2]
    assert mrirt.component_sizes(comp, 0).shape == (0,)


def test_python_entry_points_take_any_integer_dtype(env):
    torch, mrirt = env["torch"], env["mrirt"]
    case = cc.by_name("random_0.31_mask_0x2a")
    name, lab, mask, _ = case
    classes = [b for b in range(32) if (mask >> b) & 1]
    for conn in (1, 3):
        want, wn, _ = _ref(case, conn)
        for how, vol in (("numpy int16", lab), ("device int64", torch.from_numpy(lab).cuda().to(torch.int64)), ("numpy int32", lab.astype(np.int32))):
            comp, n = mrirt.label_components(vol, classes, conn)
            assert n == wn and np.array_equal(comp.cpu().numpy(), want), (how, conn)
    wide = np.zeros((4, 5, 6), np.int32)
    wide[1, 2, 3] = 65536 + 1                              # int16 would read it as class 1
    assert mrirt.label_components(wide, 1)[1] == 0
    sc = mrirt.slice_counts(torch.from_numpy(lab).cuda())
    assert sc.dtype == torch.int64 and tuple(sc.shape) == (lab.shape[2], 3) and np.array_equal(sc.cpu().numpy(), cr.slice_counts(lab))


@pytest.mark.parametrize("conn", (1, 3))
@pytest.mark.parametrize("which", (0, 1), ids=[c[0] for c in cc.large_cases()])
def test_larger_cases_by_properties_and_stored_scipy_hashes(env, which, conn):
    torch = env["torch"]
    name, lab, mask = cc.large_cases()[which]
    golden = np.load(GOLDEN / "cc_scipy.npz")
    dev = torch.from_numpy(lab).cuda()
    comp, n = _abi_label(env, dev, lab.shape, mask, conn)
    got = comp.array(np.int32, lab.shape)
    inside = cr.inside(lab, mask)
    print(name, conn, "N", n, "stored", int(golden[f"{name}_c{conn}_n"]))
    assert np.array_equal(got > 0, inside), "components > 0 exactly on the mask"
    for d in cr.forward_offsets(conn):                     # every adjacent inside pair carries equal numbers
        lo = tuple(slice(max(0, -x), lab.shape[k] - max(0, x)) for k, x in enumerate(d))
        hi = tuple(slice(max(0, x), lab.shape[k] - max(0, -x)) for k, x in enumerate(d))
        both = inside[lo] & inside[hi]
        assert np.array_equal(got[lo][both], got[hi][both]), d
    assert cr.first_occurrences_increase(got, n), "the numbers are 1 .. N with increasing first occurrence"
    assert n == int(golden[f"{name}_c{conn}_n"])
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(golden[f"{name}_c{conn}_sha256"])
    if which == 0 and conn == 1:
        assert n == cc.LARGE_CHECKER_ROOTS > 1024 * 1024   # the scan of the chunk sums recursed


@pytest.mark.parametrize("pair", cc.metric_pairs(), ids=[p[0] for p in cc.metric_pairs()])
def test_compute_multi_metrics_on_device_tensors_equals_the_notebook(env, pair):
    torch, mrirt = env["torch"], env["mrirt"]
    name, pred, truth = pair
    want = json.loads((GOLDEN / "cc_metrics.json").read_text())[name]
    got = mrirt.compute_multi_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(truth).cuda())
    print(name, got)
    assert got == want and list(got) == list(mrirt.compute_multi_metrics(pred, truth))


def test_remove_small_components_on_a_device_prediction(env):
    torch, mrirt = env["torch"], env["mrirt"]
    lab = cc.by_name("random_0.31_mask_0x3e")[1]
    dev = torch.from_numpy(lab).cuda()
    for classes, mask, min_voxels, conn, keep, fill in ((None, 0xFFFFFFFE, 4, 1, False, 0), ((1, 3), 0b1010, 2, 3, False, -1),
                                                        (2, 0b100, 0, 2, True, 5), (None, 0xFFFFFFFE, 10 ** 6, 1, False, 0)):
        out = mrirt.remove_small_components(dev, classes, min_voxels, conn, keep, fill)
        assert out.is_cuda and out.dtype == torch.int16 and out.data_ptr() != dev.data_ptr()
        assert np.array_equal(out.cpu().numpy(), cr.remove_small(lab, mask, min_voxels, conn, keep, fill)), (classes, min_voxels, conn, keep)
    assert torch.equal(dev, torch.from_numpy(lab).cuda())                    # the input is left as it was
