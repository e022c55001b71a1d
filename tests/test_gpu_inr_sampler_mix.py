"""The tumour index and the mixed sampler on the GPU (csrc/inr_lossx.hip) against the NumPy restatements of inr_lossx_ref.py,
under ==: counts and index against np.flatnonzero(seg > 0) per case (an empty case, a full case, a case whose only tumour voxel
is the last one, volumes that are no multiple of the 4096-voxel chunk), the mixed draw for every n / n_tumour of
inr_lossx_cases.py with the empty case in the cache (so the fallback fires), and n_tumour = 0 against mrirt_inr_sample_batch."""
import ctypes as C

import numpy as np
import pytest
import torch

import inr_lossx_cases as cases
import inr_lossx_ref as lx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def inr():
    import mrirt
    assert torch.cuda.is_available()
    return mrirt.inr


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("shape", range(len(cases.MIX_SHAPES)), ids=["x".join(map(str, s)) for s in cases.MIX_SHAPES])
def test_count_and_index_equal_flatnonzero(inr, shape):
    import mrirt
    lib = mrirt._lib.lib()
    cs = cases.mix_cases(shape)
    assert int(np.prod(cases.MIX_SHAPES[shape])) <= 300000 and int(np.prod(cases.MIX_SHAPES[shape])) % 4096 != 0
    want_index, want_offsets = lx.tumour_index(cs)
    cache = inr.VoxelCache(cs)
    counts = torch.full((len(cs) + 1,), -7, dtype=torch.int64, device=DEV)
    assert lib.mrirt_inr_tumour_count(C.byref(cache.desc), C.c_void_p(counts.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert _np(counts).tolist() == np.diff(want_offsets).tolist() + [-7]
    assert _np(counts)[0] == 0 and _np(counts)[1] == np.prod(cases.MIX_SHAPES[shape]) and _np(counts)[2] == 1
    # the index through the C ABI: exactly offsets[-1] entries and one spare, a scratch of exactly the stated size between guards
    total = int(want_offsets[-1])
    index = torch.full((total + 1,), -7, dtype=torch.int32, device=DEV)
    offsets = torch.from_numpy(want_offsets).to(DEV)
    nbytes = int(lib.mrirt_inr_tumour_index_scratch_bytes(C.byref(cache.desc)))
    guard = 4096
    buf = torch.full((guard + nbytes + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = lib.mrirt_inr_tumour_index(C.byref(cache.desc), C.c_void_p(offsets.data_ptr()), C.c_void_p(index.data_ptr()),
                                    C.c_void_p(buf.data_ptr() + guard), nbytes, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((buf[:guard] == 0x5A).all()) and bool((buf[guard + nbytes:] == 0x5A).all())
    got = _np(index)
    assert got[total] == -7
    assert np.array_equal(got[:total].view(np.uint32), want_index)
    # the Python layer builds the same, once
    t = cache.tumour_index()
    assert cache.tumour_index() is t and t.index == cache.tumour_voxels.data_ptr()
    assert np.array_equal(_np(cache.tumour_offsets), want_offsets)
    assert np.array_equal(_np(cache.tumour_voxels)[:total].view(np.uint32), want_index)


@pytest.mark.parametrize("n", cases.MIX_NS)
def test_mixed_sampler_equals_the_restatement(inr, n):
    cs = cases.mix_cases(0)
    cache = inr.VoxelCache(cs)
    index, offsets = lx.tumour_index(cs)
    fallback = indexed = 0
    for batch in (0, 2 ** 32 + 5):
        plain = [_np(x) for x in cache.sample(cases.MIX_SEED, batch, n)]
        for nt in cases.mix_n_tumours(n):
            coords, feats, labels = (_np(x) for x in cache.sample(cases.MIX_SEED, batch, n, n_tumour=nt))
            want = lx.sample_mix(cs, cases.MIX_SEED, batch, n, nt, index, offsets)
            assert np.array_equal(coords, want[0]) and np.array_equal(feats, want[1]) and np.array_equal(labels, want[2]), (batch, nt)
            used = want[3]
            assert (labels[used] > 0).all()              # every label of a non-fallback tumour draw
            assert np.array_equal(coords[nt:], plain[0][nt:]) and np.array_equal(labels[nt:], plain[2][nt:])
            indexed += int(used.sum())
            fallback += int(nt - used.sum())
            if nt == 0:
                assert all(np.array_equal(a, b) for a, b in zip((coords, feats, labels), plain))
    if n >= 255:
        assert fallback > 0 and indexed > 0              # the empty case is in the cache


def test_n_tumour_zero_accepts_a_null_index(inr):
    import mrirt
    lib = mrirt._lib.lib()
    cs = cases.mix_cases(1)
    cache = inr.VoxelCache(cs)
    n = 1000
    want = [_np(x) for x in cache.sample(99, 4, n)]
    coords = torch.empty((n, 3), dtype=torch.float32, device=DEV)
    feats = torch.empty((n, cases.MIX_MODS), dtype=torch.float32, device=DEV)
    labels = torch.empty(n, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())               # noqa: E731
    assert lib.mrirt_inr_sample_batch_mix(C.byref(cache.desc), None, 99, 4, n, 0, p(coords), p(feats), p(labels), None) == 0
    torch.cuda.synchronize()
    assert all(np.array_equal(_np(a), b) for a, b in zip((coords, feats, labels), want))
    assert cache._tumour is None                         # sample(n_tumour=0) never builds the index
    a = [_np(x) for x in cache.sample(99, 4, n, n_tumour=n)]
    b = [_np(x) for x in cache.sample(99, 4, n, n_tumour=n)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[2], want[2])


def test_torch_operators_match_the_ctypes_path(inr):
    import mrirt
    cs = cases.mix_cases(1)
    cache = inr.VoxelCache(cs)
    n, nt = 1000, 400
    signed = lambda v: v - 2 ** 64 if v >= 2 ** 63 else v          # noqa: E731
    want = [_np(x) for x in cache.sample(cases.MIX_SEED, 2 ** 32 + 5, n, n_tumour=nt)]
    cache.tumour_index()
    H, W, D = cases.MIX_SHAPES[1]
    for ops in (torch.ops.mrirt, mrirt.torch_ops.load_native()):
        got = ops.inr_sample_batch_mix(cache.mods_table, cache.seg_table, cache.tumour_voxels, cache.tumour_offsets, cases.MIX_MODS, H, W, D,
                                       signed(cases.MIX_SEED), signed(2 ** 32 + 5), n, nt)
        assert all(np.array_equal(_np(x), y) for x, y in zip(got, want))
        plain = ops.inr_sample_batch_mix(cache.mods_table, cache.seg_table, None, None, cases.MIX_MODS, H, W, D, signed(cases.MIX_SEED), 3, n, 0)
        assert all(np.array_equal(_np(x), _np(y)) for x, y in zip(plain, cache.sample(cases.MIX_SEED, 3, n)))
