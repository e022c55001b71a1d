"""Case preparation on the GPU (csrc/prep.hip).  The contract is equality: the window and the normalised volume
with volume.normalize_intensity on the same data, the Gaussian with SciPy's stored outputs and the NumPy restatement
(tests/prep_ref.py), the z-score with the fp32 formula on the device's own constants — NaN matching NaN, -0.0 == +0.0.  The one
tolerance is the project's bar against the host's fp32 z-score: 8 x the host's own deviation from the fp64 evaluation."""
import ctypes as C
import pathlib

import numpy as np
import pytest

import prep_ref as pr

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "prep_gauss.npz"
f32 = np.float32
GUARD = 1024                                    # bytes either side of a guarded buffer
BLOCK, MAXB = 4096, 512                         # values per histogram block, per-block partials kept (csrc/prep_index.h)


@pytest.fixture(scope="module")
def env():
    import torch
    import mrirt
    from mrirt import _lib, volume
    assert torch.cuda.is_available()
    return dict(torch=torch, mrirt=mrirt, lib=_lib.lib(), _lib=_lib, volume=volume)


def _mri_like(rng, shape):
    return (rng.integers(0, 4096, size=shape) * (rng.random(shape) < 0.6)).astype(np.float32)


def _window_cases():
    rng = np.random.default_rng(19)
    yield "n1", np.array([[[3.5]]], dtype=np.float32)
    yield "n2", np.array([[[3.5, -1.0]]], dtype=np.float32)
    yield "2x3x5", rng.standard_normal((2, 3, 5)).astype(np.float32)
    for n in (BLOCK - 1, BLOCK, BLOCK + 1):                                     # either side of one histogram block
        yield f"z_{n}", rng.standard_normal((1, 1, n)).astype(np.float32)
    yield "x_4097", rng.standard_normal((BLOCK + 1, 1, 1)).astype(np.float32)
    yield "y_4097", rng.standard_normal((1, BLOCK + 1, 1)).astype(np.float32)
    # either side of the per-block partial count: 512 x 4096 = 2 097 152
    yield "partials_minus_1", _mri_like(rng, (7, 1, 299593))
    yield "partials_exact", _mri_like(rng, (128, 128, 128))
    yield "partials_plus_1", _mri_like(rng, (3, 3, 233017))
    yield "fp32_index_131802", _mri_like(rng, (6, 11, 1997)) + rng.random((6, 11, 1997)).astype(np.float32)
    yield "brats_240x240x155", _mri_like(rng, (240, 240, 155))
    yield "constant", np.full((9, 10, 11), 7.25, dtype=np.float32)
    yield "two_valued", np.where(rng.random((33, 34, 35)) < 0.3, 2.0, -1.0).astype(np.float32)
    yield "negatives", (-np.abs(rng.standard_normal((20, 21, 22))) * 100).astype(np.float32)
    yield "denormals", (rng.integers(-50, 50, size=(20, 21, 22)).astype(np.float32) * f32(1e-42)).astype(np.float32)
    yield "denormals_and_normals", np.where(rng.random((20, 21, 22)) < 0.5, f32(3e-41), rng.standard_normal((20, 21, 22))).astype(np.float32)
    yield "signed_zeros", np.where(rng.random((20, 21, 22)) < 0.5, 0.0, -0.0).astype(np.float32)
    yield "zeros_and_values", np.where(rng.random((20, 21, 22)) < 0.5, -0.0, rng.standard_normal((20, 21, 22))).astype(np.float32)
    # all keys share their three leading radix digits: only the last pass tells them apart
    yield "last_digit", (np.uint32(0x42280000) + rng.integers(0, 256, size=(20, 21, 22)).astype(np.uint32)).view(np.float32)
    v = rng.standard_normal((20, 21, 22)).astype(np.float32)
    v[2, 3, 4] = np.nan
    yield "one_nan", v
    v = rng.standard_normal((20, 21, 22)).astype(np.float32)
    v[0, 0, 0], v[1, 1, 1] = np.inf, -np.inf
    yield "infs", v
    v = np.full((5, 6, 7), np.inf, dtype=np.float32)
    v[0, 0, 0] = 1.0
    yield "mostly_inf", v


WINDOW_CASES = list(_window_cases())


@pytest.mark.parametrize("name,vol", WINDOW_CASES, ids=[c[0] for c in WINDOW_CASES])
def test_window_and_normalisation_equal_the_host_function(env, name, vol):
    volume = env["volume"]
    assert vol.dtype == np.float32 and vol.ndim == 3
    with np.errstate(all="ignore"):
        want_lin, want_norm, want_dims = volume.normalize_intensity(vol)
    lin, norm, dims, window = volume.normalize_intensity_device(vol)
    assert lin.is_cuda and norm.is_cuda and window.is_cuda and dims.dtype == np.uint32 and dims.tolist() == want_dims.tolist()
    rec = window.cpu().numpy()
    want_rec = pr.window(vol)
    print(name, "record", rec.tolist(), "restated", want_rec.tolist())
    assert pr.same(rec, want_rec), f"{name}: the window record differs from the restated order statistics"
    got_norm, got_lin = norm.cpu().numpy(), lin.cpu().numpy()
    assert got_norm.shape == vol.shape and got_norm.dtype == np.float32 and got_lin.shape == (vol.size,)
    assert pr.same(got_norm, want_norm), f"{name}: normalised volume differs from volume.normalize_intensity"
    assert pr.same(got_lin, want_lin), f"{name}: linear buffer differs from volume.normalize_intensity"
    assert np.array_equal(got_lin.view(np.uint32), volume.flatten_xyz(got_norm).view(np.uint32))       # both layouts, the same bits
    if name == "constant":
        assert rec[2] == f32(1e-6) and rec[0] == rec[1] == rec[3] == rec[4] == f32(7.25)
    if name == "one_nan":
        assert np.isnan(got_norm).all()
    # a second call gives the same bits; a device tensor is accepted like the array
    lin2, norm2, _, window2 = volume.normalize_intensity_device(env["torch"].from_numpy(vol).cuda())
    assert np.array_equal(window2.cpu().numpy().view(np.uint32), rec.view(np.uint32))
    assert np.array_equal(norm2.cpu().numpy().view(np.uint32), got_norm.view(np.uint32))
    assert np.array_equal(lin2.cpu().numpy().view(np.uint32), got_lin.view(np.uint32))


def test_other_percentiles_equal_numpy(env):
    volume = env["volume"]
    rng = np.random.default_rng(23)
    vol = rng.standard_normal((13, 14, 15)).astype(np.float32)
    for qs in ((0.0, 100.0), (25.0, 75.0), (50.0, 50.0), (33.3, 66.6)):
        rec = volume.prep_window_device(vol, qs).cpu().numpy()
        assert rec[5].tobytes() == np.percentile(vol, qs[0]).tobytes() and rec[6].tobytes() == np.percentile(vol, qs[1]).tobytes(), qs


class _Guarded:
    """A device buffer of `nbytes` with GUARD bytes of 0xA5 either side."""

    def __init__(self, torch, nbytes, fill=None):
        self.nbytes = nbytes
        pad = (nbytes + 255) // 256 * 256
        self.raw = torch.full((GUARD + pad + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.ptr = C.c_void_p(self.raw.data_ptr() + GUARD)
        if fill is not None:
            self.raw[GUARD:GUARD + nbytes] = torch.from_numpy(np.frombuffer(fill.tobytes(), dtype=np.uint8).copy()).cuda()

    def intact(self):
        h = self.raw.cpu().numpy()
        return bool((h[:GUARD] == 0xA5).all() and (h[GUARD + self.nbytes:] == 0xA5).all())

    def array(self, dtype, shape):
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype).reshape(shape).copy()


@pytest.mark.parametrize("shape", [(2, 3, 5), (33, 31, 35), (1, 1, BLOCK + 1)], ids=str)
def test_nothing_is_written_outside_the_scratch_and_the_outputs(env, shape):
    torch, l = env["torch"], env["lib"]
    rng = np.random.default_rng(29)
    vol = _mri_like(rng, shape) + rng.random(shape).astype(np.float32)
    n = vol.size
    need = l.mrirt_prep_scratch_bytes(n)
    src = _Guarded(torch, 4 * n, vol)
    scratch, rec = _Guarded(torch, need), _Guarded(torch, 32)
    norm, lin = _Guarded(torch, 4 * n), _Guarded(torch, 4 * n)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert l.mrirt_prep_window(src.ptr, n, 1.0, 99.5, rec.ptr, scratch.ptr, need, s) == 0
    dims = (C.c_uint32 * 3)(*shape)
    assert l.mrirt_prep_normalize(src.ptr, dims, rec.ptr, norm.ptr, lin.ptr, s) == 0
    torch.cuda.synchronize()
    for g in (src, scratch, rec, norm, lin):
        assert g.intact()
    want_lin, want_norm, _ = env["volume"].normalize_intensity(vol)
    assert pr.same(rec.array(np.float32, (8,)), pr.window(vol))
    assert pr.same(norm.array(np.float32, shape), want_norm) and pr.same(lin.array(np.float32, (n,)), want_lin)
    # either output alone
    only_norm, only_lin = _Guarded(torch, 4 * n), _Guarded(torch, 4 * n)
    assert l.mrirt_prep_normalize(src.ptr, dims, rec.ptr, only_norm.ptr, None, s) == 0
    assert l.mrirt_prep_normalize(src.ptr, dims, rec.ptr, None, only_lin.ptr, s) == 0
    torch.cuda.synchronize()
    assert only_norm.intact() and only_lin.intact()
    assert pr.same(only_norm.array(np.float32, shape), want_norm) and pr.same(only_lin.array(np.float32, (n,)), want_lin)


# --- z-score --------------------------------------------------------------------------------------------------------------
ZBLOCK = 256 * 8                                # values one reduction block takes before it strides (csrc/prep_index.h)


def _zscore_cases():
    rng = np.random.default_rng(31)
    yield "M4_17x19x23", np.stack([_mri_like(rng, (17, 19, 23)) for _ in range(4)])
    yield "M1_17x19x23", _mri_like(rng, (1, 17, 19, 23))
    for n in (ZBLOCK - 1, ZBLOCK, ZBLOCK + 1, 256 * ZBLOCK - 1, 256 * ZBLOCK + 1):      # either side of one block, of all blocks
        yield f"M2_n{n}", np.stack([_mri_like(rng, (1, 1, n)) for _ in range(2)])
    m = np.stack([_mri_like(rng, (5, 6, 7)) for _ in range(4)])
    m[1] = 0                                     # all zeros: left unchanged
    m[2] = 0
    m[2, 1, 2, 3] = 7                            # one non-zero voxel: sigma == 0
    yield "zeros_and_single", m


ZSCORE_CASES = list(_zscore_cases())


@pytest.mark.parametrize("name,mods", ZSCORE_CASES, ids=[c[0] for c in ZSCORE_CASES])
def test_zscore(env, name, mods):
    volume = env["volume"]
    z, stats = volume.zscore_nonzero_device(mods)
    assert z.is_cuda and tuple(z.shape) == mods.shape and tuple(stats.shape) == (4, mods.shape[0])
    got = z.cpu().numpy()
    st = stats.cpu().numpy()
    zmu, zdiv, cnt = volume.zscore_constants(stats)
    for m in range(mods.shape[0]):
        mu, sg, count = pr.zscore_stats(mods[m])
        # integer-valued voxels in 0..4095: every fp64 sum of the first pass is exact
        assert cnt[m] == count and st[0, m] == mu, (name, m)
        assert st[1, m] in (sg, np.nextafter(sg, f32(np.inf)), np.nextafter(sg, f32(-np.inf))), (name, m, st[1, m], sg)
        assert st[2, m] == f32(st[1, m] + f32(1e-6)) == zdiv[m] and zmu[m] == st[0, m]
        assert pr.same(got[m], pr.zscore_apply(mods[m], st[0, m], st[1, m], count)), (name, m)
        if count == 0:
            assert np.array_equal(got[m], mods[m])
        if count == 1:
            assert st[1, m] == 0
        host = volume.zscore_nonzero(mods[m])
        z64 = pr.zscore_f64(mods[m])
        dev_host, dev_gpu = float(np.abs(host - z64).max()), float(np.abs(got[m] - z64).max())
        vs_host = float(np.abs(got[m] - host).max())
        print(f"{name}[{m}]: host fp32 deviation from fp64 {dev_host:.3e}, device's {dev_gpu:.3e}, device vs host {vs_host:.3e}")
        assert vs_host <= 8 * dev_host, (name, m, vs_host, dev_host)
    # two calls, the same bits; in place on a device tensor
    t = env["torch"].from_numpy(mods).cuda()
    z2, stats2 = volume.zscore_nonzero_device(t, out=t)
    assert z2 is t and np.array_equal(stats2.cpu().numpy().view(np.uint32), st.view(np.uint32))
    assert np.array_equal(t.cpu().numpy().view(np.uint32), got.view(np.uint32))


# --- Gaussian -------------------------------------------------------------------------------------------------------------
GAUSS_SHAPES = [(1, 1, 1), (2, 3, 1), (5, 1, 7), (9, 8, 7), (33, 17, 20)]


def _tag(shape):
    return "x".join(str(v) for v in shape)


@pytest.mark.parametrize("sigma", [0.5, 2.3])
@pytest.mark.parametrize("shape", GAUSS_SHAPES, ids=_tag)
def test_gaussian_equals_scipys_stored_output_through_the_raw_abi(env, shape, sigma):
    torch, l = env["torch"], env["lib"]
    g = np.load(GOLDEN)
    a, w, want = g[f"in_{_tag(shape)}"], g[f"w_{sigma}"], g[f"out_{_tag(shape)}_{sigma}"]
    r = (len(w) - 1) // 2
    src, out, scratch = _Guarded(torch, a.nbytes, a), _Guarded(torch, a.nbytes), _Guarded(torch, a.nbytes)
    wc = (C.c_double * len(w))(*w.tolist())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dims = (C.c_uint32 * 3)(*shape)
    assert l.mrirt_prep_gaussian3d(src.ptr, dims, wc, r, out.ptr, scratch.ptr, s) == 0
    torch.cuda.synchronize()
    assert src.intact() and out.intact() and scratch.intact()
    assert np.array_equal(out.array(np.float32, shape), want), (shape, sigma)
    assert np.array_equal(src.array(np.float32, shape), a)
    # in place
    assert l.mrirt_prep_gaussian3d(src.ptr, dims, wc, r, src.ptr, scratch.ptr, s) == 0
    torch.cuda.synchronize()
    assert src.intact() and scratch.intact() and np.array_equal(src.array(np.float32, shape), want)


_GAUSS_REF = {}


def _gauss_ref(shape, sigma):
    key = (shape, sigma)
    if key not in _GAUSS_REF:
        rng = np.random.default_rng(hash(key) % 2**32)
        a = (rng.standard_normal(shape) * 100).astype(np.float32)
        want = pr.gaussian_filter(a, sigma)
        a.setflags(write=False)
        want.setflags(write=False)
        _GAUSS_REF[key] = (a, want)
    return _GAUSS_REF[key]


# sigma 1.0: r = 4; sigma 4.0: r = 16.  Axes shorter than, equal to and longer than r; last extents on both sides of the
# threshold (8) between the two tile shapes; more than one tile along every axis; one 64 x 48 x 40 volume.
@pytest.mark.parametrize("shape,sigma", [((3, 4, 5), 1.0), ((2, 3, 9), 1.0), ((4, 4, 4), 1.0), ((5, 16, 17), 4.0), ((16, 16, 16), 4.0),
                                         ((70, 3, 2), 1.0), ((3, 70, 7), 0.5), ((2, 5, 130), 2.3), ((35, 34, 8), 1.0), ((40, 9, 33), 4.0),
                                         ((64, 48, 40), 0.5), ((64, 48, 40), 2.3)], ids=str)
def test_gaussian_function_equals_the_restatement(env, shape, sigma):
    volume, torch = env["volume"], env["torch"]
    a, want = _gauss_ref(shape, sigma)
    got = volume.gaussian_filter_device(a, sigma)
    assert got.is_cuda and tuple(got.shape) == shape
    assert np.array_equal(got.cpu().numpy(), want), (shape, sigma)
    t = torch.from_numpy(a.copy()).cuda()
    res = volume.gaussian_filter_device(t, sigma, out=t)                # in place
    assert res is t and np.array_equal(t.cpu().numpy().view(np.uint32), got.cpu().numpy().view(np.uint32))


def test_gaussian_radius_zero_is_the_identity(env):
    rng = np.random.default_rng(37)
    a = rng.standard_normal((9, 10, 11)).astype(np.float32)
    a[0, 0, 0], a[1, 1, 1] = -0.0, f32(1e-42)
    got = env["volume"].gaussian_filter_device(a, 0.12).cpu().numpy()
    assert len(env["volume"].gaussian_weights(0.12)) == 1 and np.array_equal(got.view(np.uint32), a.view(np.uint32))
