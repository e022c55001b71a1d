"""The coordinate-injection INR on the GPU (csrc/inr_inject.hip) against the NumPy restatement of its
definition (tests/inject_ref.py), the reference notebook's recorded logits and prediction (tests/golden/inject.npz) and SciPy's
recorded boundary maps (tests/golden/boundary.npz).

Every output and the scratch are sized exactly as the ABI states and lie between guard blocks; each call runs twice, on buffers
pre-filled with 0x00 and with 0xFF, and must give the same bits both times and leave the guards alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import inject_cases as ic
import inject_ref as ref
from mrirt import _lib, inr

pytestmark = pytest.mark.gpu
GUARD = 4096
DEV = "cuda"


class Arena:
    """Buffers of exactly the asked size between two guard blocks, everything pre-filled with one byte."""

    def __init__(self, fill):
        self.fill, self.blocks = fill, []

    def alloc(self, nbytes, dtype=torch.uint8):
        raw = torch.full((GUARD + nbytes + (-nbytes) % 16 + GUARD,), self.fill, dtype=torch.uint8, device=DEV)
        self.blocks.append((raw, nbytes))
        return raw[GUARD:GUARD + nbytes].view(dtype)

    def check(self):
        for raw, nbytes in self.blocks:
            assert bool((raw[:GUARD] == self.fill).all()) and bool((raw[GUARD + nbytes:] == self.fill).all()), "guard block overwritten"


def guarded(fn):
    """fn(arena) -> tuple of tensors / None; run on 0x00- and 0xFF-filled arenas, same bits, guards intact."""
    outs = []
    for fill in (0x00, 0xFF):
        a = Arena(fill)
        res = fn(a)
        torch.cuda.synchronize()
        a.check()
        outs.append([None if t is None else t.cpu().numpy().copy() for t in res])
    for x, y in zip(*outs):
        assert (x is None and y is None) or x.tobytes() == y.tobytes(), "result depends on what the buffers held before"
    return outs[0]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _up(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(DEV)


def desc_of(F, M, widths, cl, ml):
    d = _lib.InjectDesc()
    d.numLayers, d.fourierDim, d.numMods = len(widths), F, M
    for i, w in enumerate(widths):
        d.width[i] = w
    d.coordLayers, d.modLayers = ref.bits(cl, ml, len(widths))
    return d


def dropout(seed, keep, samples=1, sample0=0, index0=0):
    d = _lib.InjectDropout()
    d.seed, d.keep, d.samples, d.sample0, d.reserved, d.index0 = seed, keep, samples, sample0, 0, index0
    return d


class Net:
    def __init__(self, params, desc):
        w, b = ref.flat(params)
        self.desc, self.B, self.w, self.b = desc, _up(params["fourier"]["B"]), _up(w), _up(b)
        self.C = desc.width[desc.numLayers - 1]

    def scratch(self, arena, n):
        nbytes = _lib.lib().mrirt_inject_scratch_bytes(C.byref(self.desc), n)
        assert nbytes > 0
        return arena.alloc(nbytes), nbytes


def forward(net, coords, mods, drop=None, want_logits=True, want_argmax=True):
    n = coords.shape[0]
    c, m = _up(coords), (_up(mods) if net.desc.numMods else None)

    def run(a):
        logits = a.alloc(4 * n * net.C, torch.float32) if want_logits else None
        am = a.alloc(2 * n, torch.int16) if want_argmax else None
        scratch, nbytes = net.scratch(a, n)
        rc = _lib.lib().mrirt_inject_forward(C.byref(net.desc), _ptr(net.B), _ptr(net.w), _ptr(net.b), _ptr(c), _ptr(m), n,
                                             C.byref(drop) if drop is not None else None, _ptr(logits), _ptr(am), _ptr(scratch), nbytes, None)
        assert rc == 0, rc
        return logits, am
    logits, am = guarded(run)
    return (logits.reshape(n, net.C) if logits is not None else None), am


def uncertainty(net, coords, mods, drop, want_mean=True):
    n = coords.shape[0]
    c, m = _up(coords), (_up(mods) if net.desc.numMods else None)

    def run(a):
        ent = a.alloc(4 * n, torch.float32)
        mean = a.alloc(4 * n * net.C, torch.float32) if want_mean else None
        scratch, nbytes = net.scratch(a, n)
        rc = _lib.lib().mrirt_inject_uncertainty(C.byref(net.desc), _ptr(net.B), _ptr(net.w), _ptr(net.b), _ptr(c), _ptr(m), n, C.byref(drop),
                                                 _ptr(ent), _ptr(mean), _ptr(scratch), nbytes, None)
        assert rc == 0, rc
        return ent, mean
    ent, mean = guarded(run)
    return ent, (mean.reshape(n, net.C) if mean is not None else None)


def volume(net, mods, chunk, drop=None):
    hwd = mods.shape[1:]
    n = hwd[0] * hwd[1] * hwd[2]
    m = _up(mods)

    def run(a):
        pred = a.alloc(2 * n, torch.int16)
        ent = a.alloc(4 * n, torch.float32) if drop is not None else None
        scratch, nbytes = net.scratch(a, chunk)
        rc = _lib.lib().mrirt_inject_predict_volume(C.byref(net.desc), _ptr(net.B), _ptr(net.w), _ptr(net.b), _ptr(m), (C.c_uint32 * 3)(*hwd), chunk,
                                                    C.byref(drop) if drop is not None else None, _ptr(pred), _ptr(ent), _ptr(scratch), nbytes, None)
        assert rc == 0, rc
        return pred, ent
    return guarded(run)


# ---- exact tier ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact(name):
    case = next(c for c in ic.EXACT if c[0] == name)
    params, _, coords, mods = ic.exact_case(case)
    return case, params, coords, mods, Net(params, desc_of(*case[2:7]))


@pytest.mark.parametrize("name", [c[0] for c in ic.EXACT])
def test_exact_tier_bits_equal_the_fp32_restatement(name):
    case, params, coords, mods, net = _exact(name)
    want = ref.forward32(params, coords, mods, case[5], case[6])
    logits, am = forward(net, coords, mods)
    bad = ~((logits.view(np.uint32) == want.view(np.uint32)) | (np.isnan(logits) & np.isnan(want)))
    print(name, "differing logits:", int(bad.sum()), "of", bad.size)
    assert ref.same_bits(logits, want)
    assert np.array_equal(am, ref.argmax(want))
    only_am = forward(net, coords, mods, want_logits=False)[1]
    assert np.array_equal(only_am, am)


@pytest.mark.parametrize("case", ic.INTEGER, ids=[c[0] for c in ic.INTEGER])
def test_integer_tier_sums_are_exact(case):
    params, coords8, mods = ic.integer_case(case)
    z8, _ = ref.forward_int(params, coords8, mods, case[5], case[6])
    net = Net(params, desc_of(*case[2:7]))
    logits, am = forward(net, (coords8 / 8.0).astype(np.float32), mods.astype(np.float32))
    got8 = logits.astype(np.float64) * 8
    assert np.array_equal(got8, np.round(got8)) and np.array_equal(got8.astype(np.int64), z8)
    assert np.array_equal(am, np.argmax(z8, 1).astype(np.int16))


# ---- tolerance tier ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tol(name):
    case = next(c for c in ic.TOLERANCE if c[0] == name)
    params, coords, mods = ic.tolerance_case(case)
    z32, z64 = ref.forward32(params, coords, mods, case[5], case[6]), ref.forward64(params, coords, mods, case[5], case[6])
    return case, params, coords, mods, Net(params, desc_of(*case[2:7])), z32, z64


@pytest.mark.parametrize("name", [c[0] for c in ic.TOLERANCE])
def test_tolerance_tier_against_fp64(name):
    case, params, coords, mods, net, z32, z64 = _tol(name)
    logits, _ = forward(net, coords, mods)
    tau, dev = ic.tau(z32, z64), float(np.abs(logits.astype(np.float64) - z64).max())
    print(name, "max |logit - ref64|", dev, "bound 8 max |ref32 - ref64|", tau)
    assert dev <= tau


@functools.lru_cache(maxsize=None)
def _golden():
    g = ic.load_golden()
    params = inr.inject_load(g)
    hwd = tuple(int(v) for v in g["hwd"])
    cl, ml = [int(v) for v in g["coord_layers"]], [int(v) for v in g["mod_layers"]]
    coords, mods = ref.grid_coords(hwd), ref.volume_mods(g["mods"])
    z32, z64 = ref.forward32(params, coords, mods, cl, ml), ref.forward64(params, coords, mods, cl, ml)
    return g, params, hwd, cl, ml, coords, mods, ic.tau(z32, z64), z64, Net(params, desc_of(128, 4, (64, 64, 64, 4), cl, ml))


def test_notebook_logits_within_the_same_bound():
    g, params, hwd, cl, ml, coords, mods, tau, z64, net = _golden()
    logits, _ = forward(net, coords, mods)
    dev64 = float(np.abs(logits.astype(np.float64) - g["logits64"]).max())
    dev32 = float(np.abs(logits.astype(np.float64) - g["logits32"].astype(np.float64)).max())
    print("max |logit - notebook fp64|", dev64, "max |logit - notebook fp32|", dev32, "bound", tau)
    assert dev64 <= tau and float(np.abs(logits.astype(np.float64) - z64).max()) <= tau


# ---- dropout -------------------------------------------------------------------------------------------------------------------
DROP_NETS = ["n63_F14_M1_L3_coords", "n64_F16_M4_L5_both_first_mods_last", "n65_F18_M8_L8_coords_first_both_last", "n257_F128_M4_notebook"]


@pytest.mark.parametrize("keep", [0.5, 0.25])
@pytest.mark.parametrize("name", DROP_NETS)
def test_dropout_bits_equal_the_restated_masks(name, keep):
    case, params, coords, mods, net = _exact(name)
    seed, s, i0 = 0x1234567887654321, 5, (1 << 32) - 17            # the global index crosses 2^32 inside the call
    want = ref.forward32(params, coords, mods, case[5], case[6], dict(seed=seed, keep=keep, s=s), i0)
    logits, am = forward(net, coords, mods, dropout(seed, keep, 1, s, i0))
    assert ref.same_bits(logits, want) and np.array_equal(am, ref.argmax(want))
    assert not ref.same_bits(logits, ref.forward32(params, coords, mods, case[5], case[6]))       # the mask does something


def test_keep_one_is_the_evaluation_forward_and_seed_and_sample_matter():
    case, params, coords, mods, net = _exact("n257_F128_M4_notebook")
    ev = forward(net, coords, mods)[0]
    assert forward(net, coords, mods, dropout(9, 1.0, 1, 3, 0))[0].tobytes() == ev.tobytes()
    a = forward(net, coords, mods, dropout(9, 0.5, 1, 0, 0))[0]
    b = forward(net, coords, mods, dropout(9, 0.5, 1, 1, 0))[0]
    c = forward(net, coords, mods, dropout(10, 0.5, 1, 0, 0))[0]
    assert forward(net, coords, mods, dropout(9, 0.5, 1, 0, 0))[0].tobytes() == a.tobytes()
    assert a.tobytes() != b.tobytes() and a.tobytes() != c.tobytes() and a.tobytes() != ev.tobytes()


def test_rows_keep_their_bits_when_a_call_is_split():
    case, params, coords, mods, net = _tol("notebook_shape")[:5]
    whole = forward(net, coords, mods, dropout(3, 0.7, 1, 2, 1000))[0]
    parts = [forward(net, coords[a:b], mods[a:b], dropout(3, 0.7, 1, 2, 1000 + a))[0] for a, b in ((0, 1), (1, 64), (64, 129), (129, 257))]
    assert np.concatenate(parts).tobytes() == whole.tobytes()


# ---- uncertainty ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 5, 64])
@pytest.mark.parametrize("name", [c[0] for c in ic.TOLERANCE])
def test_uncertainty_against_fp64_with_the_restated_masks(name, S):
    case, params, coords, mods, net = _tol(name)[:5]
    n = 257 if S < 64 else 65
    coords, mods = coords[:n], mods[:n]
    seed, keep, s0, i0 = 42, 0.7, 3, 77
    e32, m32 = ref.uncertainty32(params, coords, mods, case[5], case[6], seed, keep, S, s0, i0)
    e64, m64 = ref.uncertainty64(params, coords, mods, case[5], case[6], seed, keep, S, s0, i0)
    ent, mean = uncertainty(net, coords, mods, dropout(seed, keep, S, s0, i0))
    te, tm = 8 * float(np.abs(e32 - e64).max()), 8 * float(np.abs(m32 - m64).max())
    de, dm = float(np.abs(ent - e64).max()), float(np.abs(mean - m64).max())
    print(name, S, "entropy dev", de, "bound", te, "mean dev", dm, "bound", tm)
    assert de <= te and dm <= tm
    assert uncertainty(net, coords, mods, dropout(seed, keep, S, s0, i0), want_mean=False)[0].tobytes() == ent.tobytes()


def test_one_sample_without_mask_is_the_entropy_of_the_evaluation_softmax():
    case, params, coords, mods, net, z32, z64 = _tol("notebook_shape")
    ent, mean = uncertainty(net, coords, mods, dropout(1, 1.0, 1, 0, 0))
    e = np.exp(z64 - z64.max(1, keepdims=True))
    p64 = e / e.sum(1, keepdims=True)
    e64 = -(p64 * np.log(p64 + 1e-10)).sum(1)
    e32, p32 = ref.entropy32(ref.softmax32(z32), 1)
    te, tm = 8 * float(np.abs(e32 - e64).max()), 8 * float(np.abs(p32 - p64).max())
    print("entropy dev", float(np.abs(ent - e64).max()), "bound", te)
    assert float(np.abs(ent - e64).max()) <= te and float(np.abs(mean - p64).max()) <= tm
    # and exactly the library's own softmax of the evaluation logits
    logits = forward(net, coords, mods)[0]
    e_gpu, _ = ref.entropy32(ref.softmax32(logits), 1)
    assert float(np.abs(ent - e_gpu).max()) <= te


# ---- volume --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hwd", ic.VOLUMES, ids=["x".join(map(str, v)) for v in ic.VOLUMES])
def test_volume_equals_the_point_entry_points_for_every_chunk(hwd):
    params, mods = ic.volume_case(hwd)
    net = Net(params, desc_of(16, 4, (17, 64, 13, 4), (1, 2), (2,)))
    n = hwd[0] * hwd[1] * hwd[2]
    coords, flat = ref.grid_coords(hwd), ref.volume_mods(mods)
    am = forward(net, coords, flat)[1]
    ent = uncertainty(net, coords, flat, dropout(11, 0.7, 5, 0, 0), want_mean=False)[0]
    plain = volume(net, mods, n)[0]
    assert np.array_equal(plain, am)
    for chunk in (64, 100, n):
        pred, e = volume(net, mods, chunk, dropout(11, 0.7, 5, 0, 0))
        assert np.array_equal(pred, am), chunk
        assert e.tobytes() == ent.tobytes(), chunk


def test_volume_against_the_notebook_pred():
    g, params, hwd, cl, ml, coords, mods, tau, z64, net = _golden()
    top = np.sort(g["logits64"], 1)
    decided = (top[:, -1] - top[:, -2]) > 2 * tau
    left_out = 1.0 - decided.mean()
    print("voxels left out:", left_out, "2 tau", 2 * tau)
    assert left_out <= 0.005
    for chunk in (64, 100, coords.shape[0]):
        pred = volume(net, g["mods"], chunk)[0]
        assert np.array_equal(pred[decided], g["pred"].reshape(-1)[decided]), chunk


# ---- boundary weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vol", ic.load_boundary(), ids=[v[0] for v in ic.load_boundary()])
def test_boundary_weights_equal_scipy(vol):
    name, seg, want = vol
    hwd = (C.c_uint32 * 3)(*seg.shape)
    lab = _up(seg, np.int16)

    def run(a):
        nbytes = _lib.lib().mrirt_boundary_weights_scratch_bytes(hwd)
        out, scratch = a.alloc(4 * seg.size, torch.float32), a.alloc(nbytes)
        rc = _lib.lib().mrirt_boundary_weights(_ptr(lab), hwd, 4, _ptr(out), _ptr(scratch), nbytes, None)
        assert rc == 0, rc
        return (out,)
    got = guarded(run)[0].reshape(seg.shape)
    assert ref.same_bits(got, want)


# ---- Python surface ------------------------------------------------------------------------------------------------------------
def test_python_surface_against_the_abi_calls(tmp_path):
    g, params, hwd, cl, ml, coords, mods, tau, z64, net = _golden()
    path = tmp_path / "model_final.npz"
    np.savez_compressed(path, **{k: v for k, v in g.items() if k == "fourier_B" or k.startswith("mlp_")})
    p = inr.inject_load(path)
    logits, am = forward(net, coords, mods)
    got, got_am = inr.inject_forward(p, coords, mods, want_argmax=True)               # the notebook's own layer lists
    assert got.cpu().numpy().tobytes() == logits.tobytes() and np.array_equal(got_am.cpu().numpy(), am)
    d = inr.inject_forward(p, coords, mods, dropout=inr.inject_dropout(5, 0.5, 1, 2, 9))
    assert d.cpu().numpy().tobytes() == forward(net, coords, mods, dropout(5, 0.5, 1, 2, 9))[0].tobytes()
    case = {"mods": g["mods"], "seg": np.zeros(hwd, np.int16)}
    pred, seg = inr.predict_full_volume(p, case, chunk_size=300)
    assert seg is case["seg"] and pred.dtype == torch.int16 and tuple(pred.shape) == hwd
    assert np.array_equal(pred.cpu().numpy().reshape(-1), am) and np.array_equal(pred.cpu().numpy(), g["pred"])
    keep = float(np.float32(1.0) - np.float32(0.3))
    ent = inr.compute_uncertainty_mc_dropout(p, coords, mods, n_samples=5, seed=7, dropout_rate=0.3)
    want = uncertainty(net, coords, mods, dropout(7, keep, 5, 0, 0), want_mean=False)[0]
    assert ent.cpu().numpy().tobytes() == want.tobytes()
    pred2, _, evol = inr.predict_full_volume(p, case, chunk_size=123, uncertainty=inr.inject_dropout(7, keep, 5))
    assert np.array_equal(pred2.cpu().numpy(), pred.cpu().numpy()) and evol.cpu().numpy().reshape(-1).tobytes() == want.tobytes()
    assert evol.dtype == torch.float32 and tuple(evol.shape) == hwd
    for name, seg_v, w in ic.load_boundary()[:3]:
        assert ref.same_bits(inr.boundary_weights(seg_v).cpu().numpy(), w), name
