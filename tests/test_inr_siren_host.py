"""The SIREN training entry points' argument checks, on the CPU: every refusal returns its code before anything is launched (no
GPU is present; the pointers handed over are never dereferenced), the scratch size is monotone in n and at least the ReLU
step's, siren_init keeps its bounds and train_siren refuses bad arguments before any work."""
import ctypes as C

import numpy as np
import pytest

from mrirt import _lib

ERR_NULL, ERR_ARG = -1, -5
P = C.c_void_p(0x1000)            # a non-NULL, 16-byte aligned "device pointer" that is never read
BAD = C.c_void_p(0x1004)          # misaligned
NS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 16384, 16385, 65536, 10 ** 6, 2 ** 31 - 1)


def desc(kind=3, layers=3, ind=7, out=4, hidden=64, K=0, M=0, w0=30.0):
    d = _lib.InrDesc()
    d.kind, d.numLayers, d.inDim, d.outDim, d.hidden, d.fourierFreqs, d.numMods, d.w0 = kind, layers, ind, out, hidden, K, M, w0
    return d


def bad_descs():
    """Every descriptor the SIREN entry points refuse: ReLU kinds, Fourier features, w0 of 0 / NaN / inf, bad shapes."""
    return [desc(kind=0, ind=7, M=4), desc(kind=0, ind=31, K=4, M=4), desc(kind=2), desc(kind=4), desc(K=1), desc(kind=1, ind=13, K=1, M=4),
            desc(w0=0.0), desc(w0=-0.0), desc(w0=float("nan")), desc(w0=float("inf")), desc(w0=float("-inf")),
            desc(hidden=48), desc(out=17), desc(out=0), desc(layers=1), desc(layers=9), desc(ind=0), desc(ind=129),
            desc(kind=1, ind=8, M=4), desc(kind=1, ind=12, M=9)]


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_scratch_bytes(lib):
    for d, relu in ((desc(), desc(kind=2)), (desc(kind=1, M=4), desc(kind=0, M=4)), (desc(ind=128, hidden=256, layers=8, out=16), desc(kind=2, ind=128, hidden=256, layers=8, out=16))):
        prev = 0
        for n in NS:
            b = lib.mrirt_siren_train_scratch_bytes(C.byref(d), n)
            assert b >= prev > -1 and b > 0 and b % 256 == 0, n
            r = lib.mrirt_inr_train_scratch_bytes(C.byref(relu), n)
            assert r > 0 and b >= r + (d.numLayers - 1) * n * d.hidden * 4, n          # the ReLU step's, and the cosines behind it
            prev = b
        for n in (0, -1, 2 ** 31):
            assert lib.mrirt_siren_train_scratch_bytes(C.byref(d), n) == 0
    for d in bad_descs():
        assert lib.mrirt_siren_train_scratch_bytes(C.byref(d), 100) == 0
    assert lib.mrirt_siren_train_scratch_bytes(None, 100) == 0
    assert lib.mrirt_siren_train_scratch_bytes(C.byref(desc(w0=-1.5)), 100) > 0          # any finite non-zero w0
    for kind in (1, 3):                                   # the existing entry points go on refusing the SIREN kinds
        assert lib.mrirt_inr_train_scratch_bytes(C.byref(desc(kind=kind, ind=7, M=4)), 100) == 0


def test_forward_refusals(lib):
    d, n = desc(), 100
    nb = lib.mrirt_siren_train_scratch_bytes(C.byref(d), n)
    ok = [C.byref(d), P, P, None, P, n, P, P, nb, None]
    f = lib.mrirt_siren_forward_f32
    for i in (0, 1, 2, 4, 6, 7):                          # desc, w, b, feats (raw kind), logits, scratch
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for n_bad in (0, -1, 2 ** 31):
        a = list(ok); a[5] = n_bad
        assert f(*a) == ERR_ARG
    for short in (nb - 1, lib.mrirt_inr_train_scratch_bytes(C.byref(desc(kind=2)), n), 0, -1):          # the ReLU step's size is too short
        a = list(ok); a[8] = short
        assert f(*a) == ERR_ARG
    a = list(ok); a[7] = BAD
    assert f(*a) == ERR_ARG
    for bd in bad_descs():
        a = list(ok); a[0] = C.byref(bd); a[3] = P
        assert f(*a) == ERR_ARG
    sd = desc(kind=1, M=4)
    nbs = lib.mrirt_siren_train_scratch_bytes(C.byref(sd), n)
    assert f(C.byref(sd), P, P, None, P, n, P, P, nbs, None) == ERR_NULL          # the coords kind needs coords
    assert f(C.byref(sd), P, P, P, None, n, P, P, nbs, None) == ERR_NULL          # ... and its intensities


def test_backward_refusals(lib):
    d, n = desc(), 100
    nb = lib.mrirt_siren_train_scratch_bytes(C.byref(d), n)
    f = lib.mrirt_siren_backward
    ok = [C.byref(d), P, n, P, P, P, 0, P, nb, None]
    for i in (0, 1, 3, 4, 5, 7):
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for i, v in ((2, 0), (2, -1), (2, 2 ** 31), (6, 2), (6, 4), (8, nb - 1), (7, BAD)):          # n, unknown flags, scratch
        a = list(ok); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)
    for bd in bad_descs():
        a = list(ok); a[0] = C.byref(bd)
        assert f(*a) == ERR_ARG


def _cache(M=4):
    c = _lib.InrCache()
    c.mods, c.seg, c.ncases, c.numMods = 0x1000, 0x1000, 2, M
    c.hwd[0], c.hwd[1], c.hwd[2] = 16, 16, 16
    return c


def _cfg(micro=512, accum=2, warmup=2, decay=10):
    c = _lib.InrTrainCfg()
    c.microBatch, c.accum, c.warmupSteps, c.decaySteps, c.seed, c.peakLr, c.minLr, c.diceWeight = micro, accum, warmup, decay, 7, 1e-3, 1e-5, 0.5
    for k in range(16):
        c.classWeights[k] = 1.0
    c.adamw = _lib.AdamW(0.0, 0.9, 0.999, 1e-8, 1e-4, 1.0)
    return c


def test_train_run_refusals(lib):
    d, cache, cfg = desc(kind=1, M=4), _cache(), _cfg()
    st = _lib.InrTrainState(*[0x1000] * 6)
    size, run = lib.mrirt_siren_train_run_scratch_bytes, lib.mrirt_siren_train_run
    nb = size(C.byref(d), C.byref(cache), C.byref(cfg))
    assert nb > 0 and nb % 256 == 0
    assert nb > lib.mrirt_inr_train_run_scratch_bytes(C.byref(desc(kind=0, M=4)), C.byref(cache), C.byref(cfg)) > 0
    ok = [C.byref(d), C.byref(cache), C.byref(cfg), C.byref(st), 0, 3, P, P, nb, None]
    for i in (0, 1, 2, 3, 6, 7):
        a = list(ok); a[i] = None
        assert run(*a) == ERR_NULL, i
    for i, v in ((5, 0), (8, nb - 1), (7, BAD)):
        a = list(ok); a[i] = v
        assert run(*a) == ERR_ARG, (i, v)
    # the raw SIREN kind, the ReLU kinds, a cache with another modality count, every descriptor the step refuses
    for bd in [desc(kind=3), desc(kind=0, M=4), desc(kind=2), desc(kind=1, ind=5, M=2), desc(kind=1, M=4, w0=0.0), desc(kind=1, M=4, w0=float("nan")),
               desc(kind=1, M=4, hidden=48), desc(kind=1, ind=13, K=1, M=4)]:
        assert size(C.byref(bd), C.byref(cache), C.byref(cfg)) == 0
        a = list(ok); a[0] = C.byref(bd)
        assert run(*a) == ERR_ARG
    assert size(C.byref(d), C.byref(_cache(M=2)), C.byref(cfg)) == 0
    for bc in (_cfg(micro=0), _cfg(micro=2 ** 31), _cfg(accum=0), _cfg(warmup=10, decay=10)):
        assert size(C.byref(d), C.byref(cache), C.byref(bc)) == 0
    # the existing loop goes on refusing the SIREN kind
    assert lib.mrirt_inr_train_run_scratch_bytes(C.byref(d), C.byref(cache), C.byref(cfg)) == 0
    a = list(ok); a[8] = 1 << 40
    assert lib.mrirt_inr_train_run(*a) == ERR_ARG


def test_siren_init_bounds():
    import mrirt
    p = mrirt.inr.siren_init(3, 7, [64, 64, 64], 4, w0=30.0)
    assert sorted(p) == ["l0", "l1", "l2", "l3"]
    dims = [7, 64, 64, 64, 4]
    for i in range(4):
        w, b = p[f"l{i}"]["w"], p[f"l{i}"]["b"]
        assert w.dtype == np.float32 and w.shape == (dims[i], dims[i + 1]) and b.shape == (dims[i + 1],) and not b.any()
        lim = np.sqrt(6.0 / dims[i]) / (30.0 if i == 0 else 1.0)
        assert np.abs(w).max() <= lim and np.abs(w).max() > 0.9 * lim and abs(float(w.mean())) < 0.1 * lim
    q = mrirt.inr.siren_init(3, 7, [64, 64, 64], 4, w0=30.0)
    assert all(np.array_equal(p[k]["w"], q[k]["w"]) for k in p)
    assert np.abs(mrirt.inr.siren_init(3, 7, [32], 4, w0=1.0)["l0"]["w"]).max() > 0.5


def test_python_argument_errors():
    import mrirt
    inr = mrirt.inr
    d = inr.siren_train_desc([7, 64, 64, 4], 4, 30.0)
    assert (d.kind, d.numLayers, d.inDim, d.hidden, d.outDim, d.numMods, d.fourierFreqs) == (1, 3, 7, 64, 4, 4, 0)
    assert inr.siren_train_desc([9, 32, 2], None).kind == 3
    for bad in (lambda: inr.siren_train_desc([7, 64, 32, 4], 4), lambda: inr.siren_train_desc([7, 4], 4), lambda: inr.siren_train_desc([8, 64, 4], 4),
                lambda: inr.siren_train_desc([7, 64, 4], 4, 0.0), lambda: inr.siren_train_desc([7, 64, 4], 4, float("nan")),
                lambda: inr.make_siren_loss_and_grad(4, [1.0, 1.0], 0.5)):
        with pytest.raises(ValueError):
            bad()
    cfg = dict(GLOBAL_BATCH_SIZE=64, MICRO_BATCH_SIZE=32, HIDDEN_DIMS=[32], LR=1e-3, MIN_LR=1e-5, WARMUP_STEPS=2, TRAIN_STEPS=10, RNG_SEED=1,
               NUM_CLASSES=4, DICE_WEIGHT=0.5, CLASS_WEIGHTS=[1.0] * 4, CLIP_NORM=1.0)
    for bad in (dict(cfg, W0=0.0), dict(cfg, W0=float("inf")), dict(cfg, FOURIER_FREQS=2), dict(cfg, MICRO_BATCH_SIZE=0), dict(cfg, TRAIN_STEPS=0),
                dict(cfg, WARMUP_STEPS=5, TRAIN_STEPS=10)):          # decay_steps - warmup = 0: refused before any work
        with pytest.raises(ValueError):
            inr.train_siren(bad, [])
