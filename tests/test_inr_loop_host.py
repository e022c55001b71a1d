"""The training loop's entry points' argument checks, on the CPU: every refusal returns its code before anything is launched
(no GPU is present; the pointers handed over are never dereferenced)."""
import ctypes as C

import pytest

from mrirt import _lib

ERR_NULL, ERR_DIMS, ERR_ARG = -1, -2, -5
P = C.c_void_p(0x1000)            # a non-NULL, 16-byte aligned "device pointer" that is never read
BAD = C.c_void_p(0x1004)          # misaligned
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def cache(ncases=2, M=2, hwd=(3, 5, 7), mods=0x1000, seg=0x1000):
    c = _lib.InrCache()
    c.mods, c.seg, c.ncases, c.numMods = mods, seg, ncases, M
    c.hwd[0], c.hwd[1], c.hwd[2] = hwd
    return c


def desc(kind=0, layers=3, K=2, M=2, hidden=32, out=3):
    d = _lib.InrDesc()
    d.kind, d.numLayers, d.inDim, d.outDim, d.hidden, d.fourierFreqs, d.numMods = kind, layers, 3 + 6 * K + M, out, hidden, K, M
    return d


def cfg(micro=300, accum=2, warmup=2, decay=12, peak=5e-3, end=1e-4, dw=0.5, cw=1.0, hp=None):
    c = _lib.InrTrainCfg()
    c.microBatch, c.accum, c.warmupSteps, c.decaySteps, c.seed, c.peakLr, c.minLr, c.diceWeight = micro, accum, warmup, decay, 7, peak, end, dw
    for k in range(16):
        c.classWeights[k] = cw
    c.adamw = hp or adamw()
    return c


def adamw(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-4, clip=1.0):
    return _lib.AdamW(lr, b1, b2, eps, wd, clip)


def test_sample_batch_refusals(lib):
    f = lib.mrirt_inr_sample_batch
    ok = [C.byref(cache()), 1, 0, 100, P, P, P, None]
    for i in (0, 4, 5, 6):                                # cache, coords, feats (M > 0), labels
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    assert f(C.byref(cache(seg=None)), 1, 0, 100, P, P, P, None) == ERR_NULL
    assert f(C.byref(cache(mods=None)), 1, 0, 100, P, P, P, None) == ERR_NULL
    for n in (0, -1, 2 ** 31):
        a = list(ok); a[3] = n
        assert f(*a) == ERR_ARG, n
    for hwd in ((1, 5, 7), (3, 1, 7), (3, 5, 1), (3, 5, 0), (2048, 1024, 1024), (65536, 65536, 2)):
        assert f(C.byref(cache(hwd=hwd)), 1, 0, 100, P, P, P, None) == ERR_DIMS, hwd
    for nc in (0, 65536):
        assert f(C.byref(cache(ncases=nc)), 1, 0, 100, P, P, P, None) == ERR_ARG, nc
    assert f(C.byref(cache(M=9)), 1, 0, 100, P, P, P, None) == ERR_ARG


def test_adamw_refusals(lib):
    f = lib.mrirt_inr_adamw_step
    nw, nb = 1000, 70
    nbytes = lib.mrirt_inr_adamw_scratch_bytes(nw + nb)
    assert nbytes > 0 and nbytes % 256 == 0
    prev = 0
    for n in (1, 255, 256, 257, 65536, 65537, 2 ** 31 - 1):
        b = lib.mrirt_inr_adamw_scratch_bytes(n)
        assert b >= prev and b > 0
        prev = b
    for n in (0, -1, 2 ** 31):
        assert lib.mrirt_inr_adamw_scratch_bytes(n) == 0
    ok = [P, P, P, P, P, P, P, P, nw, nb, C.byref(adamw()), 0, 1.0, P, P, nbytes, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 10, 13, 14):
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for i, v in ((8, 0), (8, -1), (9, -1), (8, 2 ** 31), (12, NAN), (12, INF), (15, nbytes - 1), (15, -1), (14, BAD), (13, C.c_void_p(0x1004))):
        a = list(ok); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)
    for hp in (adamw(lr=NAN), adamw(lr=INF), adamw(b1=1.0), adamw(b1=-0.1), adamw(b1=NAN), adamw(b2=1.0), adamw(b2=INF), adamw(eps=0.0),
               adamw(eps=NAN), adamw(wd=INF), adamw(wd=NAN), adamw(clip=NAN), adamw(clip=-INF)):
        a = list(ok); a[10] = C.byref(hp)
        assert f(*a) == ERR_ARG


def test_lr_schedule_refusals(lib):
    out = C.c_double()
    f = lib.mrirt_inr_lr_schedule
    assert f(1e-3, 1e-5, 2, 12, 0, None) == ERR_NULL
    for peak, end, w, d in ((1e-3, 1e-5, 10, 10), (1e-3, 1e-5, 10, 5), (0.0, 0.0, 2, 12), (-1e-3, 0.0, 2, 12), (NAN, 0.0, 2, 12), (INF, 0.0, 2, 12),
                            (1e-3, NAN, 2, 12), (1e-3, -1e-5, 2, 12)):
        assert f(peak, end, w, d, 0, C.byref(out)) == ERR_ARG, (peak, end, w, d)


def test_train_run_refusals(lib):
    f, fb = lib.mrirt_inr_train_run, lib.mrirt_inr_train_run_scratch_bytes
    d, c, g = desc(), cache(), cfg()
    nbytes = fb(C.byref(d), C.byref(c), C.byref(g))
    assert nbytes > 0 and nbytes % 256 == 0
    assert nbytes > lib.mrirt_inr_train_scratch_bytes(C.byref(d), 300)
    st = _lib.InrTrainState(*[0x1000] * 6)
    ok = [C.byref(d), C.byref(c), C.byref(g), C.byref(st), 0, 3, P, P, nbytes, None]
    for i in (0, 1, 2, 3, 6, 7):
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for k in range(6):
        ptrs = [0x1000] * 6
        ptrs[k] = None
        a = list(ok); a[3] = C.byref(_lib.InrTrainState(*ptrs))
        assert f(*a) == ERR_NULL, k
    for i, v in ((5, 0), (8, nbytes - 1), (7, BAD)):
        a = list(ok); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)
    bad_cfg = [cfg(accum=0), cfg(micro=0), cfg(micro=2 ** 31), cfg(warmup=12, decay=12), cfg(peak=0.0), cfg(peak=NAN), cfg(end=INF), cfg(dw=NAN),
               cfg(dw=INF), cfg(cw=NAN), cfg(hp=adamw(b1=1.0)), cfg(hp=adamw(eps=0.0)), cfg(hp=adamw(wd=NAN)), cfg(hp=adamw(clip=NAN))]
    for b in bad_cfg:
        a = list(ok); a[2] = C.byref(b)
        assert f(*a) == ERR_ARG
        assert fb(C.byref(d), C.byref(c), C.byref(b)) == 0
    for bd in (desc(kind=2), desc(kind=1), desc(M=4), desc(hidden=48), desc(out=17)):        # raw / SIREN kinds, other modality count, bad shapes
        a = list(ok); a[0] = C.byref(bd)
        assert f(*a) == ERR_ARG
        assert fb(C.byref(bd), C.byref(c), C.byref(g)) == 0
    for bc, code in ((cache(hwd=(1, 5, 7)), ERR_DIMS), (cache(ncases=0), ERR_ARG), (cache(seg=None), ERR_NULL)):
        a = list(ok); a[1] = C.byref(bc)
        assert f(*a) == code
        assert fb(C.byref(d), C.byref(bc), C.byref(g)) == 0
    assert fb(None, C.byref(c), C.byref(g)) == 0 and fb(C.byref(d), None, C.byref(g)) == 0 and fb(C.byref(d), C.byref(c), None) == 0


def test_struct_sizes(lib):
    for which, st in ((7, _lib.InrCache), (8, _lib.AdamW), (9, _lib.InrTrainCfg), (10, _lib.InrTrainState)):
        assert lib.mrirt_sizeof(which) == C.sizeof(st)
