"""The training entry points' argument checks, on the CPU: every refusal returns its code before anything is launched (no
GPU is present; the pointers handed over are never dereferenced), and mrirt_inr_train_scratch_bytes is monotone in n."""
import ctypes as C

import pytest

from mrirt import _lib

ERR_NULL, ERR_ARG = -1, -5
P = C.c_void_p(0x1000)            # a non-NULL, 16-byte aligned "device pointer" that is never read
BAD = C.c_void_p(0x1004)          # misaligned


def desc(kind=2, layers=3, ind=7, out=4, hidden=64, K=0, M=0):
    d = _lib.InrDesc()
    d.kind, d.numLayers, d.inDim, d.outDim, d.hidden, d.fourierFreqs, d.numMods = kind, layers, ind, out, hidden, K, M
    return d


@pytest.fixture(scope="module")
def lib():
    l = _lib.lib()
    assert l.mrirt_status_string(ERR_NULL).startswith(b"NULL") or b"NULL" in l.mrirt_status_string(ERR_NULL)
    return l


def test_scratch_bytes(lib):
    d = desc()
    prev = 0
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 16384, 16385, 65536, 10 ** 6, 2 ** 31 - 1):
        b = lib.mrirt_inr_train_scratch_bytes(C.byref(d), n)
        assert b >= prev > -1 and b > 0 and b % 256 == 0, n
        assert b >= lib.mrirt_inr_loss_scratch_bytes(n) > 0
        prev = b
    for n in (0, -1, 2 ** 31):
        assert lib.mrirt_inr_train_scratch_bytes(C.byref(d), n) == 0
        assert lib.mrirt_inr_loss_scratch_bytes(n) == 0
    for kind in (1, 3):                                   # the SIREN kinds
        assert lib.mrirt_inr_train_scratch_bytes(C.byref(desc(kind=kind, ind=7, M=4)), 100) == 0
    assert lib.mrirt_inr_train_scratch_bytes(C.byref(desc(hidden=48)), 100) == 0
    assert lib.mrirt_inr_train_scratch_bytes(C.byref(desc(out=17)), 100) == 0
    assert lib.mrirt_inr_train_scratch_bytes(C.byref(desc(kind=0, ind=31, K=4, M=4)), 100) > 0
    assert lib.mrirt_inr_train_scratch_bytes(C.byref(desc(kind=0, ind=30, K=4, M=4)), 100) == 0
    assert lib.mrirt_inr_train_scratch_bytes(None, 100) == 0


def test_forward_refusals(lib):
    d, n = desc(), 100
    nb = lib.mrirt_inr_train_scratch_bytes(C.byref(d), n)
    ok = [C.byref(d), P, P, None, P, n, P, P, nb, None]
    f = lib.mrirt_inr_forward_f32
    for i in (0, 1, 2, 4, 6, 7):                          # desc, w, b, feats (raw kind), logits, scratch
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for n_bad in (0, -5, 2 ** 31):
        a = list(ok); a[5] = n_bad
        assert f(*a) == ERR_ARG
    a = list(ok); a[8] = nb - 1
    assert f(*a) == ERR_ARG
    a = list(ok); a[7] = BAD
    assert f(*a) == ERR_ARG
    for kind in (1, 3):
        a = list(ok); a[0] = C.byref(desc(kind=kind, ind=7, M=4)); a[3] = P
        assert f(*a) == ERR_ARG
    fd = desc(kind=0, ind=31, K=4, M=4)
    nbf = lib.mrirt_inr_train_scratch_bytes(C.byref(fd), n)
    assert f(C.byref(fd), P, P, None, P, n, P, P, nbf, None) == ERR_NULL          # the Fourier kind needs coords
    assert f(C.byref(fd), P, P, P, None, n, P, P, nbf, None) == ERR_NULL          # ... and its intensities


def test_loss_refusals(lib):
    n = 100
    nb = lib.mrirt_inr_loss_scratch_bytes(n)
    cw = (C.c_float * 16)(*([1.0] * 16))
    f = lib.mrirt_inr_loss
    ok = [P, P, n, 4, cw, 0.5, P, P, P, P, nb, None]
    for i in (0, 1, 4, 6, 7, 9):                          # logits, labels, class_weights, loss, aux, scratch
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for i, v in ((2, 0), (2, -1), (3, 0), (3, 17), (5, float("nan")), (5, float("inf")), (5, float("-inf")), (10, nb - 1), (9, BAD)):
        a = list(ok); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)


def test_backward_refusals(lib):
    d, n = desc(), 100
    nb = lib.mrirt_inr_train_scratch_bytes(C.byref(d), n)
    f = lib.mrirt_inr_backward
    ok = [C.byref(d), P, n, P, P, P, 0, P, nb, None]
    for i in (0, 1, 3, 4, 5, 7):
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for i, v in ((2, 0), (2, -1), (6, 2), (8, nb - 1), (7, BAD), (0, C.byref(desc(kind=1, ind=7, M=4))), (0, C.byref(desc(kind=3)))):
        a = list(ok); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)
