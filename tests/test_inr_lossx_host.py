"""The argument checks of the extended loss, the tumour index, the mixed sampler and mrirt_inr_train_run_ext, on the CPU: every
refusal returns its code before anything is launched (no GPU is present; the pointers handed over are never dereferenced)."""
import ctypes as C
import pathlib
import re

import pytest

from mrirt import _lib
from test_inr_loop_host import BAD, ERR_ARG, ERR_DIMS, ERR_NULL, INF, NAN, P, cache, cfg, desc

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("mrirt_inr_loss_ext_scratch_bytes", "mrirt_inr_loss_ext", "mrirt_inr_tumour_count", "mrirt_inr_tumour_index_scratch_bytes",
               "mrirt_inr_tumour_index", "mrirt_inr_sample_batch_mix", "mrirt_inr_train_run_ext_scratch_bytes", "mrirt_inr_train_run_ext")


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def ext(gamma=0.0, eps=0.0, dw=0.5, fp=0.0, ta=0.8, tb=0.2, tw=0.0, reg=0.0, e=2, flags=1, cw=1.0, alpha=1.0):
    x = _lib.InrLossExt()
    for k in range(16):
        x.classWeights[k], x.focalAlpha[k] = cw, alpha
    x.diceWeight, x.focalGamma, x.labelSmoothing = dw, gamma, eps
    x.edemaFpWeight, x.tverskyAlpha, x.tverskyBeta, x.tverskyWeight, x.edemaLogitReg, x.edemaClass, x.flags = fp, ta, tb, tw, reg, e, flags
    return x


BAD_EXT = [dict(gamma=-1.0), dict(gamma=NAN), dict(gamma=0.5), dict(gamma=0.999), dict(gamma=8.5), dict(gamma=INF), dict(eps=-0.01), dict(eps=1.0),
           dict(eps=NAN), dict(dw=NAN), dict(dw=INF), dict(fp=-0.1), dict(fp=INF), dict(fp=NAN), dict(ta=-1.0), dict(ta=NAN), dict(tb=-1.0), dict(tb=INF),
           dict(tw=-0.5), dict(tw=NAN), dict(reg=-1.0), dict(reg=INF), dict(cw=NAN), dict(cw=INF), dict(flags=3, alpha=NAN), dict(flags=4),
           dict(e=4, fp=0.1), dict(e=4, tw=0.1), dict(e=7, reg=0.1)]
GOOD_EXT = [dict(), dict(gamma=1.0), dict(gamma=8.0), dict(eps=0.999), dict(e=4), dict(e=99, ta=5.0), dict(flags=1, alpha=NAN), dict(flags=0), dict(flags=3),
            dict(e=3, fp=0.1, tw=0.2, reg=0.3)]


def test_struct_sizes_and_symbols(lib):
    assert lib.mrirt_sizeof(13) == C.sizeof(_lib.InrLossExt) == 168
    assert lib.mrirt_sizeof(14) == C.sizeof(_lib.InrTumourIndex) == 16
    assert lib.mrirt_sizeof(15) == C.sizeof(_lib.InrTrainExt) == 40
    assert lib.mrirt_sizeof(12) == 0 and lib.mrirt_sizeof(16) == 0 and lib.mrirt_abi_version() == 4      # 12 stays unassigned
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mrirt.h").read_text(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert s in _lib.ABI_SYMBOLS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, header), s
    assert "inr_lossx.hip" in _lib.HIP_SOURCES


def test_loss_ext_scratch_bytes(lib):
    f = lib.mrirt_inr_loss_ext_scratch_bytes
    prev = 0
    for n in (1, 255, 256, 257, 65536, 65537, 2 ** 31 - 1):
        assert f(n) >= max(prev, lib.mrirt_inr_loss_scratch_bytes(n)) and f(n) % 256 == 0
        prev = f(n)
    assert f(65537) == f(2 ** 31 - 1) == ((257 * 71 * 8 + 255) & ~255)
    for n in (0, -1, 2 ** 31):
        assert f(n) == 0


def test_loss_ext_refusals(lib):
    f = lib.mrirt_inr_loss_ext
    n, nc = 1000, 4
    nbytes = lib.mrirt_inr_loss_ext_scratch_bytes(n)
    ok = [P, P, n, nc, C.byref(ext()), P, P, P, P, P, nbytes, None]
    for i in (0, 1, 4, 5, 6, 9):                         # logits, labels, ext, loss, aux, scratch; terms and dlogits may be NULL
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for i, v in ((2, 0), (2, -1), (2, 2 ** 31), (3, 0), (3, 17), (10, nbytes - 1), (10, -1), (9, BAD), (10, lib.mrirt_inr_loss_scratch_bytes(n))):
        a = list(ok); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)
    for kw in BAD_EXT:
        a = list(ok); a[4] = C.byref(ext(**kw))
        assert f(*a) == ERR_ARG, kw
    a = list(ok); a[4] = C.byref(ext(e=1, fp=0.1)); a[3] = 1          # the edema class must exist among num_classes
    assert f(*a) == ERR_ARG


def test_tumour_refusals(lib):
    cnt, idx, size = lib.mrirt_inr_tumour_count, lib.mrirt_inr_tumour_index, lib.mrirt_inr_tumour_index_scratch_bytes
    c = cache()
    nbytes = size(C.byref(c))
    assert nbytes == 256 * 1 and size(C.byref(cache(ncases=3, hwd=(67, 66, 65)))) == ((3 * 71 * 4 + 255) & ~255)
    assert cnt(None, P, None) == ERR_NULL and cnt(C.byref(c), None, None) == ERR_NULL
    ok = [C.byref(c), P, P, P, nbytes, None]
    for i in (0, 1, 2, 3):
        a = list(ok); a[i] = None
        assert idx(*a) == ERR_NULL, i
    for i, v in ((4, nbytes - 1), (4, -1), (3, BAD)):
        a = list(ok); a[i] = v
        assert idx(*a) == ERR_ARG, (i, v)
    for hwd in ((2048, 2048, 1024), (65536, 65536, 2), (4, 65536, 65536), (4294967295, 4294967295, 4294967295)):      # H W D >= 2^32
        b = cache(hwd=hwd)
        assert cnt(C.byref(b), P, None) == ERR_ARG and idx(C.byref(b), P, P, P, 1 << 40, None) == ERR_ARG and size(C.byref(b)) == 0, hwd
    for hwd in ((2048, 1024, 1024), (1, 5, 7)):          # the cache's own limits stay: H W D in [2^31, 2^32), an axis below 2
        b = cache(hwd=hwd)
        assert cnt(C.byref(b), P, None) == ERR_DIMS and idx(C.byref(b), P, P, P, 1 << 40, None) == ERR_DIMS and size(C.byref(b)) == 0, hwd
    assert cnt(C.byref(cache(seg=None)), P, None) == ERR_NULL and cnt(C.byref(cache(ncases=0)), P, None) == ERR_ARG


def test_sample_batch_mix_refusals(lib):
    f = lib.mrirt_inr_sample_batch_mix
    t = _lib.InrTumourIndex(0x1000, 0x1000)
    ok = [C.byref(cache()), C.byref(t), 1, 0, 100, 40, P, P, P, None]
    for i in (0, 1, 6, 7, 8):                            # cache, index (n_tumour > 0), coords, feats (M > 0), labels
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for bad in (_lib.InrTumourIndex(None, 0x1000), _lib.InrTumourIndex(0x1000, None)):
        a = list(ok); a[1] = C.byref(bad)
        assert f(*a) == ERR_NULL
    for n, nt in ((100, 101), (100, -1), (0, 0), (2 ** 31, 0), (1, 2)):
        a = list(ok); a[4], a[5] = n, nt
        assert f(*a) == ERR_ARG, (n, nt)
    assert f(C.byref(cache(hwd=(1, 5, 7))), C.byref(t), 1, 0, 100, 40, P, P, P, None) == ERR_DIMS


def train_ext(loss=None, muon=None, index=0x1000, offsets=0x1000, nt=0):
    x = _lib.InrTrainExt()
    if loss is not None:
        x.loss = C.pointer(loss)
    if muon is not None:
        x.muon = C.pointer(muon)
    x.tumour = _lib.InrTumourIndex(index, offsets)
    x.nTumour = nt
    return x


def test_train_run_ext_refusals(lib):
    f, fb = lib.mrirt_inr_train_run_ext, lib.mrirt_inr_train_run_ext_scratch_bytes
    d, c, g = desc(), cache(), cfg()
    muon = _lib.Muon(0.95, 1e-8, 0.0, (C.c_float * 3)(3.4445, -4.7750, 2.0315), 5, 1)
    plain = lib.mrirt_inr_train_run_scratch_bytes(C.byref(d), C.byref(c), C.byref(g))
    empty, full = train_ext(index=None, offsets=None), train_ext(ext(gamma=2.0, e=2, fp=0.1), muon, nt=120)
    assert fb(C.byref(d), C.byref(c), C.byref(g), C.byref(empty)) == plain > 0
    nbytes = fb(C.byref(d), C.byref(c), C.byref(g), C.byref(full))
    assert nbytes == lib.mrirt_inr_train_run_muon_scratch_bytes(C.byref(d), C.byref(c), C.byref(g)) + lib.mrirt_inr_loss_ext_scratch_bytes(300)
    sd = desc(kind=1, K=0); sd.w0 = 30.0                 # the SIREN kind picks the SIREN step
    assert fb(C.byref(sd), C.byref(c), C.byref(g), C.byref(empty)) == lib.mrirt_siren_train_run_scratch_bytes(C.byref(sd), C.byref(c), C.byref(g)) > 0
    st = _lib.InrTrainState(*[0x1000] * 6)
    ok = [C.byref(d), C.byref(c), C.byref(g), C.byref(full), C.byref(st), 0, 3, P, P, nbytes, None]
    for i in (0, 1, 2, 3, 4, 7, 8):
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for i, v in ((6, 0), (9, nbytes - 1), (8, BAD)):
        a = list(ok); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)
    bad = [(train_ext(ext(gamma=0.5)), ERR_ARG), (train_ext(ext(e=3, fp=0.1)), ERR_ARG), (train_ext(nt=301), ERR_ARG), (train_ext(nt=-1), ERR_ARG),
           (train_ext(nt=5, index=None), ERR_NULL), (train_ext(nt=5, offsets=None), ERR_NULL),
           (train_ext(muon=_lib.Muon(1.0, 1e-8, 0.0, (C.c_float * 3)(1, 1, 1), 5, 1)), ERR_ARG)]
    for x, code in bad:                                  # desc() has 3 classes: edema class 3 does not exist
        a = list(ok); a[3] = C.byref(x); a[9] = 1 << 40
        assert f(*a) == code
        assert fb(C.byref(d), C.byref(c), C.byref(g), C.byref(x)) == 0
    for b in (cfg(accum=0), cfg(micro=0), cfg(peak=NAN)):
        a = list(ok); a[2] = C.byref(b)
        assert f(*a) == ERR_ARG and fb(C.byref(d), C.byref(c), C.byref(b), C.byref(full)) == 0
    a = list(ok); a[0] = C.byref(desc(kind=2))           # the raw kinds have no run
    assert f(*a) == ERR_ARG
    assert fb(None, C.byref(c), C.byref(g), C.byref(full)) == 0 and fb(C.byref(d), C.byref(c), C.byref(g), None) == 0
    # what the checks accept, seen through the size function (nothing here may reach a launch: the pointers are not real)
    d4 = desc(out=4)
    for kw in GOOD_EXT:
        assert fb(C.byref(d4), C.byref(c), C.byref(g), C.byref(train_ext(ext(**kw), index=None, offsets=None))) > 0, kw
    for kw in BAD_EXT:
        assert fb(C.byref(d4), C.byref(c), C.byref(g), C.byref(train_ext(ext(**kw)))) == 0, kw
