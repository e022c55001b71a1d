"""Muon's ABI, argument checks and configuration handling, on the CPU: every refusal returns its code before anything is
launched (no GPU is present; the pointers handed over are never dereferenced)."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

from mrirt import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
ERR_NULL, ERR_DIMS, ERR_ARG = -1, -2, -5
P = C.c_void_p(0x1000)            # a non-NULL, 16-byte aligned "device pointer" that is never read
BAD = C.c_void_p(0x1004)          # misaligned
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def desc(kind=0, layers=3, K=2, M=2, hidden=32, out=3, w0=0.0):
    d = _lib.InrDesc()
    in_dim = 3 + 6 * K + M if kind == 0 else 3 + M
    d.kind, d.numLayers, d.inDim, d.outDim, d.hidden, d.fourierFreqs, d.numMods, d.w0 = kind, layers, in_dim, out, hidden, K if kind == 0 else 0, M, w0
    return d


def muon(beta=0.95, eps=1e-8, wd=0.0, coeffs=(3.4445, -4.7750, 2.0315), steps=5, nesterov=1):
    return _lib.Muon(beta, eps, wd, (C.c_float * 3)(*coeffs), steps, nesterov)


def adamw(lr=2e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, clip=1.0):
    return _lib.AdamW(lr, b1, b2, eps, wd, clip)


BAD_MUON = [dict(beta=1.0), dict(beta=-0.1), dict(beta=NAN), dict(beta=INF), dict(eps=0.0), dict(eps=-1e-8), dict(eps=NAN), dict(eps=INF),
            dict(wd=NAN), dict(wd=INF), dict(coeffs=(NAN, 1.0, 1.0)), dict(coeffs=(1.0, INF, 1.0)), dict(coeffs=(1.0, 1.0, -INF)),
            dict(steps=0), dict(steps=17), dict(nesterov=2)]
BAD_DESC = [dict(hidden=48), dict(out=17), dict(layers=9), dict(layers=1), dict(kind=1, w0=0.0), dict(kind=7)]


def test_struct_size_and_symbols(lib):
    assert lib.mrirt_sizeof(11) == C.sizeof(_lib.Muon) == 32
    assert lib.mrirt_sizeof(12) == 0
    assert lib.mrirt_abi_version() == 4
    header = (ROOT / "include" / "mrirt.h").read_text()
    declared = set(re.findall(r"\b(mrirt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib.ABI_SYMBOLS)
    for s in ("mrirt_muon_scratch_bytes", "mrirt_muon_orthogonalize", "mrirt_muon_step", "mrirt_inr_train_run_muon_scratch_bytes",
              "mrirt_inr_train_run_muon"):
        assert s in _lib.ABI_SYMBOLS and hasattr(lib, s)


def test_scratch_bytes(lib):
    prev = 0
    for hidden in (32, 64, 128, 256):
        b = lib.mrirt_muon_scratch_bytes(C.byref(desc(hidden=hidden)))
        assert b > prev and b % 256 == 0
        prev = b
    assert lib.mrirt_muon_scratch_bytes(C.byref(desc(kind=1, w0=30.0))) > 0          # the SIREN kinds too
    assert lib.mrirt_muon_scratch_bytes(None) == 0
    for bd in BAD_DESC:
        assert lib.mrirt_muon_scratch_bytes(C.byref(desc(**bd))) == 0, bd
    # four matrices of the flat layout (m^, O, two iterates) and two sets of Gram matrices fit
    d = desc(hidden=64)
    dims = [d.inDim, 64, 64, 3]
    nw = sum(a * b for a, b in zip(dims[:-1], dims[1:]))
    gram = sum(min(a, b) ** 2 for a, b in zip(dims[:-1], dims[1:]))
    assert lib.mrirt_muon_scratch_bytes(C.byref(d)) >= 4 * (4 * nw + 2 * gram)


def test_orthogonalize_refusals(lib):
    f = lib.mrirt_muon_orthogonalize
    d = desc()
    nbytes = lib.mrirt_muon_scratch_bytes(C.byref(d))
    ok = [C.byref(d), P, P, C.byref(muon()), P, nbytes, None]
    for i in (0, 1, 2, 3, 4):
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for i, v in ((5, nbytes - 1), (5, -1), (5, 0), (4, BAD)):
        a = list(ok); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)
    for bad in BAD_MUON:
        a = list(ok); a[3] = C.byref(muon(**bad))
        assert f(*a) == ERR_ARG, bad
    for bd in BAD_DESC:
        a = list(ok); a[0] = C.byref(desc(**bd))
        assert f(*a) == ERR_ARG, bd
    for good in (dict(beta=0.0), dict(steps=1), dict(steps=16), dict(nesterov=0), dict(wd=0.1)):       # the edges of the accepted ranges
        a = list(ok); a[3] = C.byref(muon(**good)); a[5] = nbytes - 1
        assert f(*a) == ERR_ARG                                                   # reaches the scratch check: the hp passed


def test_step_refusals(lib):
    f = lib.mrirt_muon_step
    d = desc()
    nbytes = lib.mrirt_muon_scratch_bytes(C.byref(d))
    ok = [C.byref(d), P, P, P, P, P, P, P, C.byref(muon()), C.byref(adamw()), 0, 1.0, P, P, nbytes, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13):
        a = list(ok); a[i] = None
        assert f(*a) == ERR_NULL, i
    for i, v in ((11, NAN), (11, INF), (14, nbytes - 1), (14, -1), (13, BAD), (12, C.c_void_p(0x1004))):
        a = list(ok); a[i] = v
        assert f(*a) == ERR_ARG, (i, v)
    for bad in BAD_MUON:
        a = list(ok); a[8] = C.byref(muon(**bad))
        assert f(*a) == ERR_ARG, bad
    for hp in (adamw(lr=NAN), adamw(lr=INF), adamw(b1=1.0), adamw(b2=-0.1), adamw(eps=0.0), adamw(wd=NAN), adamw(clip=NAN), adamw(clip=-INF)):
        a = list(ok); a[9] = C.byref(hp)
        assert f(*a) == ERR_ARG
    for bd in BAD_DESC:
        a = list(ok); a[0] = C.byref(desc(**bd))
        assert f(*a) == ERR_ARG, bd


def _cache(M=2, hwd=(3, 5, 7), ncases=2, seg=0x1000):
    c = _lib.InrCache()
    c.mods, c.seg, c.ncases, c.numMods = 0x1000, seg, ncases, M
    c.hwd[0], c.hwd[1], c.hwd[2] = hwd
    return c


def _cfg(micro=300, accum=2, warmup=0, decay=12, peak=2e-4, end=2e-4, hp=None):
    c = _lib.InrTrainCfg()
    c.microBatch, c.accum, c.warmupSteps, c.decaySteps, c.seed, c.peakLr, c.minLr, c.diceWeight = micro, accum, warmup, decay, 7, peak, end, 0.5
    for k in range(16):
        c.classWeights[k] = 1.0
    c.adamw = hp or adamw(lr=0.0, clip=0.0)
    return c


def test_train_run_muon_refusals(lib):
    f, fb = lib.mrirt_inr_train_run_muon, lib.mrirt_inr_train_run_muon_scratch_bytes
    for d in (desc(), desc(kind=1, w0=30.0)):                                     # both families by desc->kind
        c, g = _cache(), _cfg()
        nbytes = fb(C.byref(d), C.byref(c), C.byref(g))
        plain = (lib.mrirt_siren_train_run_scratch_bytes if d.kind == 1 else lib.mrirt_inr_train_run_scratch_bytes)(C.byref(d), C.byref(c), C.byref(g))
        assert plain > 0 and nbytes == plain + lib.mrirt_muon_scratch_bytes(C.byref(d))
        st = _lib.InrTrainState(*[0x1000] * 6)
        ok = [C.byref(d), C.byref(c), C.byref(g), C.byref(muon()), C.byref(st), 0, 3, P, P, nbytes, None]
        for i in (0, 1, 2, 3, 4, 7, 8):
            a = list(ok); a[i] = None
            assert f(*a) == ERR_NULL, i
        for i, v in ((6, 0), (9, nbytes - 1), (9, plain), (8, BAD)):
            a = list(ok); a[i] = v
            assert f(*a) == ERR_ARG, (i, v)
        for bad in BAD_MUON:
            a = list(ok); a[3] = C.byref(muon(**bad))
            assert f(*a) == ERR_ARG, bad
        for b in (_cfg(accum=0), _cfg(micro=0), _cfg(warmup=12), _cfg(peak=0.0), _cfg(hp=adamw(b1=1.0)), _cfg(hp=adamw(eps=0.0))):
            a = list(ok); a[2] = C.byref(b)
            assert f(*a) == ERR_ARG
            assert fb(C.byref(d), C.byref(c), C.byref(b)) == 0
        for bd in (dict(M=4), dict(hidden=48), dict(out=17)):
            bad_desc = desc(kind=d.kind, w0=d.w0, **bd)
            a = list(ok); a[0] = C.byref(bad_desc)
            assert f(*a) == ERR_ARG, bd
            assert fb(C.byref(bad_desc), C.byref(c), C.byref(g)) == 0
        a = list(ok); a[1] = C.byref(_cache(hwd=(1, 5, 7)))
        assert f(*a) == ERR_DIMS
    raw = desc(kind=2)
    assert fb(C.byref(raw), C.byref(_cache()), C.byref(_cfg())) == 0              # the raw kinds have no sampler input: refused
    assert fb(None, C.byref(_cache()), C.byref(_cfg())) == 0


# ---- configuration ---------------------------------------------------------------------------------------------------------------

def test_config_parsing():
    from mrirt import inr
    assert inr._optimizer_of({}) is None
    for other in ("adamw", "sgd", "Muon", "", None):                              # anything but "muon": the reference's else-branch
        assert inr._optimizer_of({"OPTIMIZER_CHOICE": other}) is None
    hp = inr._optimizer_of({"OPTIMIZER_CHOICE": "muon"})
    assert (hp.beta, hp.eps, hp.weightDecay, hp.nsSteps, hp.nesterov) == (np.float32(0.95), np.float32(1e-8), 0.0, 5, 1)
    assert list(hp.nsCoeffs) == [np.float32(3.4445), np.float32(-4.7750), np.float32(2.0315)]
    assert (inr.MUON_BETA, inr.MUON_NS_STEPS, inr.MUON_NS_COEFFS, inr.MUON_EPS, inr.MUON_WEIGHT_DECAY, inr.MUON_NESTEROV) == \
        (0.95, 5, (3.4445, -4.7750, 2.0315), 1e-8, 0.0, True)
    assert (inr.MUON_BIAS_B1, inr.MUON_BIAS_B2, inr.MUON_BIAS_EPS, inr.MUON_BIAS_WEIGHT_DECAY) == (0.9, 0.999, 1e-8, 0.0)
    hp = inr._optimizer_of({"OPTIMIZER_CHOICE": "muon", "MUON_BETA": 0.9, "MUON_NS_STEPS": 3, "MUON_NESTEROV": False, "MUON_WEIGHT_DECAY": 0.01})
    assert (hp.beta, hp.nsSteps, hp.nesterov, hp.weightDecay) == (np.float32(0.9), 3, 0, np.float32(0.01))
    with pytest.raises(ValueError):
        inr.muon_hp(ns_coeffs=(1.0, 2.0))


CONFIG = dict(GLOBAL_BATCH_SIZE=64, MICRO_BATCH_SIZE=64, FOURIER_FREQS=1, HIDDEN_DIMS=[32], LR=2e-4, MIN_LR=2e-4, WARMUP_STEPS=0, TRAIN_STEPS=4,
              RNG_SEED=1, NUM_CLASSES=3, DICE_WEIGHT=0.5, CLASS_WEIGHTS=[1.0, 1.0, 1.0], CLIP_NORM=0.0)


def _checkpoint(tmp_path, optimizer):
    dims = [3 + 6 + 1, 32, 3]
    flat = {}
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        flat[f"W_{i}"], flat[f"b_{i}"] = np.zeros((a, b), np.float32), np.zeros(b, np.float32)
    ck = tmp_path / f"{optimizer or 'plain'}.npz"
    np.savez_compressed(ck, **flat)
    nw, nb = 10 * 32 + 32 * 3, 35
    extra = {"optimizer": np.str_(optimizer)} if optimizer == "muon" else {}
    np.savez_compressed(ck.with_name(ck.stem + "_opt.npz"), step=np.int64(2), mu_w=np.zeros(nw, np.float32), mu_b=np.zeros(nb, np.float32),
                        nu_w=np.zeros(nw, np.float32), nu_b=np.zeros(nb, np.float32), **extra)
    return ck


def test_resume_with_the_other_optimiser_is_refused(tmp_path):
    """Refused from the files alone, before a cache is built or the GPU is touched (there is none here)."""
    from mrirt import inr
    cases = [{"mods": np.zeros((1, 4, 4, 4), np.float32), "seg": np.zeros((4, 4, 4), np.int16)}]
    with pytest.raises(ValueError, match="adamw's, the config asks for muon"):
        inr.train_inr(dict(CONFIG, OPTIMIZER_CHOICE="muon"), cases, resume_from=_checkpoint(tmp_path, "adamw"))      # no key: AdamW's
    with pytest.raises(ValueError, match="muon's, the config asks for adamw"):
        inr.train_inr(CONFIG, cases, resume_from=_checkpoint(tmp_path, "muon"))
    with pytest.raises(ValueError, match="muon's, the config asks for adamw"):
        inr.train_siren(dict({k: v for k, v in CONFIG.items() if k != "FOURIER_FREQS"}, OPTIMIZER_CHOICE="sgd"), cases,
                        resume_from=_checkpoint(tmp_path, "muon"))
