"""The fp64 reference of the K1 backward pass pinned on the CPU, and the ABI's refusals (no GPU needed).

brats_grad_ref.py is what test_gpu_brats_grad.py measures the kernel against, so it is checked here three ways: its fp64 frame
against the oracle's fp32 frame, its autograd gradients against central differences of its own forward, and its closed form
(the formulas of include/mrirt.h) against autograd.  The decisions fp32 and fp64 must take alike (early termination, the two
saturation ends of the window) are asserted to have a margin on every sample of every case."""
import ctypes as C

import numpy as np
import pytest
import torch

import brats_grad_cases as bc
import brats_grad_ref as ref
from mrirt import _lib, params
from oracle import oracle_np as onp


@pytest.fixture(scope="module")
def solved():
    out = {}
    for c in bc.CASES:
        d = bc.data(c["name"])
        out[c["name"]] = (ref.autograd(c, d), ref.closed_form(c, d))
    return out


@pytest.mark.parametrize("name", bc.NAMES)
def test_fp64_forward_matches_the_oracle(name, solved):
    c, d = bc.BY_NAME[name], bc.data(name)
    H, W = c["hw"]
    frame = onp.brats_main(c["params"], d["vols"], d["labels"], d["preds"], c["ext"])
    C64 = solved[name][0][2].reshape(H, W, 3)
    assert np.abs(C64 - frame[..., :3]).max() <= 1e-5


@pytest.mark.parametrize("name", bc.NAMES)
def test_closed_form_equals_autograd(name, solved):
    (gv, gtf, _), cf = solved[name]
    for m in range(4):
        assert (gv[m] is None) == (cf.grad_vols[m] is None)
        if gv[m] is not None:
            assert np.all(np.abs(gv[m] - cf.grad_vols[m]) <= 1e-10 * np.maximum(cf.A_vols[m], 1.0))
            assert np.all(cf.grad_vols[m][cf.A_vols[m] == 0] == 0)
    assert np.all(np.abs(gtf - cf.grad_tf) <= 1e-10 * np.maximum(cf.A_tf, 1.0))


@pytest.mark.parametrize("name", bc.NAMES)
def test_autograd_equals_central_differences(name, solved):
    """32 voxels and the four scalars per case, relative error 1e-6.  The differences are taken per pixel before they are summed
    (C+ - C- is exact to 1e-16 of a pixel's colour instead of 1e-16 of the whole loss), with h = 5e-7 — below the 1e-6 margin that
    test_decisions_have_margin asserts, so no perturbed sample crosses a saturation end or flips a termination.  What is left of
    the difference's rounding is absolute, ~1e-16 / h; a relative 1e-6 therefore means something only on gradients well above
    1e-4, so the voxels are the 32 with the largest |gradient| (modality by modality, round robin)."""
    c, d = bc.BY_NAME[name], bc.data(name)
    (gv, gtf, _), cf = solved[name]
    G = torch.from_numpy(np.asarray(d["G"], np.float64).reshape(-1, 4)[:, :3])
    p = c["params"]
    tf0 = np.array([float(np.float32(p[k])) for k in ("ww", "wl", "intensityAlpha", "gamma")])
    base = [None if v is None else v.astype(np.float64) for v in d["vols"]]

    def diff(vols_p, vols_m, tf_p, tf_m):
        with torch.no_grad():
            Cp = ref.forward(c, d, [None if v is None else torch.from_numpy(v) for v in vols_p], torch.from_numpy(tf_p))
            Cm = ref.forward(c, d, [None if v is None else torch.from_numpy(v) for v in vols_m], torch.from_numpy(tf_m))
        return float(((Cp - Cm) * G).sum())

    h = 5e-7
    mods = [m for m in range(4) if gv[m] is not None]
    picks = []
    for m in mods:
        order = np.argsort(-np.abs(gv[m]))[: (32 + len(mods) - 1) // len(mods)]
        picks += [(m, int(i)) for i in order]
    for m, i in picks[:32]:
        vp, vm = [None if v is None else v.copy() for v in base], [None if v is None else v.copy() for v in base]
        vp[m][i] += h
        vm[m][i] -= h
        fd = diff(vp, vm, tf0, tf0) / (2 * h)
        assert abs(fd - gv[m][i]) <= 1e-6 * abs(gv[m][i]) + 1e-300, (name, m, i, fd, gv[m][i])
    for k in range(4):
        # ww and wl move u, so they keep h; intensityAlpha and gamma move only T, and by less than 0.2 h at the termination threshold
        # (T = 0.01 there; |dT/da| <= T sum(val) dt, |dT/dgamma| <= T a dt sum|val ln u|, at most 48 steps): h = 1e-5 stays inside the
        # 1e-5 margin on T and takes the difference's rounding twenty times further down
        hk = h if k < 2 else 1e-5
        tp, tm = tf0.copy(), tf0.copy()
        tp[k] += hk
        tm[k] -= hk
        fd = diff(base, base, tp, tm) / (2 * hk)
        assert abs(fd - gtf[k]) <= 1e-6 * abs(gtf[k]) + 1e-300, (name, k, fd, gtf[k])


@pytest.mark.parametrize("name", bc.NAMES)
def test_decisions_have_margin(name, solved):
    """What keeps the fp32 kernel's decisions and the fp64 reference's identical, over EVERY sample of the case: the transmittance
    in front of each loop test is not within 1e-5 of the termination threshold, and u is not within 1e-6 of either saturation end."""
    _, cf = solved[name]
    for s in cf.rec.steps:
        assert s.margin_T.min() > 1e-5, (name, s.margin_T.min())
        assert np.abs(s.u).min() > 1e-6 and np.abs(s.u - 1.0).min() > 1e-6, name


def test_the_case_list_covers_what_it_claims(solved):
    both = 0
    for name in bc.NAMES:
        _, cf = solved[name]
        assert len(cf.rec.steps) <= 48, name
        if cf.rec.steps:
            u = np.concatenate([s.u for s in cf.rec.steps])
            both += int((u < 0).any() and (u > 1).any())
    assert both >= 8                                              # both saturation ends occur
    assert not solved["all_miss"][1].rec.steps
    for name in ("dense_ert", "dense_ert_gamma_two", "overlays_dense"):   # part of the rays terminate early, part do not
        rec = solved[name][1].rec
        first = rec.steps[0].idx.size
        assert 0 < rec.steps[-1].idx.size < first, name


def test_fp32_reference_error_sets_the_tolerance(solved):
    """The largest |g_fp32,shuffled - g_fp64| / A of the reference's own fp32 evaluation over all cases and five shuffles: the
    constant next to TOL in brats_grad_cases.py is this measurement (it may only be restated from here, never from a kernel)."""
    worst = 0.0
    for c in bc.CASES:
        d = bc.data(c["name"])
        cf = solved[c["name"]][1]
        for sh in range(5):
            c32 = ref.closed_form(c, d, np.float32, sh)
            for m in range(4):
                if cf.grad_vols[m] is not None:
                    nz = cf.A_vols[m] > 0
                    assert np.all(c32.grad_vols[m][~nz] == 0)
                    if nz.any():
                        worst = max(worst, float((np.abs(c32.grad_vols[m].astype(np.float64) - cf.grad_vols[m])[nz] / cf.A_vols[m][nz]).max()))
            nz = cf.A_tf > 0
            if nz.any():
                worst = max(worst, float((np.abs(c32.grad_tf.astype(np.float64) - cf.grad_tf)[nz] / cf.A_tf[nz]).max()))
    print(f"fp32 reference error: {worst:.3e}; recorded {bc.FP32_REF_ERROR:.3e}; TOL {bc.TOL:.3e}")
    assert 0.5 * bc.FP32_REF_ERROR <= worst <= 1.05 * bc.FP32_REF_ERROR
    assert bc.TOL == min(8.0 * bc.FP32_REF_ERROR, 1e-3)


# --- the ABI's refusals: every check happens before any HIP call, so they are testable without a device --------------------
def _call(p, ext=None, vol=(0x1000, None, None, None), labels=None, preds=None, grad=0x1000, pitch=None, gv=(0x1000, None, None, None),
          gtf=0x1000, null_params=False, null_vol=False):
    P = params.brats_params(p)
    E = params.render_ext(ext) if ext is not None else None
    vp = (C.c_void_p * 4)(*vol)
    gp = (C.c_void_p * 4)(*gv)
    return int(_lib.lib().mrirt_render_brats_backward(None if null_params else C.byref(P), C.byref(E) if E is not None else None,
                                                      None if null_vol else vp, labels, preds, grad,
                                                      int(P.imageSize[0]) if pitch is None else pitch, gp, gtf, None))


def test_abi_symbol_and_refusals():
    assert "mrirt_render_brats_backward" in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), "mrirt_render_brats_backward")
    assert _lib.lib().mrirt_abi_version() == 4
    p = dict(bc.BY_NAME["one_modality"]["params"])
    NULL, DIMS, LAYOUT, ARG = -1, -2, -3, -5
    # what every K1 entry point checks
    assert _call(p, null_params=True) == NULL
    assert _call(p, null_vol=True) == NULL
    assert _call(p, grad=None) == NULL
    assert _call(p, vol=(None, None, None, None)) == NULL                       # an enabled modality without a grid
    assert _call(dict(p, showSeg=1)) == NULL and _call(dict(p, showPred=1)) == NULL
    assert _call(dict(p, dims=[13, 1, 7])) == DIMS
    assert _call(dict(p, stepSize=0.0)) == ARG and _call(dict(p, stepSize=float("nan"))) == ARG
    assert _call(p, pitch=int(p["imageSize"][0]) - 1) == ARG
    # out of scope for the backward pass
    for lay in ("brick", "vg", "quad", "vga", "mod4"):
        assert _call(p, ext=dict(layout=lay)) == LAYOUT, lay
    for lay in ("brick", "labcell"):
        assert _call(p, ext=dict(labelLayout=lay)) == LAYOUT, lay
    assert _call(p, ext=dict(shadeMode=1)) == ARG
    assert _call(p, ext=dict(tileSize=16, tileRank=0, tileWorld=2)) == ARG
    assert _call(p, ext=dict(outFormat="rgba16f")) == ARG
    assert _call(p, ext=dict(math="fast")) == ARG
    # nothing asked for: no launch, no device needed
    assert _call(p, gv=(None, None, None, None), gtf=None) == 0
    assert _call(p, ext={}, gv=(None, None, None, None), gtf=None) == 0
    assert _call(p, ext=dict(cameraMode=1, orthoHalfHeight=0.5), gv=(None, None, None, None), gtf=None) == 0
