"""The reference of the soft prediction overlay pinned on the CPU, and the two entry points' refusals (no GPU needed).

brats_soft_ref.py is what test_gpu_brats_soft.py measures the kernels against, so it is checked here three ways: its fp64 frame
for one-hot logits of +-1e4 against the oracle's class-stream render (oracle_np.brats_main_inr), its autograd gradients against
central differences of its own forward, and the closed form of include/mrirt.h against autograd.  Every loop test of every
case is asserted to have a margin, the reference's own fp32 deviation (which sets the GPU tolerances) is measured and compared
with what brats_soft_cases.py records, and the fitting loop's fp64 history is reproduced."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import brats_soft_cases as sc
import brats_soft_ref as ref
import inr_loop_ref as loop
from mrirt import _lib, params
from oracle import oracle_np as onp

warnings.filterwarnings("ignore", message="The given NumPy array is not writable")


@functools.lru_cache(maxsize=None)
def solved(name):
    c, d, g = sc.BY_NAME[name], sc.data(name), sc.geo(name)
    return ref.autograd(c, d, g), ref.closed_form(c, d, geo=g)


@functools.lru_cache(maxsize=None)
def e2e_solved(which):
    """fp64 and fp32 autograd of MLP + render, the closed form on the fp64 logits and A of the weights."""
    c, d = sc.E2E_CASE, sc.e2e_data()
    g = ref.geometry(c)
    kind, par, _ = sc.E2E_NETS[which]
    layers = sc.e2e_layers(which)
    coords, feats = ref.mlp_inputs(c, d, g)
    r64 = ref.end_to_end(c, d, (kind, par), layers, torch.float64, g, coords, feats)
    r32 = ref.end_to_end(c, d, (kind, par), layers, torch.float32, g, coords, feats)
    cf = ref.closed_form(c, dict(d, logits=r64[3].numpy()), geo=g)
    Ws = [torch.from_numpy(p["W"].astype(np.float64)) for p in layers]
    bs = [torch.from_numpy(p["b"].astype(np.float64)) for p in layers]
    Aw, Ab = ref.weight_abs_scale((kind, par), Ws, bs, torch.from_numpy(coords), torch.from_numpy(feats), cf.A)
    return r64, r32, cf, Aw, Ab


def _one_hot(name, seed=0):
    """(logits fp32 of +-1e4, classes) with a random class per row."""
    d = sc.data(name)
    rng = np.random.default_rng(1000 + seed)
    cls = rng.integers(0, d["logits"].shape[1], d["logits"].shape[0])
    z = np.full(d["logits"].shape, -1e4, np.float32)
    z[np.arange(cls.size), cls] = 1e4
    return z, cls


@pytest.mark.parametrize("name", sc.NAMES)
def test_one_hot_logits_reproduce_the_oracles_class_stream_render(name):
    c, d = sc.BY_NAME[name], sc.data(name)
    H, W = c["hw"]
    z, cls = _one_hot(name)
    C64 = ref.forward(c, d, torch.from_numpy(z), geo=sc.geo(name)).numpy().reshape(H, W, 3)
    frame = onp.brats_main_inr(dict(c["params"], showPred=1), d["vols"], None, 0, None, None, d["labels"], c["ext"],
                               class_stream=cls, ray_offsets=d["offsets"])
    assert np.abs(C64 - frame[..., :3]).max() <= 1e-5
    # ... and the event's colour is the LUT row exactly
    lut = np.asarray(c["params"]["lutColorAlpha"], np.float32).reshape(8, 4)
    _, sigma, has, _, col = ref.soft_event(torch.from_numpy(z.astype(np.float64)), lut, 0.06)
    drawn = (cls >= 1) & (cls < 8)
    assert np.array_equal(has.numpy(), drawn)
    assert np.array_equal(col.numpy()[drawn], lut[cls[drawn], :3].astype(np.float64))


@pytest.mark.parametrize("name", sc.NAMES)
def test_closed_form_equals_autograd(name):
    (ag, fr), cf = solved(name)
    assert np.all(np.abs(ag - cf.dlogits) <= 1e-10 * cf.A + 1e-300)
    assert np.all(ag[cf.A == 0] == 0) and np.all(cf.dlogits[cf.A == 0] == 0)
    assert np.all(np.abs(cf.dlogits) <= cf.A * (1 + 1e-12))
    assert np.array_equal(fr, cf.frame)
    assert not cf.A[~sc.owned_rows(name)].any()                      # gap and guard rows belong to nobody


@pytest.mark.parametrize("name", sc.NAMES)
def test_autograd_equals_central_differences(name):
    """The 24 logits with the largest |gradient| per case, relative error 1e-6.  The differences are taken per pixel before they
    are summed; h = 1e-5 moves T by less than 1e-5 relative, inside the 1e-4 band test_decisions_have_margin asserts, so no
    perturbed ray terminates elsewhere."""
    c, d, g = sc.BY_NAME[name], sc.data(name), sc.geo(name)
    (ag, _), _ = solved(name)
    G = torch.from_numpy(np.asarray(d["G"], np.float64).reshape(-1, 4)[:, :3])
    z0 = d["logits"].astype(np.float64)
    h = 1e-5
    for flat in np.argsort(-np.abs(ag).reshape(-1))[:24]:
        if ag.reshape(-1)[flat] == 0:
            break
        zp, zm = z0.copy(), z0.copy()
        zp.reshape(-1)[flat] += h
        zm.reshape(-1)[flat] -= h
        with torch.no_grad():
            fd = float(((ref.forward(c, d, torch.from_numpy(zp), geo=g) - ref.forward(c, d, torch.from_numpy(zm), geo=g)) * G).sum()) / (2 * h)
        assert abs(fd - ag.reshape(-1)[flat]) <= 1e-6 * abs(ag.reshape(-1)[flat]) + 1e-300, (name, flat, fd, ag.reshape(-1)[flat])


def _margins(rec):
    mT = min([s.margin_T.min() for s in rec.steps if s.margin_T.size] or [np.inf])
    mt = min([s.margin_t.min() for s in rec.steps if s.margin_t.size] or [np.inf])
    return mT, mt


@pytest.mark.parametrize("name", sc.NAMES + ["e2e_siren", "e2e_fourier", "fit"])
def test_decisions_have_margin(name):
    """What keeps the fp32 kernel's decisions and the fp64 reference's identical, at EVERY loop test of the case: T is not within
    a 1e-4 relative band of the termination threshold and t is not within 4 ulp of t1."""
    if name in sc.BY_NAME:
        recs = [solved(name)[1].rec]
    elif name.startswith("e2e_"):
        recs = [e2e_solved(name[4:])[2].rec]
    else:
        views, teacher, start = sc.fit_data()
        recs = []
        for layers in (teacher, start):
            for c, d in zip(sc.FIT_CASES, views):
                g = ref.geometry(c)
                co, fe = ref.mlp_inputs(c, d, g)
                Ws = [torch.from_numpy(p["W"].astype(np.float64)) for p in layers]
                bs = [torch.from_numpy(p["b"].astype(np.float64)) for p in layers]
                lg = ref.apply_net(("siren", sc.FIT_CONFIG["W0"]), Ws, bs, torch.from_numpy(co), torch.from_numpy(fe))
                recs.append(ref.forward(c, d, lg, record=True, geo=g)[1])
    for rec in recs:
        mT, mt = _margins(rec)
        assert mT > 1e-4 and mt > 4.0, (name, mT, mt)


def test_the_case_list_covers_what_it_claims():
    assert {c["classes"] for c in sc.CASES} == {1, 2, 4, 9, 16}
    assert {c["hw"] for c in sc.CASES} == {(20, 24), (8, 8)} and {c["dims"] for c in sc.CASES} == {(13, 9, 7), (8, 8, 8)}
    for name in sc.NAMES:
        assert sc.geo(name).counts.max(initial=0) <= 48, name
    assert sc.data("all_miss")["rows"] == 0 and not sc.geo("all_miss").live.any()
    for name in ("c16_dense_ert", "c4_dense_ert_seg", "reversed_gaps"):       # part of the rays terminate early, part do not
        d, rec = sc.data(name), solved(name)[1].rec
        assert 0 < rec.composited < int(d["counts"].sum()), name
        taken = np.zeros(d["counts"].size, np.int64)
        for s in rec.steps:
            if not s.empty:
                taken[s.idx] += 1
        assert (taken == d["counts"])[d["counts"] > 0].any() and (taken < d["counts"]).any(), name
    assert not solved("c1_no_events")[1].A.any()
    for name in ("c9_half_zero", "c16_dense_ert"):                              # classes >= 8 get a gradient, through the softmax alone
        assert np.abs(solved(name)[1].dlogits[:, 8:]).max() > 0
    d = sc.data("reversed_gaps")
    assert d["offsets"][0] > d["offsets"][-1] and (~sc.owned_rows("reversed_gaps"))[:d["rows"]].sum() >= 2 * 480


def test_fp32_reference_error():
    """The fp64 reference's OWN fp32 deviation, frame and gradients, over all cases and over the end-to-end composition: the
    constants in brats_soft_cases.py are this measurement (they may only be restated from here, never from a kernel), and the
    fp32 reference alone stays inside the tolerances they give."""
    wf = wg = 0.0
    for c in sc.CASES:
        name = c["name"]
        cf = solved(name)[1]
        c32 = ref.closed_form(c, sc.data(name), np.float32, geo=sc.geo(name))
        assert len(cf.rec.steps) == len(c32.rec.steps) and all(np.array_equal(a.idx, b.idx) for a, b in zip(cf.rec.steps, c32.rec.steps))
        nz = cf.A > 0
        assert np.all(c32.dlogits[~nz] == 0)
        ef = float(np.abs(c32.frame - cf.frame).max())
        eg = float((np.abs(c32.dlogits - cf.dlogits)[nz] / cf.A[nz]).max()) if nz.any() else 0.0
        assert ef <= sc.TOL_F and np.all(np.abs(c32.dlogits - cf.dlogits) <= sc.TOL_G * cf.A)
        wf, wg = max(wf, ef), max(wg, eg)
    print(f"fp32 reference error: frame {wf:.3e} (recorded {sc.FP32_REF_ERROR_FRAME:.3e}, TOL_F {sc.TOL_F:.3e}); "
          f"gradients {wg:.3e} (recorded {sc.FP32_REF_ERROR_GRAD:.3e}, TOL_G {sc.TOL_G:.3e})")
    assert 0.5 * sc.FP32_REF_ERROR_FRAME <= wf <= 1.05 * sc.FP32_REF_ERROR_FRAME
    assert 0.5 * sc.FP32_REF_ERROR_GRAD <= wg <= 1.05 * sc.FP32_REF_ERROR_GRAD
    ef = eg = 0.0
    for which in sc.E2E_NETS:
        r64, r32, cf, Aw, Ab = e2e_solved(which)
        ef = max(ef, float(np.abs(r64[2] - r32[2]).max()))
        for a, b, A in list(zip(r64[0], r32[0], Aw)) + list(zip(r64[1], r32[1], Ab)):
            assert np.all(np.abs(a) <= A * (1 + 1e-9) + 1e-300)
            assert np.all(np.abs(a - b) <= sc.TOL_E2E_G * A)
            eg = max(eg, float((np.abs(a - b)[A > 0] / A[A > 0]).max()))
    print(f"end to end: frame {ef:.3e} (recorded {sc.FP32_REF_ERROR_E2E_FRAME:.3e}, TOL {sc.TOL_E2E_F:.3e}); "
          f"grad_w / grad_b {eg:.3e} (recorded {sc.FP32_REF_ERROR_E2E_GRAD:.3e}, TOL {sc.TOL_E2E_G:.3e})")
    assert ef <= sc.TOL_E2E_F
    assert 0.5 * sc.FP32_REF_ERROR_E2E_FRAME <= ef <= 1.05 * sc.FP32_REF_ERROR_E2E_FRAME
    assert 0.5 * sc.FP32_REF_ERROR_E2E_GRAD <= eg <= 1.05 * sc.FP32_REF_ERROR_E2E_GRAD
    assert sc.TOL_F == min(8.0 * sc.FP32_REF_ERROR_FRAME, 1e-5) and sc.TOL_G == min(8.0 * sc.FP32_REF_ERROR_GRAD, 1e-3)
    assert sc.TOL_E2E_F == min(8.0 * sc.FP32_REF_ERROR_E2E_FRAME, 1e-5) and sc.TOL_E2E_G == min(8.0 * sc.FP32_REF_ERROR_E2E_GRAD, 1e-3)


def test_fit_reference_converges():
    """The fp64 loop's loss falls to at most half its start; its history is the one recorded for the GPU test, and the same
    loop in float32 deviates from it by what the cases file records (relative to the largest loss: the rule of the training
    loop's trajectory test)."""
    views, teacher, start = sc.fit_data()
    net = ("siren", sc.FIT_CONFIG["W0"])
    h64 = ref.fit_loop(sc.FIT_CASES, views, teacher, start, net, sc.FIT_STEPS, sc.FIT_CONFIG["LR"], "float64")
    h32 = ref.fit_loop(sc.FIT_CASES, views, teacher, start, net, sc.FIT_STEPS, sc.FIT_CONFIG["LR"], "float32")
    dev = loop.loss_deviation(h32, np.asarray(h64))
    print("fit history fp64:", ", ".join(f"{x:.9e}" for x in h64))
    print(f"fp32 loop deviation {dev:.3e} (recorded {sc.FIT_FP32_DEVIATION:.3e})")
    assert h64[-1] <= 0.5 * h64[0]
    assert len(sc.FIT_HISTORY_FP64) == sc.FIT_STEPS and np.allclose(h64, sc.FIT_HISTORY_FP64, rtol=1e-8, atol=0)
    assert 0.5 * sc.FIT_FP32_DEVIATION <= dev <= 1.05 * sc.FIT_FP32_DEVIATION


# --- the ABI's refusals: every check happens before any HIP call, so they are testable without a device --------------------
def _call(entry, p, ext=None, vol=(0x1000, None, None, None), labels=None, logits=0x1000, classes=4, offsets=0x1000, frame=0x1000,
          pitch=None, dlogits=0x1000, null_params=False, null_vol=False):
    P = params.brats_params(p)
    E = params.render_ext(ext) if ext is not None else None
    vp = (C.c_void_p * 4)(*vol)
    head = (None if null_params else C.byref(P), C.byref(E) if E is not None else None, None if null_vol else vp, labels, logits,
            classes, offsets, frame, int(P.imageSize[0]) if pitch is None else pitch)
    if entry == "forward":
        return int(_lib.lib().mrirt_render_brats_soft(*head, None, None))
    return int(_lib.lib().mrirt_render_brats_soft_backward(*head, dlogits, None))


@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_abi_symbols_and_refusals(entry):
    for sym in ("mrirt_render_brats_soft", "mrirt_render_brats_soft_backward"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), sym)
    assert _lib.lib().mrirt_abi_version() == 4
    p = dict(sc.BY_NAME["c4_random"]["params"])
    call = functools.partial(_call, entry)
    NULL, DIMS, LAYOUT, ARG = -1, -2, -3, -5
    assert call(p, null_params=True) == NULL
    assert call(p, null_vol=True) == NULL
    assert call(p, logits=None) == NULL
    assert call(p, offsets=None) == NULL
    assert call(p, frame=None) == NULL                                           # out_rgba / grad_rgba
    if entry == "backward":
        assert call(p, dlogits=None) == NULL
    assert call(p, vol=(None, None, None, None)) == NULL                         # an enabled modality without a grid
    assert call(dict(p, showSeg=1)) == NULL                                      # the ground-truth overlay without its grid
    assert call(dict(p, dims=[13, 1, 7])) == DIMS
    assert call(dict(p, stepSize=0.0)) == ARG and call(dict(p, stepSize=float("nan"))) == ARG
    assert call(p, pitch=int(p["imageSize"][0]) - 1) == ARG
    for lay in ("brick", "vg", "quad", "vga", "mod4"):
        assert call(p, ext=dict(layout=lay)) == LAYOUT, lay
    for lay in ("brick", "labcell"):
        assert call(p, ext=dict(labelLayout=lay)) == LAYOUT, lay
    assert call(p, ext=dict(shadeMode=1)) == ARG
    assert call(p, ext=dict(tileSize=16, tileRank=0, tileWorld=2)) == ARG
    assert call(p, ext=dict(outFormat="rgba16f")) == ARG
    assert call(p, ext=dict(math="fast")) == ARG
    assert call(p, classes=0) == ARG and call(p, classes=17) == ARG
    for k in range(1, 8):
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            lut = np.array(sc.LUT)
            lut[k, 3] = bad
            assert call(dict(p, lutColorAlpha=lut)) == ARG, (k, bad)
