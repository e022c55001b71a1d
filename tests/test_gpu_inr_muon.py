"""Muon on the GPU (csrc/inr_muon.hip) against the NumPy restatement of inr_muon_ref.py.

  orthogonalize, exact      scaled selection matrices: every sum has one term, the output EQUALS the fp32 restatement (whole
                            networks per call, ns_steps 1 and 5, all-zero rows, an all-zero matrix, guarded scratch, one NaN)
  orthogonalize, tolerance  Gaussian matrices at three scales within 8 x the fp32-CPU deviation recorded in inr_muon_cases.py
  step                      W, mu_w EQUAL the restated element-wise parts around the GPU's own orthogonalize; biases, mu_b, nu_b
                            and gnorm EQUAL mrirt_inr_adamw_step's; nu_w untouched; the whole step within tolerance of fp64
  run                       mrirt_inr_train_run_muon EQUALS the separate calls (ReLU and SIREN, accum 1 and 3); train_inr /
                            train_siren with OPTIMIZER_CHOICE = "muon": checkpoint + resume, the loss falls; the default
                            configuration still is AdamW's run
"""
import ctypes as C

import numpy as np
import pytest
import torch

import inr_loop_cases as lc
import inr_loop_ref as lr_ref
import inr_muon_cases as cases
import inr_muon_ref as ref
import inr_siren_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def inr():
    import mrirt
    assert torch.cuda.is_available()
    return mrirt.inr


def _np(t):
    return t.cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _mismatch(got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return bad[:8], got[bad[:8]], want[bad[:8]]


# ---- orthogonalize ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns_steps", cases.EXACT_NS_STEPS)
@pytest.mark.parametrize("i", range(len(cases.EXACT)), ids=[cases.exact_id(c) for c in cases.EXACT])
def test_orthogonalize_exact(inr, i, ns_steps):
    dims, m = cases.EXACT[i]["dims"], cases.exact_case(i)
    h = ref.hp(ns_steps=ns_steps)
    want = ref.ns_flat(m, dims, h)
    got = _np(inr.muon_orthogonalize(dims, _dev(m), inr.muon_hp(ns_steps=ns_steps)))
    assert got.dtype == np.float32 and got.shape == want.shape
    assert _same(got, want), _mismatch(got, want)
    assert np.isfinite(got).all()
    for l, (g, M) in enumerate(zip(ref.split(got, dims), ref.split(m, dims))):
        if not M.any():
            assert not g.any(), l                         # an all-zero matrix: all-zero output, no NaN
        else:
            assert g.any(), l


def test_orthogonalize_exact_on_guarded_scratch(inr):
    import mrirt
    dims, m = cases.EXACT[cases.GUARD_CASE]["dims"], cases.exact_case(cases.GUARD_CASE)
    desc = inr.train_desc(dims)
    nbytes = int(mrirt._lib.lib().mrirt_muon_scratch_bytes(C.byref(desc)))
    assert nbytes > 0 and nbytes % 256 == 0
    guard = 4096
    buf = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    got = _np(inr.muon_orthogonalize(dims, _dev(m), scratch=buf[guard:guard + nbytes]))
    assert _same(got, ref.ns_flat(m, dims))
    host = _np(buf)
    assert (host[:guard] == 0xA5).all() and (host[guard + nbytes:] == 0xA5).all()


def test_orthogonalize_one_nan_poisons_its_layer_only(inr):
    dims, m = cases.EXACT[cases.NAN_CASE]["dims"], cases.exact_case(cases.NAN_CASE)
    clean = _np(inr.muon_orthogonalize(dims, _dev(m)))
    bad = m.copy()
    offs = np.cumsum([0] + [a * b for a, b in zip(dims[:-1], dims[1:])])
    bad[offs[cases.NAN_LAYER] + 5] = np.nan
    got = _np(inr.muon_orthogonalize(dims, _dev(bad)))
    for l, (g, c) in enumerate(zip(ref.split(got, dims), ref.split(clean, dims))):
        if l == cases.NAN_LAYER:
            assert np.isnan(g).all()
        else:
            assert _same(g, c), l
    assert _same(got, ref.ns_flat(bad, dims))


@pytest.mark.parametrize("name", list(cases.TOL_NETS))
def test_orthogonalize_within_tolerance(inr, name):
    """Deviations on an MI355X: see the figures this test prints; the bound is 8 x inr_muon_cases.NS_DEVIATION."""
    dims, tol = cases.TOL_NETS[name], 8.0 * cases.NS_DEVIATION[name]
    worst = 0.0
    for scale in cases.TOL_SCALES:
        m = cases.tol_case(name, scale)
        got = _np(inr.muon_orthogonalize(dims, _dev(m)))
        dev = cases.layer_deviation(got, ref.ns_flat(m, dims, None, np.float64), dims)
        print(f"{name} scale {scale:g}: deviation per layer {['%.3g' % d for d in dev]} (tolerance {tol:.3g})")
        worst = max(worst, max(dev))
        again = _np(inr.muon_orthogonalize(dims, _dev(m)))
        assert _same(got, again)                          # two calls give the same bits
    assert worst <= tol, (worst, tol)


# ---- step ------------------------------------------------------------------------------------------------------------------------

SENTINEL = -12345.5


def _state(inr, c):
    st = inr.AdamWState(list(c["dims"]), _dev(c["w"]), _dev(c["b"]), _dev(c["mu_w"]), _dev(c["mu_b"]),
                        torch.full((c["w"].size,), SENTINEL, dtype=torch.float32, device=DEV), _dev(c["nu_b"]), 0)
    return st, _dev(c["gw"]), _dev(c["gb"])


@pytest.mark.parametrize("v", cases.STEP_VARIANTS, ids=lambda v: f"nesterov{int(v['nesterov'])}-clip{v['clip']}-t{v['t']}-wd{v['wd']}")
def test_step(inr, v):
    c, dims = cases.step_case(), cases.STEP_NET
    norm = lr_ref.gnorm(c["gw"], c["gb"], cases.STEP_GSCALE)
    clip = float(np.float32(v["clip"] * norm))
    hp = inr.muon_hp(nesterov=v["nesterov"], weight_decay=v["wd"])
    h = ref.hp(nesterov=v["nesterov"], weight_decay=v["wd"])

    def run():
        st, gw, gb = _state(inr, c)
        st.step = v["t"]
        gn = _np(inr.muon_step(st, gw, gb, cases.STEP_LR, gscale=cases.STEP_GSCALE, clip_norm=clip, hp=hp))
        assert st.step == v["t"] + 1
        return st, gn
    st, gn = run()
    # the clip factor, the biases and their moments: mrirt_inr_adamw_step's, with the bias half's hyper-parameters
    sa, gw, gb = _state(inr, c)
    sa.nu_w.zero_()
    sa.step = v["t"]
    gn_a = _np(inr.adamw_step(sa, gw, gb, cases.STEP_LR, gscale=cases.STEP_GSCALE, clip_norm=clip, b1=inr.MUON_BIAS_B1, b2=inr.MUON_BIAS_B2,
                              eps=inr.MUON_BIAS_EPS, weight_decay=inr.MUON_BIAS_WEIGHT_DECAY))
    assert _same(gn, gn_a), (gn, gn_a)
    assert (gn[1] < 1.0) == (0.0 < v["clip"] < 1.0)
    for k in ("b", "mu_b", "nu_b"):
        assert _same(_np(getattr(st, k)), _np(getattr(sa, k))), k
    assert (_np(st.nu_w) == SENTINEL).all()               # no second moment of the weights: not read, not written
    # the matrices: the restated element-wise parts around the GPU's own orthogonalisation
    s = np.float32(gn[1])
    gpu_ns = lambda mhat: _np(inr.muon_orthogonalize(dims, _dev(mhat), hp))
    want = ref.step(c["w"], c["b"], c["gw"], c["gb"], c["mu_w"], c["mu_b"], c["nu_b"], dims, s, cases.STEP_LR, v["t"], cases.STEP_GSCALE, h,
                    np.float32, ns_of=gpu_ns)
    for k in ("w", "mu_w"):
        got = _np(getattr(st, k))
        assert _same(got, want[k]), (k, _mismatch(got, want[k]))
    assert not _same(_np(st.w), c["w"])
    # two calls give the same bits
    st2, gn2 = run()
    assert _same(gn, gn2) and all(_same(_np(getattr(st, k)), _np(getattr(st2, k))) for k in ("w", "b", "mu_w", "mu_b", "nu_b"))
    # the whole step against fp64
    r64, _ = cases.step_reference(v, np.float64)
    for k in ("w", "mu_w"):
        dev, tol = cases.layer_deviation(_np(getattr(st, k)), r64[k], dims), 8.0 * cases.STEP_DEVIATION[k]
        print(f"{k}: deviation per layer {['%.3g' % d for d in dev]} (tolerance {tol:.3g})")
        assert max(dev) <= tol, (k, dev, tol)


# ---- run -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def run_cache(inr):
    return inr.VoxelCache(lc.cache_cases("run"))


def _family(inr, family):
    if family == "relu":
        net = lc.RUN_NET
        dims = [3 + 6 * net["K"] + net["M"]] + [net["hidden"]] * net["hidden_layers"] + [net["classes"]]
        return inr.train_desc(dims, net["K"], net["M"]), lc.run_layers(), inr.train_scratch, inr.forward_f32, inr.backward_f32
    dims = sc.run_dims()
    return inr.siren_train_desc(dims, sc.RUN_NET["M"], sc.W0), sc.run_layers(), inr.siren_train_scratch, inr.siren_forward_f32, inr.siren_backward_f32


def _cfg(inr, c):
    return inr.train_cfg(c["micro"], c["accum"], c["seed"], c["cw"], c["dw"], c["peak"], c["end"], c["warmup"], c["decay_steps"], c["clip"],
                         b1=inr.MUON_BIAS_B1, b2=inr.MUON_BIAS_B2, eps=inr.MUON_BIAS_EPS, weight_decay=inr.MUON_BIAS_WEIGHT_DECAY)


def _bits(st):
    return [_np(getattr(st, k)).copy() for k in ("w", "b", "mu_w", "mu_b", "nu_w", "nu_b")]


@pytest.mark.parametrize("accum", [1, 3])
@pytest.mark.parametrize("family", ["relu", "siren"])
def test_run_equals_separate_calls(inr, run_cache, family, accum):
    desc, layers, make_scratch, forward, backward = _family(inr, family)
    c = lc.run_cfg(accum)
    n, nc, steps = c["micro"], c["classes"], 3
    a, b = inr.AdamWState.from_params(layers), inr.AdamWState.from_params(layers)
    scratch = make_scratch(desc, n, a.w.device)
    gw, gb = torch.empty_like(a.w), torch.empty_like(a.b)
    want_hist = np.zeros((steps, accum, 1 + 2 * nc), np.float32)
    for k in range(steps):
        t = a.step
        for j in range(accum):
            coords, feats, labels = run_cache.sample(c["seed"], t * accum + j, n)
            logits = forward(desc, a.w, a.b, coords, feats, n, scratch)
            loss, aux, dl = inr.loss_and_dlogits(logits, labels, c["cw"], c["dw"], scratch)
            backward(desc, a.w, n, dl, scratch, gw, gb, accumulate=j > 0)
            want_hist[k, j, 0], want_hist[k, j, 1:] = float(loss), _np(aux).reshape(-1)
        rate = inr.lr_schedule(c["peak"], c["end"], c["warmup"], c["decay_steps"], t)
        inr.muon_step(a, gw, gb, rate, gscale=float(np.float32(1.0) / np.float32(accum)), clip_norm=c["clip"])
    hist = _np(inr.train_run(desc, run_cache, _cfg(inr, c), b, steps, muon=inr.muon_hp()))
    assert a.step == b.step == steps
    assert _same(hist, want_hist) and np.isfinite(hist).all()
    for what, x, y in zip(("w", "b", "mu_w", "mu_b", "nu_w", "nu_b"), _bits(b), _bits(a)):
        assert _same(x, y), what
    assert not _same(_bits(b)[0], lr_ref.flat(layers)[0]) and not _bits(b)[4].any()
    # another optimiser: AdamW's run from the same start ends elsewhere
    other = inr.AdamWState.from_params(layers)
    inr.train_run(desc, run_cache, _cfg(inr, c), other, steps)
    assert not _same(_bits(other)[0], _bits(b)[0])


@pytest.mark.parametrize("family", ["relu", "siren"])
def test_train_with_muon_end_to_end(inr, tmp_path, family):
    cfg = cases.E2E_RELU if family == "relu" else cases.E2E_SIREN
    train = inr.train_inr if family == "relu" else inr.train_siren
    cache = inr.VoxelCache(lc.e2e_cases())
    params, state = train(cfg, cache, save_path=tmp_path / "a")
    loss = np.asarray(state["loss_history"])
    assert loss.shape == (40,) and np.isfinite(loss).all()
    first, last = loss[:5].mean(), loss[-5:].mean()
    need = cases.E2E_FALL[family] / 1.5
    print(f"mean of the first 5 losses {first:.4f}, of the last 5 {last:.4f}: factor {first / last:.3f} (the fp64 CPU Muon loop: "
          f"{cases.E2E_FALL[family]}; needed {need:.3f})")
    assert first / last >= need
    ck = tmp_path / "a" / "checkpoint_step000020.npz"
    with np.load(ck.with_name(ck.stem + "_opt.npz")) as z:
        assert str(z["optimizer"]) == "muon" and int(z["step"]) == 20
    p2, s2 = train(cfg, cache, resume_from=ck)
    assert s2["opt"].step == 40 and s2["loss_history"] == state["loss_history"][20:]
    leaves = lambda p: [(q["W"], q["b"]) for q in p] if isinstance(p, list) else [(p[k]["w"], p[k]["b"]) for k in sorted(p)]
    assert all(_same(a[0], b[0]) and _same(a[1], b[1]) for a, b in zip(leaves(params), leaves(p2)))
    # the other optimiser refuses this state, and Muon refuses AdamW's
    adamw_cfg = {k: v for k, v in cfg.items() if k != "OPTIMIZER_CHOICE"}
    with pytest.raises(ValueError, match="muon"):
        train(adamw_cfg, cache, resume_from=ck)
    train(dict(adamw_cfg, TRAIN_STEPS=20), cache, save_path=tmp_path / "b")
    with pytest.raises(ValueError, match="adamw"):
        train(cfg, cache, resume_from=tmp_path / "b" / "checkpoint_step000020.npz")


def test_default_config_is_still_adamw(inr):
    """No OPTIMIZER_CHOICE, or any value but "muon": the bits of the AdamW run enqueued directly."""
    cfg = dict(lc.E2E_CONFIG, TRAIN_STEPS=6, WARMUP_STEPS=1)
    cache = inr.VoxelCache(lc.e2e_cases())
    st = inr.AdamWState.from_params(lc.e2e_init())
    desc = inr.train_desc(st.dims, cfg["FOURIER_FREQS"], 4)
    c = inr.train_cfg(cfg["MICRO_BATCH_SIZE"], 2, cfg["RNG_SEED"], cfg["CLASS_WEIGHTS"], cfg["DICE_WEIGHT"], cfg["LR"], cfg["MIN_LR"], 1, 5, cfg["CLIP_NORM"])
    hist = _np(inr.train_run(desc, cache, c, st, 6)).astype(np.float64).mean(axis=1)
    for choice in (None, "adamw", "sgd"):
        conf = dict(cfg) if choice is None else dict(cfg, OPTIMIZER_CHOICE=choice)
        params, state = inr.train_inr(conf, cache)
        assert all(_same(p["W"], q["W"]) and _same(p["b"], q["b"]) for p, q in zip(params, st.params())), choice
        assert state["loss_history"] == [float(v) for v in hist[:, 0]]
        assert _np(state["opt"].nu_w).any()
