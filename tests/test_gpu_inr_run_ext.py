"""mrirt_inr_train_run_ext on the GPU: with every member NULL / 0 the bits of mrirt_inr_train_run, mrirt_siren_train_run and
mrirt_inr_train_run_muon (weights, moments, history); with a full ext the bits of the composition of the separate calls, for
ReLU and SIREN, AdamW and Muon; and train_inr with the new config keys (checkpoint / resume, the keys in _opt.npz, and a
config without them reproducing today's run)."""
import numpy as np
import pytest
import torch

import inr_loop_cases as lc
import inr_siren_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS, ACCUM, MICRO = 3, 2, 512
EXT = dict(per_class_dice=False, focal_gamma=2.0, focal_alpha=[0.25, 1.0, 2.0], label_smoothing=0.05, edema_fp_weight=0.3, tversky_edema_alpha=0.7,
           tversky_edema_beta=0.3, tversky_edema_weight=0.4, edema_logit_reg=0.2, edema_class=2)


@pytest.fixture(scope="module")
def inr():
    import mrirt
    assert torch.cuda.is_available()
    return mrirt.inr


@pytest.fixture(scope="module")
def run_cache(inr):
    return inr.VoxelCache(lc.cache_cases("run"))


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _bits(st):
    return [_np(getattr(st, k)).copy() for k in ("w", "b", "mu_w", "mu_b", "nu_w", "nu_b")]


def _family(inr, family):
    if family == "relu":
        net = lc.RUN_NET
        dims = [3 + 6 * net["K"] + net["M"]] + [net["hidden"]] * net["hidden_layers"] + [net["classes"]]
        return inr.train_desc(dims, net["K"], net["M"]), lc.run_layers(), inr.train_scratch, inr.forward_f32, inr.backward_f32
    return (inr.siren_train_desc(sc.run_dims(), sc.RUN_NET["M"], sc.W0), sc.run_layers(), inr.siren_train_scratch, inr.siren_forward_f32,
            inr.siren_backward_f32)


def _cfg(inr, c, muon):
    half = dict(b1=inr.MUON_BIAS_B1, b2=inr.MUON_BIAS_B2, eps=inr.MUON_BIAS_EPS, weight_decay=inr.MUON_BIAS_WEIGHT_DECAY) if muon else {}
    return inr.train_cfg(c["micro"], c["accum"], c["seed"], c["cw"], c["dw"], c["peak"], c["end"], c["warmup"], c["decay_steps"], c["clip"], **half)


@pytest.mark.parametrize("muon", [False, True], ids=["adamw", "muon"])
@pytest.mark.parametrize("family", ["relu", "siren"])
def test_empty_ext_gives_the_existing_runs_bits(inr, run_cache, family, muon):
    desc, layers = _family(inr, family)[:2]
    c = lc.run_cfg(ACCUM, micro=MICRO)
    a, b = inr.AdamWState.from_params(layers), inr.AdamWState.from_params(layers)
    hp = inr.muon_hp() if muon else None
    want = _np(inr.train_run(desc, run_cache, _cfg(inr, c, muon), a, STEPS, muon=hp))       # mrirt_inr_ / mrirt_siren_train_run, _run_muon
    hist = _np(inr.train_run(desc, run_cache, _cfg(inr, c, muon), b, STEPS, ext=inr.train_ext(muon=hp)))
    assert a.step == b.step == STEPS and _same(hist, want) and np.isfinite(hist).all()
    for what, x, y in zip(("w", "b", "mu_w", "mu_b", "nu_w", "nu_b"), _bits(b), _bits(a)):
        assert _same(x, y), what


@pytest.mark.parametrize("muon", [False, True], ids=["adamw", "muon"])
@pytest.mark.parametrize("family", ["relu", "siren"])
def test_full_ext_equals_the_separate_calls(inr, run_cache, family, muon):
    desc, layers, make_scratch, forward, backward = _family(inr, family)
    c = lc.run_cfg(ACCUM, micro=MICRO)
    n, nc = c["micro"], c["classes"]
    loss_ext = inr.loss_ext(c["cw"], c["dw"], **EXT)
    nt = inr.n_tumour_of(n, 0.4)
    assert nt == 204
    a, b = inr.AdamWState.from_params(layers), inr.AdamWState.from_params(layers)
    scratch = make_scratch(desc, n, a.w.device)
    gw, gb = torch.empty_like(a.w), torch.empty_like(a.b)
    want_hist = np.zeros((STEPS, ACCUM, 1 + 2 * nc), np.float32)
    for k in range(STEPS):
        t = a.step
        for j in range(ACCUM):
            coords, feats, labels = run_cache.sample(c["seed"], t * ACCUM + j, n, n_tumour=nt)
            logits = forward(desc, a.w, a.b, coords, feats, n, scratch)
            loss, aux, dl, _ = inr.loss_and_dlogits(logits, labels, None, None, ext=loss_ext)
            backward(desc, a.w, n, dl, scratch, gw, gb, accumulate=j > 0)
            want_hist[k, j, 0], want_hist[k, j, 1:] = float(loss), _np(aux).reshape(-1)
        rate = inr.lr_schedule(c["peak"], c["end"], c["warmup"], c["decay_steps"], t)
        gscale = float(np.float32(1.0) / np.float32(ACCUM))
        if muon:
            inr.muon_step(a, gw, gb, rate, gscale=gscale, clip_norm=c["clip"])
        else:
            inr.adamw_step(a, gw, gb, rate, gscale=gscale, clip_norm=c["clip"])
    ext = inr.train_ext(run_cache, loss_ext, inr.muon_hp() if muon else None, nt)
    hist = _np(inr.train_run(desc, run_cache, _cfg(inr, c, muon), b, STEPS, ext=ext))
    assert a.step == b.step == STEPS and hist.shape == want_hist.shape
    assert _same(hist, want_hist) and np.isfinite(hist).all()
    for what, x, y in zip(("w", "b", "mu_w", "mu_b", "nu_w", "nu_b"), _bits(b), _bits(a)):
        assert _same(x, y), what
    # the plain loss and sampler from the same start end elsewhere
    other = inr.AdamWState.from_params(layers)
    plain = _np(inr.train_run(desc, run_cache, _cfg(inr, c, muon), other, STEPS, muon=inr.muon_hp() if muon else None))
    assert not _same(plain, hist) and not _same(_bits(other)[0], _bits(b)[0])


NEW_KEYS = dict(FOCAL_GAMMA=2.0, FOCAL_ALPHA=[0.25, 1.0, 0.5, 2.0], LABEL_SMOOTHING=0.05, PER_CLASS_DICE=False, EDEMA_FP_WEIGHT=0.3,
                TVERSKY_EDEMA_ALPHA=0.7, TVERSKY_EDEMA_BETA=0.3, TVERSKY_EDEMA_WEIGHT=0.4, EDEMA_LOGIT_REG=0.2, EDEMA_CLASS=2, TUMOR_RATIO=0.4)


def test_train_inr_with_the_new_keys(inr, tmp_path):
    cfg = dict(lc.E2E_CONFIG, TRAIN_STEPS=12, CHECKPOINT_EVERY_STEPS=6, **NEW_KEYS)
    cache = inr.VoxelCache(lc.e2e_cases())
    params, state = inr.train_inr(cfg, cache, save_path=tmp_path / "a")
    loss = np.asarray(state["loss_history"])
    assert loss.shape == (12,) and np.isfinite(loss).all()
    ck = tmp_path / "a" / "checkpoint_step000006.npz"
    with np.load(ck.with_name(ck.stem + "_opt.npz")) as z:
        assert int(z["step"]) == 6
        assert {k for k in z.files if k.startswith("ext_")} == {"ext_" + k for k in NEW_KEYS}
        assert float(z["ext_TUMOR_RATIO"]) == 0.4 and z["ext_FOCAL_ALPHA"].tolist() == NEW_KEYS["FOCAL_ALPHA"] and float(z["ext_PER_CLASS_DICE"]) == 0.0
    p2, s2 = inr.train_inr(cfg, cache, resume_from=ck)
    assert s2["opt"].step == 12 and s2["loss_history"] == state["loss_history"][6:]
    assert all(_same(a["W"], b["W"]) and _same(a["b"], b["b"]) for a, b in zip(params, p2))
    # the run is the composition: train_run with the same ext from the same start
    st = inr.AdamWState.from_params(lc.e2e_init())
    desc = inr.train_desc(st.dims, cfg["FOURIER_FREQS"], 4)
    c = inr.train_cfg(cfg["MICRO_BATCH_SIZE"], 2, cfg["RNG_SEED"], cfg["CLASS_WEIGHTS"], cfg["DICE_WEIGHT"], cfg["LR"], cfg["MIN_LR"], cfg["WARMUP_STEPS"],
                      12 - cfg["WARMUP_STEPS"], cfg["CLIP_NORM"])
    le = inr.loss_ext(cfg["CLASS_WEIGHTS"], cfg["DICE_WEIGHT"], False, 2.0, NEW_KEYS["FOCAL_ALPHA"], 0.05, 0.3, 0.7, 0.3, 0.4, 0.2, 2)
    hist = _np(inr.train_run(desc, cache, c, st, 12, ext=inr.train_ext(cache, le, None, inr.n_tumour_of(cfg["MICRO_BATCH_SIZE"], 0.4))))
    assert state["loss_history"] == [float(v) for v in hist.astype(np.float64).mean(axis=1)[:, 0]]
    assert all(_same(p["W"], q["W"]) and _same(p["b"], q["b"]) for p, q in zip(params, st.params()))
    # another loss than the plain run's
    plain, pstate = inr.train_inr({k: v for k, v in cfg.items() if k not in NEW_KEYS}, cache)
    assert pstate["loss_history"] != state["loss_history"]


def test_a_config_without_the_keys_is_the_run_without_ext(inr, tmp_path):
    cfg = dict(lc.E2E_CONFIG, TRAIN_STEPS=6, WARMUP_STEPS=1, CHECKPOINT_EVERY_STEPS=6)
    cache = inr.VoxelCache(lc.e2e_cases())
    st = inr.AdamWState.from_params(lc.e2e_init())
    desc = inr.train_desc(st.dims, cfg["FOURIER_FREQS"], 4)
    c = inr.train_cfg(cfg["MICRO_BATCH_SIZE"], 2, cfg["RNG_SEED"], cfg["CLASS_WEIGHTS"], cfg["DICE_WEIGHT"], cfg["LR"], cfg["MIN_LR"], 1, 5, cfg["CLIP_NORM"])
    hist = _np(inr.train_run(desc, cache, c, st, 6, ext=None)).astype(np.float64).mean(axis=1)
    params, state = inr.train_inr(cfg, cache, save_path=tmp_path / "a")
    assert all(_same(p["W"], q["W"]) and _same(p["b"], q["b"]) for p, q in zip(params, st.params()))
    assert state["loss_history"] == [float(v) for v in hist[:, 0]]
    with np.load(tmp_path / "a" / "checkpoint_step000006_opt.npz") as z:
        assert not [k for k in z.files if k.startswith("ext_")]
    # the keys at their neutral values go through mrirt_inr_train_run_ext and give the same bits
    neutral, nstate = inr.train_inr(dict(cfg, FOCAL_GAMMA=0.0, TUMOR_RATIO=0.0), cache)
    assert all(_same(p["W"], q["W"]) and _same(p["b"], q["b"]) for p, q in zip(neutral, params))
    assert nstate["loss_history"] == state["loss_history"]
