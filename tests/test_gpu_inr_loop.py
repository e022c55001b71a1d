"""The INR training loop on the GPU (csrc/inr_optim.hip) against the NumPy restatements of inr_loop_ref.py.

  sampler      coords, feats, labels EQUAL the restatement, for every cache / batch size / batch index / seed of inr_loop_cases.py
  adamw        integer gradients: the norm is exact and p, mu, nu EQUAL the float32 restatement; float gradients: the norm within
               the derived bound, the update bit for bit given the device's clip factor; inf poisons, it does not fault
  run          mrirt_inr_train_run EQUALS the composition of the separate calls (micro-batch 300, and 16385 with its 512-point
               slabs), and a run continued at first_step = 3
  trajectory   8 steps against the fp64 CPU loop on the same batches, within the tolerance measured from fp32 on the CPU
  train_inr    40 steps end to end, checkpoint / resume bit for bit, the loss falls
  operators    torch.ops.mrirt.* and torch.ops.mrirt_native.* give the ctypes path's bits
"""
import math

import numpy as np
import pytest
import torch

import inr_loop_cases as cases
import inr_loop_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def inr():
    import mrirt
    assert torch.cuda.is_available()
    return mrirt.inr


@pytest.fixture(scope="module")
def caches(inr):
    return {name: inr.VoxelCache(cases.cache_cases(name)) for name in cases.SAMPLER_CACHES + ["run"]}


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("name", cases.SAMPLER_CACHES)
def test_sampler_bit_for_bit(inr, caches, name):
    cache, cs = caches[name], cases.cache_cases(name)
    ncases, M, hwd = cases.cache_shape(name)
    assert (cache.n_cases, cache.n_modalities, tuple(cache.vol_shape)) == (ncases, M, hwd)
    for seed in cases.SEEDS:
        for b in cases.BATCH_INDICES:
            for n in cases.BATCH_SIZES:
                coords, feats, labels = cache.sample(seed, b, n)
                want = ref.sample(cs, seed, b, n)
                assert coords.dtype == torch.float32 and feats.dtype == torch.float32 and labels.dtype == torch.int32
                assert tuple(feats.shape) == (n, M)
                assert _same(_np(coords), want[0]), (seed, b, n)
                assert _same(_np(feats), want[1]), (seed, b, n)
                assert _same(_np(labels), want[2]), (seed, b, n)
    a, b2, other = cache.sample(7, 1, 4097), cache.sample(7, 1, 4097), cache.sample(7, 2, 4097)
    assert all(_same(_np(x), _np(y)) for x, y in zip(a, b2))                  # two calls give the same bits
    if name != "tiny":
        assert not _same(_np(a[0]), _np(other[0]))                            # another batch index gives other points
    # the reference's method on the same voxels
    ci, x, y, z = ref.draw(7, 1, 200, ncases, hwd)
    mods, seg = cache.sample_voxels(ci, x, y, z)
    assert _same(_np(mods), _np(a[1])[:200]) and _same(_np(seg).astype(np.int32), _np(a[2])[:200]) and seg.dtype == torch.int16


def _state(inr, c, nw, nb, misalign):
    """An AdamWState over copies of the case's arrays; ``misalign`` puts every array 4 bytes off a 16-byte boundary."""
    def dev(a):
        if not misalign:
            return torch.from_numpy(a.copy()).to(DEV)
        buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
        buf[1:].copy_(torch.from_numpy(a))
        return buf[1:]
    part = lambda k: (dev(c[k][:nw]), dev(c[k][nw:]))
    (w, b), (mw, mb), (vw, vb), (gw, gb) = part("p"), part("mu"), part("nu"), part("g")
    return inr.AdamWState([1, 1], w, b, mw, mb, vw, vb, 0), gw, gb


def _check_update(inr, c, nw, nb, t, clip, gscale, lr, misalign, want_norm=None):
    st, gw, gb = _state(inr, c, nw, nb, misalign)
    assert (st.w.data_ptr() % 16 != 0) == misalign
    st.step = t
    gn = _np(inr.adamw_step(st, gw, gb, lr, gscale=gscale, clip_norm=clip))
    assert st.step == t + 1
    if want_norm is not None:
        assert gn[0] == want_norm, (gn[0], want_norm)
        assert np.float32(gn[1]) == ref.clip_factor(want_norm, float(np.float32(clip)))
    s = np.float32(gn[1])
    assert float(s) == gn[1]
    p, mu, nu = ref.adamw_update(c["p"], c["mu"], c["nu"], c["g"], s, lr, t, gscale)
    got = [np.concatenate([_np(a), _np(b)]) for a, b in ((st.w, st.b), (st.mu_w, st.mu_b), (st.nu_w, st.nu_b))]
    for what, g, r in zip(("p", "mu", "nu"), got, (p, mu, nu)):
        bad = np.flatnonzero(~((g == r) | (np.isnan(g) & np.isnan(r))))
        assert bad.size == 0, (what, bad[:8], g[bad[:8]], r[bad[:8]])
    return gn, got


@pytest.mark.parametrize("t", cases.ADAMW_STEPS)
@pytest.mark.parametrize("n", cases.ADAMW_SIZES)
def test_adamw_integer_gradients_exact(inr, n, t):
    c = cases.adamw_case(n)
    nw, nb = cases.adamw_split(n)
    gscale = 0.5                                          # exact: the squares stay integers / 4
    norm = ref.gnorm(c["g"][:nw], c["g"][nw:], gscale)
    assert norm == math.sqrt(float((c["g"].astype(np.float64) ** 2).sum()) / 4.0) and norm > 0
    for clip in (2.0 * norm, 0.5 * norm, 0.0, float("inf")):          # below the clip, above it, clipping off (two spellings)
        for misalign in (False, True):
            gn, _ = _check_update(inr, c, nw, nb, t, float(np.float32(clip)), gscale, 3e-3, misalign, want_norm=norm)
            if clip == 0.5 * norm:
                assert gn[1] < 1.0
            else:
                assert gn[1] == 1.0


def test_adamw_float_gradients(inr):
    n = cases.ADAMW_FLOAT_N
    c = cases.adamw_case(n, integer=False)
    nw, nb = cases.adamw_split(n)
    want = ref.gnorm(c["g"][:nw], c["g"][nw:], 1.0)
    for clip in (0.5 * want, 4.0 * want):
        gn, got = _check_update(inr, c, nw, nb, 17, float(np.float32(clip)), 1.0, 1e-3, False)
        err, bound = abs(gn[0] - want), 2.0 ** -53 * n * want
        print(f"gnorm {gn[0]!r} reference {want!r}: |difference| {err:.3g} (bound {bound:.3g})")
        assert err <= bound
        s_ref = float(ref.clip_factor(want, float(np.float32(clip))))
        assert abs(gn[1] - s_ref) <= 2.0 ** -23 * s_ref
        _, again = _check_update(inr, c, nw, nb, 17, float(np.float32(clip)), 1.0, 1e-3, False)
        assert all(_same(a, b) for a, b in zip(got, again))                   # two calls on copies: the same bits
    bad = dict(c, g=c["g"].copy())
    bad["g"][12345] = np.inf
    st, gw, gb = _state(inr, bad, nw, nb, False)
    gn = _np(inr.adamw_step(st, gw, gb, 1e-3, clip_norm=1.0))
    torch.cuda.synchronize()
    assert np.isinf(gn[0]) and np.isnan(gn[1])
    assert np.isnan(_np(st.w)).all() and np.isnan(_np(st.b)).all()            # the stated behaviour: the step is poisoned visibly


def _desc(inr):
    net = cases.RUN_NET
    dims = [3 + 6 * net["K"] + net["M"]] + [net["hidden"]] * net["hidden_layers"] + [net["classes"]]
    return inr.train_desc(dims, net["K"], net["M"]), dims


def _cfg(inr, c):
    return inr.train_cfg(c["micro"], c["accum"], c["seed"], c["cw"], c["dw"], c["peak"], c["end"], c["warmup"], c["decay_steps"], c["clip"])


def _composition(inr, cache, desc, c, st, steps):
    """The separate calls of one run, in Python: what mrirt_inr_train_run must reproduce bit for bit."""
    n, nc = c["micro"], c["classes"]
    scratch = inr.train_scratch(desc, n, st.w.device)
    gw, gb = torch.empty_like(st.w), torch.empty_like(st.b)
    hist = np.zeros((steps, c["accum"], 1 + 2 * nc), np.float32)
    for k in range(steps):
        t = st.step
        for a in range(c["accum"]):
            coords, feats, labels = cache.sample(c["seed"], t * c["accum"] + a, n)
            logits = inr.forward_f32(desc, st.w, st.b, coords, feats, n, scratch)
            loss, aux, dl = inr.loss_and_dlogits(logits, labels, c["cw"], c["dw"], scratch)
            inr.backward_f32(desc, st.w, n, dl, scratch, gw, gb, accumulate=a > 0)
            hist[k, a, 0], hist[k, a, 1:] = float(loss), _np(aux).reshape(-1)
        lr = inr.lr_schedule(c["peak"], c["end"], c["warmup"], c["decay_steps"], t)
        inr.adamw_step(st, gw, gb, lr, gscale=float(np.float32(1.0) / np.float32(c["accum"])), clip_norm=c["clip"])
    return hist


def _bits(st):
    return [_np(getattr(st, k)).copy() for k in ("w", "b", "mu_w", "mu_b", "nu_w", "nu_b")]


@pytest.mark.parametrize("accum", [2, 3])
def test_run_equals_composition(inr, caches, accum):
    cache, c = caches["run"], cases.run_cfg(accum)
    desc, dims = _desc(inr)
    a, b = inr.AdamWState.from_params(cases.run_layers()), inr.AdamWState.from_params(cases.run_layers())
    want_hist = _composition(inr, cache, desc, c, a, 3)
    hist = _np(inr.train_run(desc, cache, _cfg(inr, c), b, 3))
    assert b.step == 3 and hist.shape == (3, accum, 1 + 2 * c["classes"])
    assert _same(hist, want_hist)
    for what, x, y in zip(("w", "b", "mu_w", "mu_b", "nu_w", "nu_b"), _bits(b), _bits(a)):
        assert _same(x, y), what
    assert np.isfinite(hist).all() and not _same(_bits(b)[0], ref.flat(cases.run_layers())[0])
    # a second run started at first_step = 3 == steps 3..5 of one 6-step run
    more = _np(inr.train_run(desc, cache, _cfg(inr, c), b, 3))
    whole = inr.AdamWState.from_params(cases.run_layers())
    hist6 = _np(inr.train_run(desc, cache, _cfg(inr, c), whole, 6))
    assert b.step == whole.step == 6
    assert _same(hist6[:3], hist) and _same(hist6[3:], more)
    for what, x, y in zip(("w", "b", "mu_w", "mu_b", "nu_w", "nu_b"), _bits(b), _bits(whole)):
        assert _same(x, y), what


def test_run_equals_composition_at_long_slabs(inr, caches):
    """The assertion of test_run_equals_composition at a micro-batch that takes 512-point slabs: 16385 points, accum 2, two
    optimiser steps."""
    cache, c = caches["run"], cases.run_cfg(2, micro=cases.RUN_LONG_MICRO)
    assert c["micro"] == 16385
    desc, dims = _desc(inr)
    a, b = inr.AdamWState.from_params(cases.run_layers()), inr.AdamWState.from_params(cases.run_layers())
    want_hist = _composition(inr, cache, desc, c, a, 2)
    hist = _np(inr.train_run(desc, cache, _cfg(inr, c), b, 2))
    assert a.step == b.step == 2 and hist.shape == (2, 2, 1 + 2 * c["classes"])
    assert _same(hist, want_hist) and np.isfinite(hist).all()
    for what, x, y in zip(("w", "b", "mu_w", "mu_b", "nu_w", "nu_b"), _bits(b), _bits(a)):
        assert _same(x, y), what
    assert not _same(_bits(b)[0], ref.flat(cases.run_layers())[0])


def test_trajectory_against_fp64(inr, caches):
    """Deviations on an MI355X: see the figures this test prints; the tolerances are inr_loop_cases.TRAJ_TOL."""
    tc = cases.traj_case()
    want = ref.train(tc["layers"], tc["cases"], tc["cfg"], cases.TRAJ_STEPS, "float64")
    desc, dims = _desc(inr)
    st = inr.AdamWState.from_params(tc["layers"])
    hist = _np(inr.train_run(desc, caches["run"], _cfg(inr, tc["cfg"]), st, cases.TRAJ_STEPS))
    got = dict(w=_np(st.w), b=_np(st.b), dims=dims)
    figures = []
    for key in ("w", "b"):
        for layer, (g, r) in enumerate(zip(ref.unflat_key(got, key), ref.unflat_key(want, key))):
            figures.append((f"layer {layer} {key}", float(np.abs(g - r).max() / np.abs(r).max()), cases.TRAJ_TOL["params"]))
    figures.append(("losses", ref.loss_deviation(hist[:, :, 0], want["losses"]), cases.TRAJ_TOL["losses"]))
    for what, err, tol in figures:
        print(f"{what}: deviation {err:.3g} (tolerance {tol:.3g})")
    bad = [f for f in figures if not f[1] <= f[2]]
    assert not bad, bad


def test_train_inr_end_to_end(inr, tmp_path):
    cfg, cs = cases.E2E_CONFIG, cases.e2e_cases()
    cache = inr.VoxelCache(cs)
    logged = []
    params, state = inr.train_inr(cfg, cache, save_path=tmp_path / "a", log=lambda step, m: logged.append((step, m["train/loss"])))
    loss = np.asarray(state["loss_history"])
    assert loss.shape == (40,) and np.isfinite(loss).all()
    assert len(state["dice_history"]) == 4 and all(len(h) == 40 for h in state["dice_history"] + state["ce_history"])
    assert [s for s, _ in logged] == list(range(1, 41)) and [v for _, v in logged] == list(loss)
    first, last = loss[:5].mean(), loss[-5:].mean()
    print(f"mean of the first 5 losses {first:.4f}, of the last 5 {last:.4f} (the fp64 CPU reference falls by {cases.E2E_SPARE} x)")
    assert last < first
    assert [p["W"].shape for p in params] == [p["W"].shape for p in cases.e2e_init()]
    # the run starts from init_mlp(RNG_SEED, ...)
    assert all(_same(a["W"], b["W"]) and _same(a["b"], b["b"]) for a, b in zip(inr.init_mlp(cfg["RNG_SEED"], 19, cfg["HIDDEN_DIMS"], 4), cases.e2e_init()))
    # a checkpoint written at step 20 and resumed gives the bits of the uninterrupted run
    ck = tmp_path / "a" / "checkpoint_step000020.npz"
    assert ck.is_file() and (tmp_path / "a" / "checkpoint_step000040.npz").is_file()
    with np.load(ck) as z:
        assert sorted(z.files) == sorted([f"W_{i}" for i in range(3)] + [f"b_{i}" for i in range(3)])
    p2, s2 = inr.train_inr(cfg, cache, resume_from=ck)
    assert s2["opt"].step == 40 and len(s2["loss_history"]) == 20
    assert all(_same(a["W"], b["W"]) and _same(a["b"], b["b"]) for a, b in zip(params, p2))
    assert s2["loss_history"] == state["loss_history"][20:]
    # nothing is written without a save path
    assert not list(tmp_path.glob("*.npz"))
    # the reference's W_i / b_i file (no optimiser state beside it) round-trips through resume_from
    plain = tmp_path / "plain.npz"
    np.savez_compressed(plain, **{f"{k}_{i}": p[k] for i, p in enumerate(params) for k in ("W", "b")})
    short = dict(cfg, TRAIN_STEPS=6, WARMUP_STEPS=1)
    p3, s3 = inr.train_inr(short, cache, resume_from=plain)
    p4, _ = inr.train_inr(short, cache, params=params)
    assert s3["opt"].step == 6
    assert all(_same(a["W"], b["W"]) and _same(a["b"], b["b"]) for a, b in zip(p3, p4))
    # the trained network goes on to the inference path
    pred, seg = inr.predict_volume(params, cs[0], cfg["FOURIER_FREQS"])
    assert tuple(pred.shape) == (16, 16, 16)


def test_torch_operators_match_the_ctypes_path(inr, caches):
    import mrirt
    cache = caches["three"]
    n, seed, b = 1000, cases.SEEDS[1], cases.BATCH_INDICES[2]
    want = [_np(x) for x in cache.sample(seed, b, n)]
    c = cases.adamw_case(257)
    nw, nb = cases.adamw_split(257)
    st, gw, gb = _state(inr, c, nw, nb, False)
    orig = [x.clone() for x in (st.w, st.b, gw, gb, st.mu_w, st.mu_b, st.nu_w, st.nu_b)]
    st.step = 5
    gn = _np(inr.adamw_step(st, gw, gb, 2e-3, gscale=0.5, clip_norm=0.75))
    signed = lambda v: v - 2 ** 64 if v >= 2 ** 63 else v
    for ops in (torch.ops.mrirt, mrirt.torch_ops.load_native()):
        got = ops.inr_sample_batch(cache.mods_table, cache.seg_table, 4, 17, 9, 33, signed(seed), signed(b), n)
        assert all(_same(_np(x), y) for x, y in zip(got, want))
        out = ops.inr_adamw_step(*orig, 2e-3, inr.ADAMW_B1, inr.ADAMW_B2, inr.ADAMW_EPS, inr.ADAMW_WEIGHT_DECAY, 0.75, 5, 0.5)
        assert len(out) == 7
        for x, y in zip(out, (st.w, st.b, st.mu_w, st.mu_b, st.nu_w, st.nu_b)):
            assert _same(_np(x), _np(y))
        assert _same(_np(out[6]), gn)
        assert _same(_np(orig[0]), c["p"][:nw])                               # the operator does not change its arguments
