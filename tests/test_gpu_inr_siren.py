"""SIREN training on the GPU (mrirt_siren_*).

  exact       selection nets: logits, every dW_l and db_l EQUAL the fp32 NumPy restatement with the restated sine (a dot product
              with one non-zero term is that term exactly in the k-ordered fma chain of v_mfma_f32_16x16x4_f32), both kinds,
              w0 1 and 30, pre-activations up to 2^20, dlogits in one row at the block / slab edges, accumulation; one case on
              a scratch of exactly the stated size between guard blocks; after the forward the saved x', sines and cosines
              are read out of the scratch by the restated layout and compared at every row
  heads       HEAD_COVER: per width, heads that together put a gradient under every hidden unit
  batch       BATCH: n = 16383 .. 131073 with one non-zero dlogits row per slab, against np_step_slabs (the fixed-order sum of
              up to 64 non-zero partials), saved regions at every row; the raw C ABI between guard blocks at 16385 and 65537
  beyond      pre-activations beyond 2^20 and at 3e38 (sin = +0, cos = 1: the gradient passes through); a NaN and an inf input
  tolerance   random siren_init nets against the fp64 autograd step, |g - g_ref| <= tol x A with the recorded 8 x fp32-CPU
              tolerances of inr_siren_cases.py; two calls give the same bits
  loop        mrirt_siren_train_run EQUALS the separate calls; a continued run; train_siren end to end with checkpoint / resume
              bit for bit and the required fall of the loss; the trained dict goes on to pack_mlp / classify
"""
import ctypes as C

import numpy as np
import pytest
import torch

import inr_loop_cases as lc
import inr_loop_ref as lref
import inr_siren_cases as cases
import inr_siren_ref as sr
import inr_train_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096


@pytest.fixture(scope="module")
def inr():
    import mrirt
    assert torch.cuda.is_available()
    return mrirt.inr


def _np(t):
    return t.cpu().numpy()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _flat(layers):
    w, b = lref.flat(layers)
    return _dev(w), _dev(b)


def _bad(got, want):
    g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    at = np.flatnonzero(g != w)
    return (at.size, at[:6], g[at[:6]], w[at[:6]])


def _saved(scratch, dims, n):
    """(x', [h_l], [c_l]) read out of a step's scratch by the restated layout (inr_siren_ref.siren_layout)."""
    L = sr.siren_layout(dims, n)
    assert scratch.numel() >= L["bytes"] and scratch.dtype == torch.uint8

    def region(off, cols):
        return _np(scratch[off:off + n * cols * 4].view(torch.float32).reshape(n, cols))
    hidden = range(len(dims) - 2)
    return (region(L["offX"], dims[0]), [region(L["offH"] + l * L["act"], dims[1]) for l in hidden],
            [region(L["offC"] + l * L["act"], dims[1]) for l in hidden])


def _assert_saved(what, scratch, dims, n, ref):
    """x' == ins[0], h_l == ins[l + 1], c_l == cos[l]: every row, every column, bit for bit (NaN where the reference has one)."""
    x, hs, cs = _saved(scratch, dims, n)
    assert len(hs) == len(ref["cos"]) == len(ref["ins"]) - 1
    for name, got, want in [("x'", x, ref["ins"][0])] + [(f"h_{l}", h, ref["ins"][l + 1]) for l, h in enumerate(hs)] + \
                           [(f"c_{l}", c, ref["cos"][l]) for l, c in enumerate(cs)]:
        assert got.shape == want.shape, (name, got.shape, want.shape)
        bad = sr.bits_differ(got, want)
        assert bad.size == 0, (what, name, bad.size, bad[:6], got.reshape(-1)[bad[:6]], want.reshape(-1)[bad[:6]])
    print(f"{what}: x', {len(hs)} x (h, c) compared at {n} rows x {dims[0]} / {dims[1]} columns, bit for bit")


def _exact_desc(inr, e):
    c = e["net"]
    return inr.siren_train_desc(e["dims"], None if c["kind"] == cases.KIND_RAW_SIREN else c["ind"] - 3, c["w0"])


@pytest.mark.parametrize("i", range(len(cases.EXACT)), ids=[cases.exact_id(c) for c in cases.EXACT])
def test_exact_selection_nets(inr, i):
    e = cases.exact_case(i)
    desc, ref = _exact_desc(inr, e), e["ref"]
    w, b = _flat(e["layers"])
    scratch = inr.siren_train_scratch(desc, cases.N, DEV)
    logits = inr.siren_forward_f32(desc, w, b, _dev(e["coords"]), _dev(e["feats"]), cases.N, scratch)
    assert np.isfinite(ref["logits"]).all()
    assert _same(_np(logits), ref["logits"]), _bad(_np(logits), ref["logits"])
    _assert_saved(cases.exact_id(e["net"]), scratch, e["dims"], cases.N, ref)
    gw = _dev(e["init_w"]) if e["net"]["acc"] else None
    gb = _dev(e["init_b"]) if e["net"]["acc"] else None
    gw, gb = inr.siren_backward_f32(desc, w, cases.N, _dev(e["dlogits"]), scratch, gw, gb, accumulate=e["net"]["acc"])
    assert _same(_np(gw), ref["gw"]), _bad(_np(gw), ref["gw"])
    assert _same(_np(gb), ref["gb"]), _bad(_np(gb), ref["gb"])
    assert np.count_nonzero(ref["gw"]) > 0 and np.count_nonzero(ref["gb"]) > 0


def test_exact_scratch_between_guards(inr):
    """The step on a scratch of exactly mrirt_siren_train_scratch_bytes between two 4-KiB guard blocks: the same bits, and the
    guards untouched."""
    from mrirt import _lib
    e = cases.exact_case(cases.GUARD_CASE)
    desc, ref = _exact_desc(inr, e), e["ref"]
    nbytes = int(_lib.lib().mrirt_siren_train_scratch_bytes(C.byref(desc), cases.N))
    assert nbytes > 0 and nbytes % 256 == 0
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    scratch = buf[GUARD:GUARD + nbytes]
    assert scratch.data_ptr() % 16 == 0
    w, b = _flat(e["layers"])
    logits = inr.siren_forward_f32(desc, w, b, _dev(e["coords"]), _dev(e["feats"]), cases.N, scratch)
    gw, gb = inr.siren_backward_f32(desc, w, cases.N, _dev(e["dlogits"]), scratch)
    torch.cuda.synchronize()
    assert _same(_np(logits), ref["logits"]) and _same(_np(gw), ref["gw"]) and _same(_np(gb), ref["gb"])
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())
    with pytest.raises(Exception):                       # one byte less is refused before any launch
        inr.siren_forward_f32(desc, w, b, _dev(e["coords"]), _dev(e["feats"]), cases.N, scratch[:nbytes - 1])


def _selection_step(inr, e, n, w0, raw, what):
    """Forward, saved regions, backward of a selection-net case against its reference: everything ==.  Returns the bytes."""
    desc, ref = inr.siren_train_desc(e["dims"], None if raw else e["dims"][0] - 3, w0), e["ref"]
    w, b = _flat(e["layers"])
    scratch = inr.siren_train_scratch(desc, n, DEV)
    logits = _np(inr.siren_forward_f32(desc, w, b, _dev(e["coords"]), _dev(e["feats"]), n, scratch))
    assert np.isfinite(ref["logits"]).all() and logits.shape == (n, e["dims"][-1])
    assert _same(logits, ref["logits"]), _bad(logits, ref["logits"])
    _assert_saved(what, scratch, e["dims"], n, ref)
    acc = e["init_w"] is not None
    gw, gb = inr.siren_backward_f32(desc, w, n, _dev(e["dlogits"]), scratch, _dev(e["init_w"]), _dev(e["init_b"]), accumulate=acc)
    gw, gb = _np(gw), _np(gb)
    assert _same(gw, ref["gw"]), _bad(gw, ref["gw"])
    assert _same(gb, ref["gb"]), _bad(gb, ref["gb"])
    assert np.count_nonzero(ref["gw"]) > 0 and np.count_nonzero(ref["gb"]) > 0
    print(f"{what}: logits {n} x {e['dims'][-1]}, {gw.size} dW and {gb.size} db elements ==")
    return logits, gw, gb


@pytest.mark.parametrize("i", range(len(cases.HEAD_COVER)), ids=[cases.exact_id(c) for c in cases.HEAD_COVER])
def test_every_hidden_unit_under_a_head(inr, i):
    """Per width the heads of HEAD_COVER select every hidden unit once (test_inr_siren_ref.py): every column of the widest
    net's hidden layers carries a non-zero gradient in an exact test."""
    e = cases.head_cover_case(i)
    _selection_step(inr, e, cases.HEAD_N, e["net"]["w0"], True, cases.exact_id(e["net"]))


@pytest.mark.parametrize("i", range(len(cases.BATCH)), ids=[cases.batch_id(c) for c in cases.BATCH])
def test_batch_sweep_is_exact(inr, i):
    """Both sides of every doubling of the slab length from 256 to 4096 and the workload's width at 65537 points, one non-zero
    dlogits row in every slab: logits and the saved regions at every row, dW and db against the fixed-order sum over the slabs
    (np_step_slabs).  One case accumulates into non-zero gradients; one runs twice and demands the same bytes."""
    e = cases.batch_case(i)
    raw = e["kind"] == cases.KIND_RAW_SIREN
    first = _selection_step(inr, e, e["n"], e["w0"], raw, cases.batch_id(e["net"]))
    if cases.BATCH[i] == cases.BATCH_REPEAT:
        for a, b in zip(first, _selection_step(inr, e, e["n"], e["w0"], raw, cases.batch_id(e["net"]) + " again")):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", cases.GUARD_NS)
def test_batch_scratch_exactly_as_long_as_the_abi_asks(inr, n):
    """The step through the raw C ABI with a scratch of exactly mrirt_siren_train_scratch_bytes(desc, n) bytes between two
    4-KiB guard blocks, at n = 16385 (the slab count drops, the length doubles) and 65537: the bits of the batch sweep, the
    cosine region included, the guards and the rows behind the outputs untouched; one byte less is refused before any launch."""
    from mrirt import _lib
    lib = _lib.lib()
    e = cases.batch_case(cases.batch_index(7, 32, n))
    ref, dims = e["ref"], e["dims"]
    desc = inr.siren_train_desc(dims, dims[0] - 3, e["w0"])
    nbytes = int(lib.mrirt_siren_train_scratch_bytes(C.byref(desc), n))
    assert nbytes == sr.siren_layout(dims, n)["bytes"] and nbytes % 256 == 0
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    scratch = buf[GUARD:GUARD + nbytes]
    assert scratch.data_ptr() % 16 == 0
    w, b = _flat(e["layers"])
    coords, feats, dl = _dev(e["coords"]), _dev(e["feats"]), _dev(e["dlogits"])
    out = dims[-1]
    logits = torch.full((n + 1, out), -7.0, dtype=torch.float32, device=DEV)
    acc = e["init_w"] is not None
    gw = _dev(e["init_w"]) if acc else torch.full_like(w, -7.0)
    gb = _dev(e["init_b"]) if acc else torch.full_like(b, -7.0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    sp = C.c_void_p(scratch.data_ptr())
    assert lib.mrirt_siren_forward_f32(C.byref(desc), p(w), p(b), p(coords), p(feats), n, p(logits), sp, nbytes, stream) == 0
    assert lib.mrirt_siren_backward(C.byref(desc), p(w), n, p(dl), p(gw), p(gb), 1 if acc else 0, sp, nbytes, stream) == 0
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()), "the guard below the scratch was overwritten"
    assert bool((buf[GUARD + nbytes:] == 0xA5).all()), "the guard above the scratch was overwritten"
    assert bool((logits[n] == -7.0).all())
    assert _same(_np(logits[:n]), ref["logits"]) and _same(_np(gw), ref["gw"]) and _same(_np(gb), ref["gb"])
    _assert_saved(f"guards n={n}", scratch, dims, n, ref)
    # one byte less is refused before anything is launched
    assert lib.mrirt_siren_forward_f32(C.byref(desc), p(w), p(b), p(coords), p(feats), n, p(logits), sp, nbytes - 1, stream) == -5
    assert lib.mrirt_siren_backward(C.byref(desc), p(w), n, p(dl), p(gw), p(gb), 0, sp, nbytes - 1, stream) == -5
    torch.cuda.synchronize()
    assert _same(_np(gw), ref["gw"]) and bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


def test_beyond_the_domain_the_gradient_passes_through(inr):
    """A third of the rows inside +-2^20, a third with pre-activations in +-(2^20, 2^24], a third at +-3e38; p* on a row beyond
    the domain: its first-layer units store sin = +0 and cos = 1 and hand da = dh on.  Logits, saved h / c, dW, db == the
    restatement."""
    e = cases.beyond_case()
    ref = e["ref"]
    assert (ref["cos"][0][cases.BEYOND_NET["pstar"]] == 1).all() and np.count_nonzero(ref["gw"][:17 * 64]) == 17 * 4
    _selection_step(inr, e, cases.N, cases.BEYOND_NET["w0"], True, "beyond the domain")


def test_nonfinite_inputs_stay_in_their_rows(inr):
    """The same net, forward only, with one NaN and one +inf input element in two rows: those logits rows are NaN as the
    restatement's are, every other row keeps the bits of the clean run, and the saved regions match at every row."""
    e, nf = cases.beyond_case(), cases.nonfinite_case()
    desc = inr.siren_train_desc(e["dims"], None, cases.BEYOND_NET["w0"])
    w, b = _flat(e["layers"])
    scratch = inr.siren_train_scratch(desc, cases.N, DEV)
    clean = _np(inr.siren_forward_f32(desc, w, b, None, _dev(e["x"]), cases.N, scratch))
    got = _np(inr.siren_forward_f32(desc, w, b, None, _dev(nf["x"]), cases.N, scratch))
    bad = np.zeros(cases.N, bool)
    bad[list(nf["rows"])] = True
    assert np.array_equal(np.isnan(got), np.isnan(nf["logits"])) and np.isnan(got[bad]).all() and not np.isnan(got[~bad]).any()
    assert sr.bits_differ(got[~bad], clean[~bad]).size == 0 and sr.bits_differ(got, nf["logits"]).size == 0
    assert _same(clean, e["ref"]["logits"])
    _assert_saved("NaN and +inf inputs", scratch, e["dims"], cases.N, nf)


def _split(gw, gb, dims):
    return [(g["W"], g["b"]) for g in lref.unflat(np.asarray(gw), np.asarray(gb), dims)]


@pytest.mark.parametrize("name", list(cases.E2E))
def test_step_against_fp64(inr, name):
    """Deviations on an MI355X: see the figures this test prints; the tolerances are inr_siren_cases.E2E_TOL."""
    c, tol = cases.e2e_case(name), cases.E2E_TOL[name]
    ref = c["ref"]
    desc = inr.siren_train_desc(c["dims"], c["M"], cases.W0)
    w, b = _flat(c["layers"])
    scratch = inr.siren_train_scratch(desc, c["n"], DEV)
    coords, feats, labels = _dev(c["coords"]), _dev(c["feats"]), _dev(c["labels"])

    def run():
        logits = inr.siren_forward_f32(desc, w, b, coords, feats, c["n"], scratch)
        loss, aux, dl = inr.loss_and_dlogits(logits, labels, c["cw"], cases.DICE_WEIGHT, scratch)
        gw, gb = inr.siren_backward_f32(desc, w, c["n"], dl, scratch)
        return [_np(t) for t in (logits, loss, aux, dl, gw, gb)]
    logits, loss, aux, dl, gw, gb = run()
    again = run()
    assert all(_same(x, y) for x, y in zip((logits, loss, aux, dl, gw, gb), again))          # two calls give the same bits
    figures = [("logits", tc.rel_max(logits, ref["logits"]), cases.tol(tol["logits"])),
               ("loss", abs(float(loss) - ref["loss"]) / abs(ref["loss"]), cases.tol(tol["loss"])),
               ("aux", tc.rel_max(aux, ref["aux"]), cases.tol(tol["aux"])),
               ("dlogits", tc.rel_max(dl, ref["dlogits"]), cases.tol(tol["dlogits"])),
               ("grads", tc.tr.deviation(ref, dict(grads=_split(gw, gb, c["dims"]))), cases.tol(tol["grads"]))]
    for what, err, t in figures:
        print(f"{name} {what}: deviation {err:.3g} (tolerance {t:.3g})")
    bad = [f for f in figures if not f[1] <= f[2]]
    assert not bad, bad


def test_python_front_ends(inr):
    """make_siren_loss_and_grad and siren_autograd give the bits of the ctypes layer."""
    name = "siren_7_2x32_4_n321"
    c = cases.e2e_case(name)
    desc = inr.siren_train_desc(c["dims"], c["M"], cases.W0)
    w, b = _flat(c["layers"])
    scratch = inr.siren_train_scratch(desc, c["n"], DEV)
    logits = inr.siren_forward_f32(desc, w, b, _dev(c["coords"]), _dev(c["feats"]), c["n"], scratch)
    loss, aux, dl = inr.loss_and_dlogits(logits, _dev(c["labels"]), c["cw"], cases.DICE_WEIGHT, scratch)
    gw, gb = inr.siren_backward_f32(desc, w, c["n"], dl, scratch)
    want = _split(_np(gw), _np(gb), c["dims"])
    f = inr.make_siren_loss_and_grad(c["classes"], c["cw"], cases.DICE_WEIGHT, cases.W0)
    params = sr.as_dict(c["layers"])
    (loss2, aux2), grads = f(params, c["coords"], c["feats"], c["labels"])
    assert _same(_np(loss2), _np(loss)) and _same(_np(aux2["dice_per_class"]), _np(aux)[1])
    assert sorted(grads) == sorted(params)
    for i, (gW, gB) in enumerate(want):
        assert _same(_np(grads[f"l{i}"]["w"]), gW) and _same(_np(grads[f"l{i}"]["b"]), gB)
    Ws = [_dev(p["W"]).requires_grad_(True) for p in c["layers"]]
    bs = [_dev(p["b"]).requires_grad_(True) for p in c["layers"]]
    out = inr.siren_autograd(Ws, bs, c["coords"], c["feats"], cases.W0)
    assert _same(_np(out.detach()), _np(logits))
    (out * dl).sum().backward()
    for i, (gW, gB) in enumerate(want):
        assert _same(_np(Ws[i].grad), gW) and _same(_np(bs[i].grad), gB)


# ---- loop -----------------------------------------------------------------------------------------------------------------------

def _cfg(inr, c):
    return inr.train_cfg(c["micro"], c["accum"], c["seed"], c["cw"], c["dw"], c["peak"], c["end"], c["warmup"], c["decay_steps"], c["clip"])


def _composition(inr, cache, desc, c, st, steps):
    n, nc = c["micro"], c["classes"]
    scratch = inr.siren_train_scratch(desc, n, st.w.device)
    gw, gb = torch.empty_like(st.w), torch.empty_like(st.b)
    hist = np.zeros((steps, c["accum"], 1 + 2 * nc), np.float32)
    for k in range(steps):
        t = st.step
        for a in range(c["accum"]):
            coords, feats, labels = cache.sample(c["seed"], t * c["accum"] + a, n)
            logits = inr.siren_forward_f32(desc, st.w, st.b, coords, feats, n, scratch)
            loss, aux, dl = inr.loss_and_dlogits(logits, labels, c["cw"], c["dw"], scratch)
            inr.siren_backward_f32(desc, st.w, n, dl, scratch, gw, gb, accumulate=a > 0)
            hist[k, a, 0], hist[k, a, 1:] = float(loss), _np(aux).reshape(-1)
        lr = inr.lr_schedule(c["peak"], c["end"], c["warmup"], c["decay_steps"], t)
        inr.adamw_step(st, gw, gb, lr, gscale=float(np.float32(1.0) / np.float32(c["accum"])), clip_norm=c["clip"])
    return hist


KEYS = ("w", "b", "mu_w", "mu_b", "nu_w", "nu_b")


def _bits(st):
    return [_np(getattr(st, k)).copy() for k in KEYS]


@pytest.mark.parametrize("accum", [2, 3])
def test_run_equals_composition(inr, accum):
    cache, c = inr.VoxelCache(lc.cache_cases("run")), cases.run_cfg(accum)
    desc = inr.siren_train_desc(cases.run_dims(), cases.RUN_NET["M"], cases.W0)
    a, b = inr.AdamWState.from_params(cases.run_layers()), inr.AdamWState.from_params(cases.run_layers())
    want_hist = _composition(inr, cache, desc, c, a, 3)
    hist = _np(inr.train_run(desc, cache, _cfg(inr, c), b, 3))
    assert b.step == 3 and hist.shape == (3, accum, 1 + 2 * c["classes"])
    assert _same(hist, want_hist) and np.isfinite(hist).all()
    for what, x, y in zip(KEYS, _bits(b), _bits(a)):
        assert _same(x, y), what
    assert not _same(_bits(b)[0], lref.flat(cases.run_layers())[0])
    more = _np(inr.train_run(desc, cache, _cfg(inr, c), b, 3))          # continued at step 3 == steps 3..5 of a 6-step run
    whole = inr.AdamWState.from_params(cases.run_layers())
    hist6 = _np(inr.train_run(desc, cache, _cfg(inr, c), whole, 6))
    assert b.step == whole.step == 6
    assert _same(hist6[:3], hist) and _same(hist6[3:], more)
    for what, x, y in zip(KEYS, _bits(b), _bits(whole)):
        assert _same(x, y), what


def test_run_equals_composition_at_long_slabs(inr):
    """The assertion of test_run_equals_composition at a micro-batch that takes 512-point slabs: 16385 points, accum 2, two
    optimiser steps."""
    cache, c = inr.VoxelCache(lc.cache_cases("run")), cases.run_cfg(2, micro=cases.RUN_LONG_MICRO)
    assert c["micro"] == 16385 and sr.slab_len(c["micro"]) == 512
    desc = inr.siren_train_desc(cases.run_dims(), cases.RUN_NET["M"], cases.W0)
    a, b = inr.AdamWState.from_params(cases.run_layers()), inr.AdamWState.from_params(cases.run_layers())
    want_hist = _composition(inr, cache, desc, c, a, 2)
    hist = _np(inr.train_run(desc, cache, _cfg(inr, c), b, 2))
    assert a.step == b.step == 2 and hist.shape == (2, 2, 1 + 2 * c["classes"])
    assert _same(hist, want_hist) and np.isfinite(hist).all()
    for what, x, y in zip(KEYS, _bits(b), _bits(a)):
        assert _same(x, y), what
    assert not _same(_bits(b)[0], lref.flat(cases.run_layers())[0])


def test_train_siren_end_to_end(inr, tmp_path):
    """On an MI355X: see the printed means; the fp64 CPU loop falls by inr_siren_cases.E2E_FALL on the same batches."""
    cfg, cs = cases.E2E_CONFIG, lc.e2e_cases()
    cache = inr.VoxelCache(cs)
    params, state = inr.train_siren(cfg, cache, save_path=tmp_path / "a")
    loss = np.asarray(state["loss_history"])
    assert loss.shape == (40,) and np.isfinite(loss).all()
    first, last = loss[:5].mean(), loss[-5:].mean()
    need = cases.E2E_FALL / 1.5
    print(f"mean of the first 5 losses {first:.4f}, of the last 5 {last:.4f}: factor {first / last:.3f} (required {need:.3f}; the fp64 CPU "
          f"loop: {cases.E2E_FALL_MEANS[0]:.4f} -> {cases.E2E_FALL_MEANS[1]:.4f}, {cases.E2E_FALL} x)")
    assert need > 1.0 and last * need <= first
    assert sorted(params) == ["l0", "l1", "l2"] and [params[f"l{i}"]["w"].shape for i in range(3)] == [(7, 32), (32, 32), (32, 4)]
    init = inr.siren_init(cfg["RNG_SEED"], 7, cfg["HIDDEN_DIMS"], 4, cfg["W0"])
    assert all(_same(init[f"l{i}"]["w"], p["W"]) and _same(init[f"l{i}"]["b"], p["b"]) for i, p in enumerate(cases.e2e_init()))
    # a checkpoint written at step 20 and resumed gives the bits of the uninterrupted run
    ck = tmp_path / "a" / "checkpoint_step000020.npz"
    assert ck.is_file() and (tmp_path / "a" / "checkpoint_step000040.npz").is_file()
    with np.load(ck) as z:
        assert sorted(z.files) == sorted([f"W_{i}" for i in range(3)] + [f"b_{i}" for i in range(3)])
    p2, s2 = inr.train_siren(cfg, cache, resume_from=ck)
    assert s2["opt"].step == 40 and s2["loss_history"] == state["loss_history"][20:]
    assert all(_same(params[k]["w"], p2[k]["w"]) and _same(params[k]["b"], p2[k]["b"]) for k in params)
    # the returned dict goes into the inference path unchanged
    w0 = cfg["W0"]
    net = inr.pack_mlp(params, inr.KIND_SIREN, 0, 4, w0)
    coords, feats, _ = cache.sample(11, 0, 4096)
    cls = _np(inr.classify(net, coords, feats, refined=True)).astype(np.int64)
    layers = [{"W": params[f"l{i}"]["w"], "b": params[f"l{i}"]["b"]} for i in range(3)]
    desc = inr.siren_train_desc([7, 32, 32, 4], 4, w0)
    w, b = _flat(layers)
    logits = _np(inr.siren_forward_f32(desc, w, b, coords, feats, 4096, inr.siren_train_scratch(desc, 4096, DEV)))
    top = np.sort(logits, 1)
    clear = (top[:, -1] - top[:, -2]) > 1e-2 * np.abs(logits).max()
    print(f"classify: {int((~clear).sum())} of 4096 points under the margin; {int((cls[clear] != logits.argmax(1)[clear]).sum())} disagree above it")
    assert (~clear).mean() <= 0.20
    assert np.array_equal(cls[clear], logits.argmax(1)[clear])
