"""The INR training step on the GPU (csrc/inr_train.hip) against the references of inr_train_ref.py.

  exact      integer ReLU nets: logits, every dW and every db EQUAL the int64 result (a misplaced MFMA element, a wrong tile or
             slab tail, a wrong mask convention at z == 0 changes an integer)
  loss       mrirt_inr_loss on given logits against the fp64 formula
  end to end make_loss_and_grad / mlp_autograd on Fourier nets against fp64 autograd, |g - g_ref| <= tol x A with the tolerances
             of inr_train_cases.py (measured from an fp32 CPU evaluation, never from the kernel)
  determinism  two calls give the same bits
"""
import numpy as np
import pytest
import torch

import inr_train_cases as cases
import inr_train_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inr():
    import mrirt
    assert torch.cuda.is_available()
    return mrirt.inr


def _flat(layers, dev):
    w = torch.from_numpy(np.concatenate([np.asarray(p["W"], np.float32).reshape(-1) for p in layers])).to(dev)
    b = torch.from_numpy(np.concatenate([np.asarray(p["b"], np.float32).reshape(-1) for p in layers])).to(dev)
    return w, b


def _want_grads(c, w_scale=1):
    """The int64 gradients of a case in the flat layouts, the initial values of an accumulate case added."""
    ref = c["ref"]
    want_w = np.concatenate([g[0].reshape(-1) for g in ref["grads"]])
    want_b = np.concatenate([g[1].reshape(-1) for g in ref["grads"]])
    if c.get("init_w") is not None:
        want_w = want_w + w_scale * c["init_w"].astype(np.int64)
        want_b = want_b + c["init_b"].astype(np.int64)
    return want_w, want_b


def _assert_grads(gw, gb, want_w, want_b):
    assert np.array_equal(gw, gw.round()) and np.array_equal(gb, gb.round())
    bad = np.flatnonzero(gw.astype(np.int64) != want_w)
    assert bad.size == 0, (bad[:8], gw[bad[:8]], want_w[bad[:8]])
    bad = np.flatnonzero(gb.astype(np.int64) != want_b)
    assert bad.size == 0, (bad[:8], gb[bad[:8]], want_b[bad[:8]])


def _exact_step(inr, c):
    """One forward + backward of an exact case through mrirt.inr: (logits, gw, gb) as NumPy arrays."""
    dev = torch.device("cuda:0")
    n = c["x"].shape[0]
    desc = inr.train_desc(c["dims"])
    w, b = _flat(c["layers"], dev)
    scratch = inr.train_scratch(desc, n, dev)
    x = torch.from_numpy(c["x"]).to(dev)
    logits = inr.forward_f32(desc, w, b, None, x, n, scratch)
    acc = c["init_w"] is not None
    gw0 = torch.from_numpy(c["init_w"]).to(dev) if acc else None
    gb0 = torch.from_numpy(c["init_b"]).to(dev) if acc else None
    gw, gb = inr.backward_f32(desc, w, n, torch.from_numpy(c["dlogits"]).to(dev), scratch, gw0, gb0, accumulate=acc)
    return logits.cpu().numpy(), gw.cpu().numpy(), gb.cpu().numpy()


def _assert_exact_step(inr, c):
    ref = c["ref"]
    assert ref["bound"] < 2 ** 24
    logits, gw, gb = _exact_step(inr, c)
    bad = np.argwhere(logits.astype(np.int64) != ref["logits"])
    assert bad.size == 0 and np.array_equal(logits, logits.round()), (len(bad), bad[:4])
    _assert_grads(gw, gb, *_want_grads(c))
    return logits, gw, gb


@pytest.mark.parametrize("i", range(len(cases.EXACT)), ids=[cases.exact_id(c) for c in cases.EXACT])
def test_integer_nets_are_exact(inr, i):
    _assert_exact_step(inr, cases.exact_case(i))


@pytest.mark.parametrize("i", range(len(cases.SWEEP)), ids=[cases.exact_id(c) for c in cases.SWEEP])
def test_shape_sweep_is_exact(inr, i):
    """Every (hidden, in), (hidden, layers), (hidden, out) pair of the sweep's axes at n = 321 (inr_train_cases._sweep_nets)."""
    _assert_exact_step(inr, cases.sweep_case(i))


@pytest.mark.parametrize("i", range(len(cases.BATCH)), ids=[cases.exact_id(c) for c in cases.BATCH])
def test_batch_sweep_is_exact(inr, i):
    """Both sides of every doubling of the slab length from 256 to 4096; one case runs twice and demands the same bytes."""
    c = cases.batch_case(i)
    first = _assert_exact_step(inr, c)
    if cases.BATCH[i] == cases.BATCH_REPEAT:
        for a, b in zip(first, _exact_step(inr, c)):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", cases.GUARD_NS)
def test_scratch_exactly_as_long_as_the_abi_asks(inr, n):
    """The step through the raw C ABI with a scratch of exactly mrirt_inr_train_scratch_bytes(desc, n) bytes between two
    guard blocks: n = 16384 has the most slabs of any batch size, at 16385 the count drops (and the slab length doubles),
    65537 is the first n of the loss kernel's stride loop.  mrirt_inr_loss runs on the same scratch between the two passes,
    as the one-call loop uses it; the gradients are those of the batch sweep."""
    import ctypes as C
    import mrirt
    lib = mrirt._lib.lib()
    c = cases.batch_case(cases.batch_index(7, n))
    assert c["x"].shape[0] == n
    dev = torch.device("cuda:0")
    desc = inr.train_desc(c["dims"])
    nbytes = int(lib.mrirt_inr_train_scratch_bytes(C.byref(desc), n))
    assert nbytes > 0 and nbytes >= int(lib.mrirt_inr_loss_scratch_bytes(n))
    guard = 4096
    buf = torch.full((guard + nbytes + guard,), 0x5A, dtype=torch.uint8, device=dev)
    scratch = C.c_void_p(buf.data_ptr() + guard)
    assert scratch.value % 16 == 0
    w, b = _flat(c["layers"], dev)
    x, dl = torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["dlogits"]).to(dev)
    out = c["dims"][-1]
    logits = torch.full((n + 1, out), -7.0, dtype=torch.float32, device=dev)
    acc = c["init_w"] is not None
    gw = torch.from_numpy(c["init_w"]).to(dev) if acc else torch.full_like(w, -7.0)
    gb = torch.from_numpy(c["init_b"]).to(dev) if acc else torch.full_like(b, -7.0)
    labels = torch.from_numpy((np.arange(n) % out).astype(np.int32)).to(dev)
    loss, aux, dl2 = (torch.full(s, -7.0, dtype=torch.float32, device=dev) for s in ((2,), (2 * out + 1,), (n + 1, out)))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.mrirt_inr_forward_f32(C.byref(desc), p(w), p(b), None, p(x), n, p(logits), scratch, nbytes, stream) == 0
    assert lib.mrirt_inr_loss(p(logits), p(labels), n, out, (C.c_float * out)(*([1.0] * out)), 0.5, p(loss), p(aux), p(dl2), scratch, nbytes,
                              stream) == 0
    assert lib.mrirt_inr_backward(C.byref(desc), p(w), n, p(dl), p(gw), p(gb), 1 if acc else 0, scratch, nbytes, stream) == 0
    torch.cuda.synchronize()
    assert bool((buf[:guard] == 0x5A).all()), "the guard below the scratch was overwritten"
    assert bool((buf[guard + nbytes:] == 0x5A).all()), "the guard above the scratch was overwritten"
    assert bool((logits[n] == -7.0).all()) and bool((dl2[n] == -7.0).all()) and float(loss[1]) == -7.0 and float(aux[2 * out]) == -7.0
    assert bool(torch.isfinite(loss[0])) and bool(torch.isfinite(aux[:2 * out]).all()) and bool(torch.isfinite(dl2[:n]).all())
    assert np.array_equal(logits[:n].cpu().numpy().astype(np.int64), c["ref"]["logits"])
    _assert_grads(gw.cpu().numpy(), gb.cpu().numpy(), *_want_grads(c))
    # one byte less is refused before anything is launched
    assert lib.mrirt_inr_backward(C.byref(desc), p(w), n, p(dl), p(gw), p(gb), 0, scratch, nbytes - 1, stream) == -5


@pytest.mark.parametrize("i", range(len(cases.FEATURE0)), ids=[cases.feature0_id(c) for c in cases.FEATURE0])
def test_feature_builder_without_a_sine_is_exact(inr, i):
    """KIND_FOURIER_RELU with K = 0: x = (coords, modalities) assembled by tr_features_kernel, feats=None without modalities.
    Every value is a multiple of 1/2: 2 x logits, 2 x dW and db EQUAL the int64 step of the doubled net."""
    c = cases.feature0_case(i)
    ref = c["ref"]
    assert ref["bound"] < 2 ** 24
    dev = torch.device("cuda:0")
    n = c["coords"].shape[0]
    desc = inr.train_desc(c["dims"], 0, c["M"])
    w, b = _flat(c["layers"], dev)
    scratch = inr.train_scratch(desc, n, dev)
    feats = None if c["feats"] is None else torch.from_numpy(c["feats"]).to(dev)
    logits = inr.forward_f32(desc, w, b, torch.from_numpy(c["coords"]).to(dev), feats, n, scratch).cpu().numpy()
    assert np.array_equal(2.0 * logits.astype(np.float64), ref["logits"].astype(np.float64))
    gw, gb = inr.backward_f32(desc, w, n, torch.from_numpy(c["dlogits"]).to(dev), scratch)
    want_w, want_b = _want_grads(c)
    _assert_grads(2.0 * gw.cpu().numpy().astype(np.float64), gb.cpu().numpy(), want_w, want_b)


def _figure(found, what, err, tol):
    """Print one figure and note it; ``_hold`` asserts after every figure of the test is printed."""
    print(f"{what}: deviation {err:.3g} (tolerance {tol:.3g})")
    found.append((what, err, tol))


def _hold(found):
    bad = [(what, err, tol) for what, err, tol in found if not err <= tol]
    assert not bad, bad


@pytest.mark.parametrize("i", range(len(cases.LOSS)), ids=[cases.loss_id(c) for c in cases.LOSS])
def test_loss_kernel_alone(inr, i):
    c = cases.loss_case(i)
    dev = torch.device("cuda:0")
    loss, aux, dl = inr.loss_and_dlogits(torch.from_numpy(c["logits"]).to(dev), torch.from_numpy(c["labels"]).to(dev), c["cw"], c["dw"])
    ref, tol = c["ref"], cases.LOSS_TOL[i]
    assert loss.dim() == 0 and aux.shape == (2, c["classes"])
    found = []
    _figure(found, "loss", abs(float(loss) - ref["loss"]) / max(abs(ref["loss"]), 1e-300), cases.tol(tol["loss"]))
    _figure(found, "aux", cases.rel_max(aux.cpu().numpy(), ref["aux"]), cases.tol(tol["aux"]))
    _figure(found, "dlogits", cases.rel_max(dl.cpu().numpy(), ref["dlogits"]), cases.tol(tol["dlogits"]))
    first = cases.LOSS_FIRST_STRIDED
    if c["logits"].shape[0] > first:                     # the points past 256 blocks x 256 threads, on the scale of all rows
        err = np.abs(dl[first:].cpu().numpy().astype(np.float64) - ref["dlogits"][first:]).max() / np.abs(ref["dlogits"]).max()
        _figure(found, f"dlogits, rows {first}..", float(err), cases.tol(tol["dlogits"]))
    _hold(found)


def test_out_of_range_labels_read_nothing(inr):
    """Labels outside 0..C-1 are a broken precondition with an unspecified numerical effect; the call must still finish and
    the points with valid labels must keep finite gradients."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    logits = torch.from_numpy(rng.standard_normal((300, 4)).astype(np.float32)).to(dev)
    labels = rng.integers(0, 4, 300).astype(np.int32)
    labels[::7] = np.array([-1, 4, 2 ** 31 - 1, -2 ** 31, 1000], np.int32)[np.arange(labels[::7].size) % 5]
    loss, aux, dl = inr.loss_and_dlogits(logits, torch.from_numpy(labels).to(dev), [1.0, 2.0, 3.0, 4.0], 0.5)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(aux).all()) and bool(torch.isfinite(dl).all())


def _grad_deviation(grads, ref, what):
    worst = 0.0
    for l, (g, (rw, rb), (Aw, Ab)) in enumerate(zip(grads, ref["grads"], ref["A"])):
        for name, got, r, A in (("W", g["W"], rw, Aw), ("b", g["b"], rb, Ab)):
            got = got.cpu().numpy().astype(np.float64)
            assert got.shape == r.shape
            d = np.abs(got - r)
            assert (d[A == 0] == 0).all(), (what, l, name)
            worst = max(worst, float((d[A > 0] / A[A > 0]).max()))
    return worst


@pytest.mark.parametrize("name", list(cases.E2E))
def test_make_loss_and_grad_matches_fp64(inr, name):
    c = cases.e2e_case(name)
    ref, tol = c["ref"], cases.E2E_TOL[name]
    f = inr.make_loss_and_grad(c["classes"], cases.CLASS_WEIGHTS, cases.DICE_WEIGHT, c["K"])
    (loss, aux), grads = f(c["layers"], c["coords"], c["feats"], c["labels"])
    assert loss.dim() == 0 and loss.is_cuda and set(aux) == {"ce_per_class", "dice_per_class"}
    assert [tuple(g["W"].shape) for g in grads] == [tuple(p["W"].shape) for p in c["layers"]]
    got_aux = np.stack([aux["ce_per_class"].cpu().numpy(), aux["dice_per_class"].cpu().numpy()])
    # logits and dlogits of the same step through the entry points that make_loss_and_grad calls
    dev = loss.device
    w, b = _flat(c["layers"], dev)
    desc = inr.train_desc(c["dims"], c["K"], c["M"])
    scratch = inr.train_scratch(desc, c["n"], dev)
    feats = None if c["feats"] is None else torch.from_numpy(c["feats"]).to(dev)          # None: the case without modalities
    assert (feats is None) == (c["M"] == 0)
    logits = inr.forward_f32(desc, w, b, torch.from_numpy(c["coords"]).to(dev), feats, c["n"], scratch)
    loss2, _, dl = inr.loss_and_dlogits(logits, torch.from_numpy(c["labels"]).to(dev), cases.CLASS_WEIGHTS, cases.DICE_WEIGHT)
    assert torch.equal(loss2.reshape(()), loss)
    found = []
    _figure(found, "logits", cases.rel_max(logits.cpu().numpy(), ref["logits"]), cases.tol(tol["logits"]))
    _figure(found, "loss", abs(float(loss) - ref["loss"]) / abs(ref["loss"]), cases.tol(tol["loss"]))
    _figure(found, "aux", cases.rel_max(got_aux, ref["aux"]), cases.tol(tol["aux"]))
    _figure(found, "dlogits", cases.rel_max(dl.cpu().numpy(), ref["dlogits"]), cases.tol(tol["dlogits"]))
    _figure(found, "gradients (of A)", _grad_deviation(grads, ref, name), cases.tol(tol["grads"]))
    _hold(found)


def test_mlp_autograd_with_an_mse_loss(inr):
    c = cases.e2e_case("k4_m4_4x64_n1024")
    ref = cases.mse_ref(c)
    dev = torch.device("cuda:0")
    Ws = [torch.from_numpy(np.asarray(p["W"], np.float32)).to(dev).requires_grad_(True) for p in c["layers"]]
    bs = [torch.from_numpy(np.asarray(p["b"], np.float32)).to(dev).requires_grad_(True) for p in c["layers"]]
    logits = inr.mlp_autograd(Ws, bs, c["coords"], c["feats"], fourier_freqs=c["K"])
    target = torch.from_numpy(cases.mse_target(c)).to(dev)
    logits.retain_grad()
    loss = ((logits - target) ** 2).mean()
    loss.backward()
    tol, found = cases.MSE_TOL, []
    _figure(found, "logits", cases.rel_max(logits.detach().cpu().numpy(), ref["logits"]), cases.tol(tol["logits"]))
    _figure(found, "loss", abs(float(loss) - ref["loss"]) / abs(ref["loss"]), cases.tol(tol["loss"]))
    _figure(found, "dlogits", cases.rel_max(logits.grad.cpu().numpy(), ref["dlogits"]), cases.tol(tol["dlogits"]))
    _figure(found, "gradients (of A)", _grad_deviation([{"W": W.grad, "b": b.grad} for W, b in zip(Ws, bs)], ref, "mse"),
            cases.tol(tol["grads"]))
    _hold(found)


def test_two_calls_give_the_same_bits(inr):
    c = cases.e2e_case("k16_m4_4x256_n2048")
    f = inr.make_loss_and_grad(c["classes"], cases.CLASS_WEIGHTS, cases.DICE_WEIGHT, c["K"])
    runs = []
    for _ in range(2):
        (loss, aux), grads = f(c["layers"], c["coords"], c["feats"], c["labels"])
        runs.append([loss.cpu().numpy(), aux["ce_per_class"].cpu().numpy(), aux["dice_per_class"].cpu().numpy()]
                    + [g[k].cpu().numpy() for g in grads for k in ("W", "b")])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


def test_torch_operators_match_the_ctypes_path(inr):
    """torch.ops.mrirt.inr_* and torch.ops.mrirt_native.inr_* run the same entry points: same bits as mrirt.inr's calls."""
    import mrirt
    c = cases.e2e_case("k2_m1_2x32_n777")
    dev = torch.device("cuda:0")
    w, b = _flat(c["layers"], dev)
    n, dims, K = c["n"], c["dims"], c["K"]
    co, fe = torch.from_numpy(c["coords"]).to(dev), torch.from_numpy(c["feats"]).to(dev)
    lab = torch.from_numpy(c["labels"]).to(dev)
    desc = inr.train_desc(dims, K, 1)
    scratch = inr.train_scratch(desc, n, dev)
    logits = inr.forward_f32(desc, w, b, co, fe, n, scratch)
    loss, aux, dl = inr.loss_and_dlogits(logits, lab, cases.CLASS_WEIGHTS, cases.DICE_WEIGHT)
    gw, gb = inr.backward_f32(desc, w, n, dl, scratch)
    shape = (0, len(dims) - 1, dims[0], dims[-1], dims[1], K, 1)
    for ops in (torch.ops.mrirt, mrirt.torch_ops.load_native()):
        lg, sc = ops.inr_forward_f32(w, b, *shape, co, fe, n)
        ls, ax, d2 = ops.inr_loss(lg, lab, [float(v) for v in cases.CLASS_WEIGHTS], cases.DICE_WEIGHT)
        g1, g2 = ops.inr_backward(w, d2, sc, *shape, n)
        for got, want in ((lg, logits), (ls, loss), (ax, aux), (d2, dl), (g1, gw), (g2, gb)):
            assert torch.equal(got.reshape(-1), want.reshape(-1))
