"""The coordinate-injection INR's training step on the GPU (csrc/inr_inject_train.hip) against the
restated definition (tests/inject_train_ref.py): forward bits, the integer tier (== int64), the selection tier (==
backward32), the tolerance tier (fp64 autograd), determinism and flags, and the Python surface.

Every output and the scratch are sized exactly as the ABI states and lie between guard blocks; each call runs twice, on buffers
pre-filled with 0x00 and with 0xFF, and must give the same bits both times and leave the guards alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import inject_cases as ic
import inject_ref as ref
import inject_train_cases as tc
import inject_train_ref as tref
from mrirt import _lib, inr
from test_gpu_inject import DEV, Net, _ptr, _up, desc_of, dropout, forward, guarded

pytestmark = pytest.mark.gpu


def c_drop(d, index0=0):
    return None if d is None else dropout(d["seed"], d["keep"], 1, d["s"], index0)


def flat_grads(g):
    return np.asarray(g["B"], np.float32).reshape(-1), np.concatenate([np.asarray(w, np.float32).reshape(-1) for w in g["W"]]), np.concatenate(
        [np.asarray(b, np.float32).reshape(-1) for b in g["b"]])


def step(net, shape, coords, mods, drop, dlogits, old=None, flags=None, backward=True, index0=0):
    """forward_train (+ backward) on guarded, exactly sized buffers.  shape: (F, M, widths, cl, ml).  Returns a dict: logits,
    the three gradients, and the regions of the scratch the definition names (features, activations, the last dz buffers, the
    feature gradient)."""
    F, M, widths, cl, ml = shape
    n, L, Cn = coords.shape[0], len(widths), widths[-1]
    lib = _lib.lib()
    c, m = _up(coords), (_up(mods) if M else None)
    dl = _up(dlogits) if dlogits is not None else None
    dp = c_drop(drop, index0)
    nbytes = lib.mrirt_inject_train_scratch_bytes(C.byref(net.desc), n)
    lay = tref.scratch_layout(F, M, widths, cl, ml, n, lib.mrirt_inr_loss_scratch_bytes(n))
    assert nbytes == lay["bytes"] > 0
    oldf = None if old is None else [_up(x) for x in flat_grads(old)]
    fl = (1 if old is not None else 0) if flags is None else flags

    def region(scratch, off, rows, cols):
        return scratch[off:off + 4 * rows * cols].view(torch.float32).clone()

    def run(a):
        logits = a.alloc(4 * n * Cn, torch.float32)
        gB, gw, gb = a.alloc(4 * 3 * (F // 2), torch.float32), a.alloc(4 * net.w.numel(), torch.float32), a.alloc(4 * net.b.numel(), torch.float32)
        scratch = a.alloc(nbytes)
        if oldf is not None:
            for dst, src in zip((gB, gw, gb), oldf):
                dst.copy_(src)
        rc = lib.mrirt_inject_forward_train(C.byref(net.desc), _ptr(net.B), _ptr(net.w), _ptr(net.b), _ptr(c), _ptr(m), n,
                                            C.byref(dp) if dp is not None else None, _ptr(logits), _ptr(scratch), nbytes, None)
        assert rc == 0, rc
        saved = [region(scratch, lay["feat"], n, F)] + [region(scratch, lay["h"][l], n, widths[l]) for l in range(L - 1)]
        if not backward:
            return (logits, *saved)
        rc = lib.mrirt_inject_backward(C.byref(net.desc), _ptr(net.B), _ptr(net.w), _ptr(c), _ptr(m), n, C.byref(dp) if dp is not None else None,
                                       _ptr(dl), _ptr(gB), _ptr(gw), _ptr(gb), fl, _ptr(scratch), nbytes, None)
        assert rc == 0, rc
        dz = [region(scratch, lay["dz"][(L - l) & 1], n, widths[l - 1]) for l in (1, 2) if l < L]       # dz_0 and dz_1: the last two written
        return (logits, *saved, gB, gw, gb, region(scratch, lay["dF"], n, F), *dz)
    out = guarded(run)
    res = dict(logits=out[0].reshape(n, Cn), feat=out[1].reshape(n, F), h=[out[2 + l].reshape(n, widths[l]) for l in range(L - 1)])
    if backward:
        k = 1 + L
        res.update(B=out[k].reshape(-1, 3), w=out[k + 1], b=out[k + 2], dF=out[k + 3].reshape(n, F), dz=[x.reshape(n, -1) for x in out[k + 4:]])
    return res


def differing(name, what, got, want):
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    print(name, what, "differing elements:", int(bad.sum()), "of", bad.size)
    return int(bad.sum())


# ---- 1. forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in ic.EXACT])
def test_forward_train_is_the_forward_and_keeps_what_the_backward_needs(name):
    case = next(c for c in ic.EXACT if c[0] == name)
    params, _, coords, mods = ic.exact_case(case)
    net = Net(params, desc_of(*case[2:7]))
    for drop in (None, dict(seed=0x1234567887654321, keep=0.5, s=5)):
        i0 = (1 << 32) - 17 if drop else 0
        got = step(net, case[2:7], coords, mods, drop, None, backward=False, index0=i0)
        assert got["logits"].tobytes() == forward(net, coords, mods, c_drop(drop, i0))[0].tobytes()
        sv = tref.forward_saved32(params, coords, mods, case[5], case[6], drop, np.arange(case[1], dtype=np.uint64) + np.uint64(i0))
        assert ref.same_bits(got["logits"], sv["logits"]) and ref.same_bits(got["feat"], sv["feat"])
        for l, h in enumerate(sv["h"]):
            assert differing(name, f"h_{l}", got["h"][l], h) == 0


# ---- 2. integer tier -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.INTEGER, ids=[c[0] for c in tc.INTEGER])
def test_integer_tier_equals_int64(case):
    name, n, F, M, widths, cl, ml, _, _, _ = case
    params, c8, mods, dl, drop, old = tc.integer_case(case)
    r = tref.backward_int(params, c8, mods, cl, ml, dl, drop)
    net = Net(params, desc_of(F, M, widths, cl, ml))
    got = step(net, (F, M, widths, cl, ml), (c8 / 8.0).astype(np.float32), mods.astype(np.float32), drop, dl.astype(np.float32), old)
    L, half = len(widths), F // 2
    assert np.array_equal(got["logits"].astype(np.float64) * 8, r["logits8"])
    for l in range(L - 1):
        assert np.array_equal(got["h"][l].astype(np.float64) * 8, r["h8"][l]), l
    oB, ow, ob = flat_grads(old) if old is not None else (0.0, 0.0, 0.0)
    w8 = np.concatenate([w.reshape(-1) for w in r["W8"]]).astype(np.float64)
    assert np.array_equal(got["w"].astype(np.float64) * 8, w8 + 8 * np.asarray(ow, np.float64))
    assert np.array_equal(got["b"].astype(np.float64), np.concatenate(r["b"]).astype(np.float64) + np.asarray(ob, np.float64))
    for k, dz in enumerate(got["dz"]):                          # dh, masked and scaled: dz_0, dz_1
        assert np.array_equal(dz.astype(np.float64), r["dz"][k]), k
    assert np.array_equal(got["dF"][:, half:].astype(np.float64), r["dF"][:, half:])          # dF_c stays; g = dF_s took dF_s's place
    assert np.array_equal(got["dF"][:, :half].astype(np.float64), r["dF"][:, :half])
    want_B = tref.dB_of_int(r["B16"])
    if old is not None:
        want_B = (old["B"] + want_B).astype(np.float32)
    assert ref.same_bits(got["B"], want_B)


# ---- 3. selection tier ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in ic.EXACT])
def test_selection_tier_equals_the_fp32_restatement(name):
    case = next(c for c in ic.EXACT if c[0] == name)
    _, n, F, M, widths, cl, ml, _ = case
    params, _, coords, mods = tc.selection_case(case)
    net = Net(params, desc_of(F, M, widths, cl, ml))
    rng = np.random.default_rng(ic.seed_of(name))
    saved = {}
    bad = 0
    for k, row in enumerate(tc.SELECTION_ROWS):
        drop = None if k % 4 == 3 else tc.dropout_of(0.5 if k % 2 == 0 else 0.25)
        key = None if drop is None else drop["keep"]
        if key not in saved:
            saved[key] = tref.forward_saved32(params, coords, mods, cl, ml, drop)
        dl = tc.one_row_per_slab(rng, n, widths[-1], row)
        want = tref.backward32(params, coords, mods, cl, ml, dl, drop, saved=saved[key])
        got = step(net, (F, M, widths, cl, ml), coords, mods, drop, dl)
        wB, ww, wb = flat_grads(want)
        bad += differing(name, f"row {row} grad_B", got["B"].reshape(-1), wB) + differing(name, f"row {row} grad_w", got["w"], ww)
        bad += differing(name, f"row {row} grad_b", got["b"], wb)
        half = F // 2
        bad += differing(name, f"row {row} g", np.ascontiguousarray(got["dF"][:, :half]), np.ascontiguousarray(want["g"]))
    assert bad == 0


# ---- 4. tolerance tier ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tol(name):
    return tc.tolerance_reference(next(t for t in tc.TOLERANCE if t[0] == name))


@pytest.mark.parametrize("t", tc.TOLERANCE, ids=[t[0] for t in tc.TOLERANCE])
def test_tolerance_tier_against_fp64_autograd(t):
    """|g - g64| <= tol A per element.  Measured on the CPU (backward32 vs grads64, five batch orders, x 8):
    notebook_shape n 257: 1.4e-3, n 4000: 2.8e-5; widths_256_32_96 n 257: 4.8e-3, n 4000: 4.1e-5."""
    name, n, (_, _, F, M, widths, cl, ml) = t
    r = _tol(name)
    assert r["removed"] <= n // 100
    net = Net(r["params"], desc_of(F, M, widths, cl, ml))
    got = step(net, (F, M, widths, cl, ml), r["coords"], r["mods"], r["dropout"], r["dlogits"])
    g64 = r["g64"]
    wo, bo, worst = 0, 0, 0.0
    pieces = [("B", got["B"], g64["B"], g64["A"]["B"])]
    for l, (W, b) in enumerate(zip(g64["W"], g64["b"])):
        pieces.append((f"W_{l}", got["w"][wo:wo + W.size].reshape(W.shape), W, g64["A"]["W"][l]))
        pieces.append((f"b_{l}", got["b"][bo:bo + b.size], b, g64["A"]["b"][l]))
        wo, bo = wo + W.size, bo + b.size
    for what, g, want, A in pieces:
        d = np.abs(g.astype(np.float64) - want)
        rel = float((d[A > 0] / A[A > 0]).max()) if np.any(A > 0) else 0.0
        worst = max(worst, rel)
        print(name, what, "worst |g - g64| / A", rel, "tol", r["tol"])
        assert np.all(d <= r["tol"] * A), what
    print(name, "worst", worst, "tol", r["tol"], "removed", r["removed"])


# ---- 5. determinism and flags --------------------------------------------------------------------------------------------------
def test_determinism_accumulation_and_unknown_flags():
    case = next(c for c in ic.EXACT if c[0] == "n257_F128_M4_notebook")
    _, n, F, M, widths, cl, ml, _ = case
    shape = (F, M, widths, cl, ml)
    params, _, coords, mods = tc.selection_case(case)
    net = Net(params, desc_of(*shape))
    rng = np.random.default_rng(9)
    drop = tc.dropout_of(0.5)
    dl = tc.one_row_per_slab(rng, n, widths[-1], 40)
    a = step(net, shape, coords, mods, drop, dl)
    b = step(net, shape, coords, mods, drop, dl)
    for k in ("logits", "B", "w", "b"):
        assert a[k].tobytes() == b[k].tobytes(), k
    plain = tref.backward32(params, coords, mods, cl, ml, dl, drop)
    old = dict(B=rng.normal(0, 1, plain["B"].shape).astype(np.float32), W=[rng.normal(0, 1, w.shape).astype(np.float32) for w in plain["W"]],
               b=[rng.normal(0, 1, x.shape).astype(np.float32) for x in plain["b"]])
    want = tref.backward32(params, coords, mods, cl, ml, dl, drop, old=old)
    acc = step(net, shape, coords, mods, drop, dl, old)
    wB, ww, wb = flat_grads(want)
    assert differing("flags 1", "grad_B", acc["B"].reshape(-1), wB) + differing("flags 1", "grad_w", acc["w"], ww) + differing("flags 1", "grad_b", acc["b"], wb) == 0
    assert acc["w"].tobytes() != a["w"].tobytes()
    # an unknown flag bit is refused with device pointers too, and nothing is written
    lib = _lib.lib()
    nbytes = lib.mrirt_inject_train_scratch_bytes(C.byref(net.desc), n)
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    g = [torch.full((k,), 7.0, device=DEV) for k in (3 * (F // 2), net.w.numel(), net.b.numel())]
    c, m, d = _up(coords), _up(mods), _up(dl)
    for flags in (2, 3, 1 << 31):
        rc = lib.mrirt_inject_backward(C.byref(net.desc), _ptr(net.B), _ptr(net.w), _ptr(c), _ptr(m), n, None, _ptr(d), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
                                       flags, _ptr(buf), nbytes, None)
        assert rc == -5, flags
    torch.cuda.synchronize()
    assert all(bool((x == 7.0).all()) for x in g) and not bool(buf.any())


def test_a_forward_split_in_two_keeps_its_bits():
    t = tc.TOLERANCE[0]
    name, n, (_, _, F, M, widths, cl, ml) = t
    params, coords, mods, _, _ = tc.tolerance_case(t)
    net = Net(params, desc_of(F, M, widths, cl, ml))
    shape = (F, M, widths, cl, ml)
    drop = dict(seed=3, keep=0.7, s=2)
    whole = step(net, shape, coords, mods, drop, None, backward=False, index0=1000)["logits"]
    parts = [step(net, shape, coords[a:b], mods[a:b], drop, None, backward=False, index0=1000 + a)["logits"] for a, b in ((0, 129), (129, n))]
    assert np.concatenate(parts).tobytes() == whole.tobytes()


# ---- 6. Python -----------------------------------------------------------------------------------------------------------------
def _torch_params(params):
    return {"fourier": {"B": _up(params["fourier"]["B"])}, "mlp": [{"W": _up(p["W"]), "b": _up(p["b"])} for p in params["mlp"]]}


@pytest.mark.parametrize("use_ext", [False, True], ids=["loss", "loss_ext"])
def test_make_inject_loss_and_grad_equals_the_separate_calls(use_ext):
    t = tc.TOLERANCE[0]
    name, n, (_, _, F, M, widths, cl, ml) = t
    params, coords, mods, _, _ = tc.tolerance_case(t)
    rng = np.random.default_rng(1)
    labels = rng.integers(0, 4, n).astype(np.int32)
    cw, dw = [1.0, 2.0, 3.0, 1.5], 0.3
    ext = inr.loss_ext(cw, dw, focal_gamma=2.0) if use_ext else None
    drop = inr.inject_dropout(5, 0.7, 1, 2, 9)
    fn = inr.make_inject_loss_and_grad(4, cw, dw, cl, ml, ext=ext)
    (loss, aux), grads = fn(params, coords, mods, labels, dropout=drop)
    desc = inr.inject_desc(params, cl, ml)
    B, w, b = inr._inject_flat(params, DEV)
    c, m, lab = _up(coords), _up(mods), _up(labels, np.int32)
    scratch = inr.inject_train_scratch(desc, n, DEV)
    logits = inr.inject_forward_train(desc, B, w, b, c, m, n, scratch, drop)
    assert logits.cpu().numpy().tobytes() == inr.inject_forward(params, coords, mods, dropout=drop, coord_layers=cl, mod_layers=ml).cpu().numpy().tobytes()
    want_loss, want_aux, dl, *terms = inr.loss_and_dlogits(logits, lab, cw, dw, ext=ext)      # on the same logits, a scratch of its own
    gB, gw, gb = inr.inject_backward(desc, B, w, c, m, n, dl, scratch, drop)
    assert loss.cpu().numpy().tobytes() == want_loss.cpu().numpy().tobytes()
    assert aux["ce_per_class"].cpu().numpy().tobytes() == want_aux[0].cpu().numpy().tobytes()
    assert aux["dice_per_class"].cpu().numpy().tobytes() == want_aux[1].cpu().numpy().tobytes()
    assert ("terms" in aux) == use_ext and (not use_ext or aux["terms"].cpu().numpy().tobytes() == terms[0].cpu().numpy().tobytes())
    assert grads["fourier"]["B"].cpu().numpy().tobytes() == gB.cpu().numpy().tobytes() and tuple(grads["fourier"]["B"].shape) == (F // 2, 3)
    assert torch.cat([g["W"].reshape(-1) for g in grads["mlp"]]).cpu().numpy().tobytes() == gw.cpu().numpy().tobytes()
    assert torch.cat([g["b"] for g in grads["mlp"]]).cpu().numpy().tobytes() == gb.cpu().numpy().tobytes()
    assert [tuple(g["W"].shape) for g in grads["mlp"]] == [p["W"].shape for p in params["mlp"]]
    assert float(gw.abs().sum()) > 0 and float(gB.abs().sum()) > 0


def test_inject_autograd_backward_is_inject_backward():
    t = tc.TOLERANCE[1]
    name, n, (_, _, F, M, widths, cl, ml) = t
    params, coords, mods, dl, _ = tc.tolerance_case(t)
    drop = inr.inject_dropout(8, 0.7, 1, 1, 0)
    tp = _torch_params(params)
    B = tp["fourier"]["B"].requires_grad_(True)
    Ws = [p["W"].requires_grad_(True) for p in tp["mlp"]]
    bs = [p["b"].requires_grad_(True) for p in tp["mlp"]]
    c, m = _up(coords).requires_grad_(True), _up(mods).requires_grad_(True)
    logits = inr.inject_autograd(B, Ws, bs, c, m, cl, ml, drop)
    logits.backward(_up(dl))
    assert c.grad is None and m.grad is None
    desc = inr.inject_desc(params, cl, ml)
    Bf, w, b = inr._inject_flat(params, DEV)
    scratch = inr.inject_train_scratch(desc, n, DEV)
    want_logits = inr.inject_forward_train(desc, Bf, w, b, _up(coords), _up(mods), n, scratch, drop)
    gB, gw, gb = inr.inject_backward(desc, Bf, w, _up(coords), _up(mods), n, _up(dl), scratch, drop)
    assert logits.detach().cpu().numpy().tobytes() == want_logits.cpu().numpy().tobytes()
    assert B.grad.cpu().numpy().tobytes() == gB.cpu().numpy().tobytes()
    assert torch.cat([W.grad.reshape(-1) for W in Ws]).cpu().numpy().tobytes() == gw.cpu().numpy().tobytes()
    assert torch.cat([x.grad for x in bs]).cpu().numpy().tobytes() == gb.cpu().numpy().tobytes()


def test_train_inject_equals_the_composition_written_out(tmp_path):
    rng = np.random.default_rng(12)
    hwd = (12, 10, 8)
    case = {"mods": rng.normal(0, 1, (4, *hwd)).astype(np.float32), "seg": rng.integers(0, 4, hwd).astype(np.int16)}
    config = dict(NUM_CLASSES=4, RNG_SEED=21, FOURIER_DIM=16, HIDDEN_DIMS=[17, 16, 13], COORD_INJECTION_LAYERS=[1, 2, 3], MODALITY_INJECTION_LAYERS=[2],
                  DROPOUT_RATE=0.3, MICRO_BATCH_SIZE=300, ACCUM_STEPS=2, STAGE1_STEPS=3, STAGE2_STEPS=1, LR_STAGE1=2e-3, LR_STAGE2=5e-4, MIN_LR=1e-5,
                  WARMUP_STEPS=1, WEIGHT_DECAY=1e-4, CLIP_NORM=1.0, CLASS_WEIGHTS=[1.0, 2.0, 3.0, 2.0], DICE_WEIGHT=0.3)
    cache = inr.VoxelCache([case])
    logged = []
    params, state = inr.train_inject(config, cache, log=lambda s, m: logged.append((s, m["train/loss"])), save_path=tmp_path)
    # the same four steps from the separate wrappers: dropout from step 2 on (step > WARMUP_STEPS)
    cl, ml = (1, 2, 3), (2,)
    p0 = inr.inject_init(21, 16, 4, [17, 16, 13], 4, cl, ml)
    desc = inr.inject_desc(p0, cl, ml)
    B, w, b = inr._inject_flat(p0, DEV)
    nw = w.numel()
    wB = torch.cat([w, B.reshape(-1)])
    st = inr.AdamWState([], wB, b, torch.zeros_like(wB), torch.zeros_like(b), torch.zeros_like(wB), torch.zeros_like(b), 0)
    gwB, gb = torch.empty_like(wB), torch.empty_like(b)
    scratch = inr.inject_train_scratch(desc, 300, DEV)
    sched = inr.two_stage_schedule(3, 1, 2e-3, 5e-4, 1, 1e-5)
    keep = float(np.float32(1.0) - np.float32(0.3))
    losses, dropped = [], 0
    for t in range(4):
        per = []
        for k in range(2):
            g = 2 * t + k
            c, m, lab = cache.sample(21, g, 300)
            drop = inr.inject_dropout(21, keep, 1, g, 0) if t > 1 else None
            dropped += drop is not None
            logits = inr.inject_forward_train(desc, wB[nw:], wB[:nw], b, c, m, 300, scratch, drop)
            loss, _, dl = inr.loss_and_dlogits(logits, lab, config["CLASS_WEIGHTS"], 0.3, scratch)
            inr.inject_backward(desc, wB[nw:], wB[:nw], c, m, 300, dl, scratch, drop, gwB[nw:], gwB[:nw], gb, accumulate=k > 0)
            per.append(loss)
        inr.adamw_step(st, gwB, gb, sched(t), 0.5, 1.0, weight_decay=1e-4)
        losses.append(float(torch.stack(per).mean()))
    assert dropped == 4
    opt = state["opt"]
    assert opt.step == 4 and [s for s, _ in logged] == [1, 2, 3, 4]
    for k in ("w", "b", "mu_w", "mu_b", "nu_w", "nu_b"):
        assert getattr(opt, k).cpu().numpy().tobytes() == getattr(st, k).cpu().numpy().tobytes(), k
    assert state["loss_history"] == losses == [v for _, v in logged]
    assert ref.same_bits(params["fourier"]["B"].reshape(-1), wB[nw:].cpu().numpy())
    assert not ref.same_bits(params["fourier"]["B"], p0["fourier"]["B"]) and not ref.same_bits(params["mlp"][1]["W"], p0["mlp"][1]["W"])
    loaded = inr.inject_load(tmp_path / "model_final.npz")
    assert ref.same_bits(loaded["fourier"]["B"], params["fourier"]["B"])
    assert all(ref.same_bits(a["W"], q["W"]) and ref.same_bits(a["b"], q["b"]) for a, q in zip(loaded["mlp"], params["mlp"]))
    pred, seg = inr.predict_full_volume(loaded, case, chunk_size=500)
    assert tuple(pred.shape) == hwd and pred.dtype == torch.int16 and seg is case["seg"]
    assert int(pred.min()) >= 0 and int(pred.max()) <= 3
