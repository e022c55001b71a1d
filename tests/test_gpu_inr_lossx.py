"""mrirt_inr_loss_ext on the GPU (csrc/inr_lossx.hip): the neutral configuration against mrirt_inr_loss
bit for bit, every option alone and together against the fp64 restatement of scripts/jax_inr_brats.py's loss
(tests/inr_lossx_ref.py) within the recorded tolerances of tests/inr_lossx_cases.py, finiteness at the edges of the domain,
repeatability, the optional outputs, the exact scratch size, and the whole step through make_loss_and_grad(ext=...)."""
import ctypes as C

import numpy as np
import pytest
import torch

import inr_lossx_cases as cases
import inr_siren_cases as sc
import inr_train_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def inr():
    import mrirt
    assert torch.cuda.is_available()
    return mrirt.inr


def _ext(inr, cw, opt):
    return inr.loss_ext(cw, opt["dice_weight"], opt["per_class_dice"], opt["focal_gamma"], opt["focal_alpha"], opt["label_smoothing"],
                        opt["edema_fp_weight"], opt["tversky_alpha"], opt["tversky_beta"], opt["tversky_weight"], opt["edema_logit_reg"],
                        opt["edema_class"])


def _figure(found, what, err, tol):
    print(f"{what}: deviation {err:.3g} (tolerance {tol:.3g})")
    found.append((what, err, tol))


def _hold(found):
    bad = [(what, err, tol) for what, err, tol in found if not err <= tol]
    assert not bad, bad


@pytest.mark.parametrize("i", range(len(tc.LOSS)), ids=[tc.loss_id(c) for c in tc.LOSS])
def test_neutral_configuration_gives_the_plain_loss_bits(inr, i):
    c = tc.loss_case(i)
    z, lab = torch.from_numpy(c["logits"]).to(DEV), torch.from_numpy(c["labels"]).to(DEV)
    loss0, aux0, dl0 = inr.loss_and_dlogits(z, lab, c["cw"], c["dw"])
    loss1, aux1, dl1, terms = inr.loss_and_dlogits(z, lab, None, None, ext=inr.loss_ext(c["cw"], c["dw"], per_class_dice=True))
    assert np.array_equal(loss0.cpu().numpy(), loss1.cpu().numpy())
    assert np.array_equal(aux0.cpu().numpy(), aux1.cpu().numpy())
    assert np.array_equal(dl0.cpu().numpy(), dl1.cpu().numpy())
    assert terms.shape == (5,) and bool(torch.isfinite(terms).all())


@pytest.mark.parametrize("name", list(cases.LOSS))
def test_every_option_against_the_fp64_restatement(inr, name):
    c = cases.loss_case(name)
    ref, tol = c["ref"], cases.LOSS_TOL[name]
    z, lab = torch.from_numpy(c["logits"]).to(DEV), torch.from_numpy(c["labels"]).to(DEV)
    loss, aux, dl, terms = inr.loss_and_dlogits(z, lab, None, None, ext=_ext(inr, c["cw"], c["opt"]))
    assert loss.dim() == 0 and aux.shape == (2, c["classes"]) and terms.shape == (5,) and dl.shape == z.shape
    found = []
    _figure(found, "loss", abs(float(loss) - ref["loss"]) / max(abs(ref["loss"]), 1e-300), cases.tol(tol["loss"]))
    _figure(found, "aux", tc.rel_max(aux.cpu().numpy(), ref["aux"]), cases.tol(tol["aux"]))
    _figure(found, "terms", tc.rel_max(terms.cpu().numpy(), ref["terms"]), cases.tol(tol["terms"]))
    _figure(found, "dlogits", tc.rel_max(dl.cpu().numpy(), ref["dlogits"]), cases.tol(tol["dlogits"]))
    first = tc.LOSS_FIRST_STRIDED
    if c["n"] > first:                                   # the points past 256 blocks x 256 threads, on the scale of all rows
        err = np.abs(dl[first:].cpu().numpy().astype(np.float64) - ref["dlogits"][first:]).max() / np.abs(ref["dlogits"]).max()
        _figure(found, f"dlogits, rows {first}..", float(err), cases.tol(tol["dlogits"]))
    _hold(found)


def test_a_missing_term_would_show(inr):
    """The tolerances are far below what dropping any one option changes in the fp64 loss of the all-options case."""
    import inr_lossx_ref as lx
    c = cases.loss_case("all_n257_c4")
    for k, v in (("focal_gamma", 0.0), ("label_smoothing", 0.0), ("per_class_dice", True), ("edema_fp_weight", 0.0), ("tversky_weight", 0.0),
                 ("edema_logit_reg", 0.0), ("focal_alpha", None)):
        other = lx.loss_alone(c["logits"], c["labels"], c["cw"], dict(c["opt"], **{k: v}))
        assert abs(other["loss"] - c["ref"]["loss"]) / abs(c["ref"]["loss"]) > 100 * cases.tol(cases.LOSS_TOL["all_n257_c4"]["loss"]), k


@pytest.mark.parametrize("gamma", [1.0, 2.0, 5.0])
def test_extreme_logits_and_foreign_labels_stay_finite(inr, gamma):
    """|z| = 100 with the label on the winning class (pt rounds to 1 in fp32, every other probability underflows to 0) and on a
    losing class (pt = 0, log p = -200), and labels outside 0..C-1: every output finite."""
    n, nc = 600, 4
    rng = np.random.default_rng(11)
    z = np.full((n, nc), -100.0, np.float32)
    win = rng.integers(0, nc, n)
    z[np.arange(n), win] = 100.0
    labels = win.astype(np.int32)
    labels[1::3] = (win[1::3] + 1) % nc
    labels[2::9] = np.array([-1, nc, 2 ** 31 - 1, -2 ** 31], np.int32)[np.arange(labels[2::9].size) % 4]
    p = torch.softmax(torch.from_numpy(z), -1).numpy()
    assert (p[np.arange(n), win] == 1.0).all()           # pt == 1 in fp32
    alpha = [0.25, 1.0, 0.5, 2.0]
    for eps, fa in ((0.0, None), (0.05, alpha)):
        ext = inr.loss_ext([0.5, 1.0, 2.0, 1.5], 0.5, False, gamma, fa, eps, 0.3, 0.7, 0.3, 0.4, 0.2, 2)
        out = inr.loss_and_dlogits(torch.from_numpy(z).to(DEV), torch.from_numpy(labels).to(DEV), None, None, ext=ext)
        for name, t in zip(("loss", "aux", "dlogits", "terms"), out):
            assert bool(torch.isfinite(t).all()), (name, gamma, eps)


def test_two_calls_give_the_same_bits(inr):
    c = cases.loss_case("all_big_c4")
    z, lab = torch.from_numpy(c["logits"]).to(DEV), torch.from_numpy(c["labels"]).to(DEV)
    ext = _ext(inr, c["cw"], c["opt"])
    a = inr.loss_and_dlogits(z, lab, None, None, ext=ext)
    b = inr.loss_and_dlogits(z, lab, None, None, ext=ext)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


@pytest.mark.parametrize("n", [257, cases.BIG])
def test_raw_abi_optional_outputs_and_exact_scratch(inr, n):
    """Through the C ABI with a scratch of exactly mrirt_inr_loss_ext_scratch_bytes(n) bytes between two guard blocks and one
    spare row behind every output; dlogits = NULL and terms = NULL are accepted and change nothing else."""
    import mrirt
    lib = mrirt._lib.lib()
    c = cases.loss_case("all_n257_c4" if n == 257 else "all_big_c4")
    nc = c["classes"]
    nbytes = int(lib.mrirt_inr_loss_ext_scratch_bytes(n))
    assert nbytes == ((min(-(-n // 256), 256) + 1) * 71 * 8 + 255 & ~255) >= int(lib.mrirt_inr_loss_scratch_bytes(n))
    guard = 4096
    buf = torch.full((guard + nbytes + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    scratch = C.c_void_p(buf.data_ptr() + guard)
    assert scratch.value % 16 == 0
    z, lab = torch.from_numpy(c["logits"]).to(DEV), torch.from_numpy(c["labels"]).to(DEV)
    ext = _ext(inr, c["cw"], c["opt"])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())               # noqa: E731
    outs = []
    for want_dl, want_terms in ((True, True), (False, True), (True, False), (False, False)):
        loss, aux, terms, dl = (torch.full(s, -7.0, dtype=torch.float32, device=DEV) for s in ((2,), (2 * nc + 1,), (6,), (n + 1, nc)))
        rc = lib.mrirt_inr_loss_ext(p(z), p(lab), n, nc, C.byref(ext), p(loss), p(aux), p(terms) if want_terms else None,
                                    p(dl) if want_dl else None, scratch, nbytes, stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert float(loss[1]) == -7.0 and float(aux[2 * nc]) == -7.0 and float(terms[5]) == -7.0 and bool((dl[n] == -7.0).all())
        assert want_dl or bool((dl == -7.0).all())
        assert want_terms or bool((terms == -7.0).all())
        outs.append((loss[:1].cpu().numpy(), aux[:2 * nc].cpu().numpy(), terms[:5].cpu().numpy(), dl[:n].cpu().numpy()))
    assert bool((buf[:guard] == 0x5A).all()), "the guard below the scratch was overwritten"
    assert bool((buf[guard + nbytes:] == 0x5A).all()), "the guard above the scratch was overwritten"
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])
    assert np.array_equal(outs[1][2], outs[0][2]) and np.array_equal(outs[2][3], outs[0][3])
    assert tc.rel_max(outs[0][3], c["ref"]["dlogits"]) <= cases.tol(cases.LOSS_TOL["all_n257_c4" if n == 257 else "all_big_c4"]["dlogits"])
    # one byte less is refused before anything is launched
    assert lib.mrirt_inr_loss_ext(p(z), p(lab), n, nc, C.byref(ext), p(loss), p(aux), None, None, scratch, nbytes - 1, stream) == -5


def _grad_deviation(grads, ref):
    worst = 0.0
    for g, (rw, rb), (Aw, Ab) in zip(grads, ref["grads"], ref["A"]):
        for got, r, A in ((g["W"], rw, Aw), (g["b"], rb, Ab)):
            got = got.cpu().numpy().astype(np.float64)
            assert got.shape == r.shape
            d = np.abs(got - r)
            assert (d[A == 0] == 0).all()
            worst = max(worst, float((d[A > 0] / A[A > 0]).max()))
    return worst


def _hold_step(loss, aux, grads, ref, tol):
    assert set(aux) == {"ce_per_class", "dice_per_class", "terms"} and aux["terms"].shape == (5,)
    got_aux = np.stack([aux["ce_per_class"].cpu().numpy(), aux["dice_per_class"].cpu().numpy()])
    found = []
    _figure(found, "loss", abs(float(loss) - ref["loss"]) / abs(ref["loss"]), cases.tol(tol["loss"]))
    _figure(found, "aux", tc.rel_max(got_aux, ref["aux"]), cases.tol(tol["aux"]))
    _figure(found, "gradients (of A)", _grad_deviation(grads, ref), cases.tol(tol["grads"]))
    _hold(found)


def test_relu_step_with_the_extended_loss(inr):
    c = cases.relu_step_case()
    ext = _ext(inr, tc.CLASS_WEIGHTS, cases.step_opt())
    (loss, aux), grads = inr.make_loss_and_grad(c["classes"], tc.CLASS_WEIGHTS, 0.0, c["K"], ext=ext)(c["layers"], c["coords"], c["feats"], c["labels"])
    _hold_step(loss, aux, grads, c["ref"], cases.STEP_TOL["relu"])
    (plain, aux0), _ = inr.make_loss_and_grad(c["classes"], tc.CLASS_WEIGHTS, tc.DICE_WEIGHT, c["K"])(c["layers"], c["coords"], c["feats"], c["labels"])
    assert set(aux0) == {"ce_per_class", "dice_per_class"} and float(plain) != float(loss)


def test_siren_step_with_the_extended_loss(inr):
    c = cases.siren_step_case()
    ext = _ext(inr, c["cw"], cases.step_opt())
    params = {f"l{i}": {"w": p["W"], "b": p["b"]} for i, p in enumerate(c["layers"])}
    (loss, aux), grads = inr.make_siren_loss_and_grad(c["classes"], c["cw"], 0.0, sc.W0, ext=ext)(params, c["coords"], c["feats"], c["labels"])
    glist = [{"W": grads[f"l{i}"]["w"], "b": grads[f"l{i}"]["b"]} for i in range(len(c["layers"]))]
    _hold_step(loss, aux, glist, c["ref"], cases.STEP_TOL["siren"])


def test_torch_operators_match_the_ctypes_path(inr):
    import mrirt
    c = cases.loss_case("all_n257_c4")
    o = c["opt"]
    z, lab = torch.from_numpy(c["logits"]).to(DEV), torch.from_numpy(c["labels"]).to(DEV)
    want = inr.loss_and_dlogits(z, lab, None, None, ext=_ext(inr, c["cw"], o))
    for ops in (torch.ops.mrirt, mrirt.torch_ops.load_native()):
        loss, aux, terms, dl = ops.inr_loss_ext(z, lab, [float(v) for v in c["cw"]], [float(v) for v in o["focal_alpha"]], o["dice_weight"],
                                                o["per_class_dice"], o["focal_gamma"], o["label_smoothing"], o["edema_fp_weight"], o["tversky_alpha"],
                                                o["tversky_beta"], o["tversky_weight"], o["edema_logit_reg"], o["edema_class"])
        for got, w in zip((loss.reshape(()), aux, dl, terms), want):
            assert np.array_equal(got.cpu().numpy(), w.cpu().numpy())
        neutral = ops.inr_loss_ext(z, lab, [float(v) for v in c["cw"]], [], 0.5, True, 0.0, 0.0, 0.0, 0.8, 0.2, 0.0, 0.0, 2)
        plain = inr.loss_and_dlogits(z, lab, c["cw"], 0.5)
        assert np.array_equal(neutral[0].cpu().numpy().reshape(()), plain[0].cpu().numpy()) and np.array_equal(neutral[3].cpu().numpy(), plain[2].cpu().numpy())
