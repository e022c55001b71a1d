"""The references of the INR training tests, checked on the CPU: the fp64 loss against the reference project's own loss_fn
(tests/golden/inr_train_loss.npz, captured by tests/golden/make_inr_train_goldens.py), the fp64 gradients against central
differences, and the preconditions of every case of inr_train_cases.py."""
import numpy as np
import pytest
import torch

import inr_train_cases as cases
import inr_train_ref as tr


def _golden(golden_dir, i):
    z = np.load(golden_dir / "inr_train_loss.npz")
    K, M, nc, nl = (int(v) for v in z[f"c{i}_meta"])
    layers = [{"W": z[f"c{i}_W{l}"], "b": z[f"c{i}_b{l}"]} for l in range(nl)]
    return z, K, nc, layers


@pytest.mark.parametrize("i", [0, 1])
def test_loss_matches_the_reference_loss_fn(golden_dir, i):
    z, K, nc, layers = _golden(golden_dir, i)
    x = tr.build_input(z[f"c{i}_coords"], z[f"c{i}_feats"], K, torch.float64).numpy()
    got = tr.step(layers, x, tr.model_loss(z[f"c{i}_labels"], z[f"c{i}_cw"], float(z[f"c{i}_dw"]), nc))
    assert abs(got["loss"] - float(z[f"c{i}_loss"])) <= 1e-13 * abs(float(z[f"c{i}_loss"]))
    np.testing.assert_allclose(got["aux"][0], z[f"c{i}_ce_per_class"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["aux"][1], z[f"c{i}_dice_per_class"], rtol=1e-13, atol=0)
    if i == 1:
        assert got["aux"][0][nc - 1] == 0.0                # the class that never occurs: count clamps to 1


@pytest.mark.parametrize("i", [0, 1])
def test_gradients_match_central_differences(golden_dir, i):
    z, K, nc, layers = _golden(golden_dir, i)
    x = tr.build_input(z[f"c{i}_coords"], z[f"c{i}_feats"], K, torch.float64).numpy()
    loss = tr.model_loss(z[f"c{i}_labels"], z[f"c{i}_cw"], float(z[f"c{i}_dw"]), nc)
    ref = tr.step(layers, x, loss)
    shapes = [(p["W"].shape, p["b"].shape) for p in layers]
    theta = np.concatenate([np.concatenate([p["W"].reshape(-1), p["b"]]) for p in layers])
    grad = np.concatenate([np.concatenate([gw.reshape(-1), gb]) for gw, gb in ref["grads"]])

    def f(t):
        ls, o = [], 0
        for ws, bs in shapes:
            W = t[o:o + ws[0] * ws[1]].reshape(ws); o += W.size
            b = t[o:o + bs[0]]; o += b.size
            ls.append({"W": W, "b": b})
        return tr.step(ls, x, loss)["loss"]
    rng = np.random.default_rng(i)
    idx = rng.choice(theta.size, 60, replace=False)
    fd = tr.central_differences(f, theta, idx, h=1e-6)
    # fp64 central differences with h = 1e-6: truncation ~h^2, rounding ~1e-16 / h; a kink inside +-h would show as O(1)
    assert np.abs(fd - grad[idx]).max() <= 1e-8 * max(np.abs(grad).max(), 1.0)
    # dlogits too: the loss alone
    la = tr.loss_alone(ref["logits"], z[f"c{i}_labels"], z[f"c{i}_cw"], float(z[f"c{i}_dw"]))
    np.testing.assert_allclose(la["dlogits"], ref["dlogits"], rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("i", range(len(cases.EXACT)), ids=[cases.exact_id(c) for c in cases.EXACT])
def test_exact_cases_are_exact_in_fp32(i):
    c = cases.exact_case(i)
    r = c["ref"]
    assert r["bound"] < 2 ** 24
    assert r["dead_units"] >= 1 and (r["zero_units"] >= 1 or c["x"].shape[0] == 1 and r["zero_units"] >= 0)
    if c["init_w"] is not None:
        assert np.abs(c["init_w"]).max() + r["bound"] < 2 ** 24
    # the fp64 autograd reference agrees with the int64 one, mask convention at z == 0 included (torch.relu'(0) = 0)
    got = tr.step(c["layers"], c["x"], lambda lg: ((lg * torch.as_tensor(c["dlogits"], dtype=lg.dtype)).sum(), None))
    assert np.array_equal(got["logits"], r["logits"])
    for (gw, gb), (rw, rb) in zip(got["grads"], r["grads"]):
        assert np.array_equal(gw, rw) and np.array_equal(gb, rb)


def _check_exact(c, autograd=True):
    r = c["ref"]
    assert r["bound"] < 2 ** 24
    assert r["dead_units"] >= 1 and r["zero_units"] >= 1
    if c["init_w"] is not None:
        assert np.abs(c["init_w"]).max() + r["bound"] < 2 ** 24
    if autograd:
        got = tr.step(c["layers"], c["x"], lambda lg: ((lg * torch.as_tensor(c["dlogits"], dtype=lg.dtype)).sum(), None))
        assert np.array_equal(got["logits"], r["logits"])
        for (gw, gb), (rw, rb) in zip(got["grads"], r["grads"]):
            assert np.array_equal(gw, rw) and np.array_equal(gb, rb)


@pytest.mark.parametrize("i", range(len(cases.SWEEP)), ids=[cases.exact_id(c) for c in cases.SWEEP])
def test_sweep_cases_are_exact_in_fp32(i):
    _check_exact(cases.sweep_case(i))


@pytest.mark.parametrize("i", range(len(cases.BATCH)), ids=[cases.exact_id(c) for c in cases.BATCH])
def test_batch_cases_are_exact_in_fp32(i):
    _check_exact(cases.batch_case(i))


@pytest.mark.parametrize("i", range(len(cases.FEATURE0)), ids=[cases.feature0_id(c) for c in cases.FEATURE0])
def test_feature0_cases_are_exact_in_fp32(i):
    """The doubled net's int64 step is 2 x logits, 2 x dW and 1 x db of the network on (coords, modalities): checked against
    fp64 autograd of the network itself; below 2^24 on the doubled net, every value of the step is exact in fp32."""
    c = cases.feature0_case(i)
    r = c["ref"]
    assert r["bound"] < 2 ** 24 and r["dead_units"] >= 1 and r["zero_units"] >= 1
    assert np.array_equal(c["x"], tr.build_input(c["coords"], c["feats"], 0, torch.float64).numpy())
    assert set(np.unique(c["coords"])) == {-1.0, -0.5, 0.0, 0.5, 1.0} and (c["feats"] is None) == (c["M"] == 0)
    got = tr.step(c["layers"], c["x"], lambda lg: ((lg * torch.as_tensor(c["dlogits"], dtype=lg.dtype)).sum(), None))
    assert np.array_equal(2 * got["logits"], r["logits"])
    for (gw, gb), (rw, rb) in zip(got["grads"], r["grads"]):
        assert np.array_equal(2 * gw, rw) and np.array_equal(gb, rb)
    assert any((np.abs(gw) % 1 == 0.5).any() for gw, _ in got["grads"])          # the halves do occur: the scaling is needed


def test_sweep_and_batch_cases_cover_the_issue():
    S, B = cases.SWEEP, cases.BATCH
    assert len(S) == 36 and len({cases.exact_id(c) for c in S + B + cases.EXACT}) == len(S) + len(B) + len(cases.EXACT)
    hids = {32, 64, 128, 256}
    for axis, values in ((0, cases.SWEEP_INS), (2, cases.SWEEP_DEPTHS), (3, cases.SWEEP_OUTS)):
        assert {(c[1], c[axis]) for c in S} == {(h, v) for h in hids for v in values}, axis
    assert cases.SWEEP_INS == (1, 15, 16, 17, 63, 64, 65, 127, 128) and cases.SWEEP_DEPTHS == (2, 3, 8)
    assert cases.SWEEP_OUTS == (1, 2, 3, 5, 15, 16)
    assert {c[4] for c in S} == {321} and sum(c[5] for c in S) == 9
    assert [c[4] for c in B if c[:4] == (7, 32, 2, 4)] == [16383, 16384, 16385, 32768, 32769, 65536, 65537, 131073]
    assert [c[4] for c in B if c[:4] == (31, 64, 3, 4)] == [16383, 16384, 16385, 32768, 32769] and len(B) == 13
    assert [c for c in B if c[5]] == [(7, 32, 2, 4, 65537, True)] and cases.BATCH_REPEAT in B
    assert all((7, 32, 2, 4, n, n == 65537) in B for n in cases.GUARD_NS) and cases.GUARD_NS == (16384, 16385, 65537)
    assert {c[0] for c in cases.FEATURE0} == {0, 5, 8}


def test_exact_cases_cover_the_shapes():
    E = cases.EXACT
    assert {c[1] for c in E} == {32, 64, 128, 256} and {c[2] for c in E} == {2, 3, 5, 8}
    assert {c[0] for c in E} == {1, 7, 31, 103, 128} and {c[3] for c in E} == {1, 4, 16}
    assert {c[4] for c in E} == {1, 63, 64, 65, 257, 1000} and sum(c[5] for c in E) == 1
    assert sum(cases.exact_case(i)["ref"]["zero_units"] for i in range(len(E))) > 0


@pytest.mark.parametrize("name", list(cases.E2E))
def test_end_to_end_cases_and_their_tolerances(name):
    c = cases.e2e_case(name)
    assert c["removed"] <= 0.05 * cases.E2E[name][5]
    assert tr.kink_free(c["layers"], c["x64"], cases.KINK_MARGIN).all()
    assert len(set(c["labels"].tolist())) == c["classes"]
    for k, v in cases.E2E_TOL[name].items():
        assert 0 < cases.tol(v) <= cases.CAP
    if name != "k16_m4_4x256_n2048":                     # (the large case takes a few seconds per order: measured once, recorded)
        d = cases.fp32_deviation(c, lambda perm: tr.model_loss(c["labels"], cases.CLASS_WEIGHTS, cases.DICE_WEIGHT, c["classes"], perm),
                                 c["ref"], orders=2, seed=1)
        # the recorded value is 8 x a measurement of this very quantity: another order, another machine stay below it
        for k, v in d.items():
            assert v <= cases.tol(cases.E2E_TOL[name][k]), (k, v)


@pytest.mark.parametrize("i", range(len(cases.LOSS)), ids=[cases.loss_id(c) for c in cases.LOSS])
def test_loss_cases(i):
    n, nc, dw, zmax = cases.LOSS[i]
    c = cases.loss_case(i)
    if nc >= 4:
        assert (c["labels"] != nc - 1).all()             # a class absent from the batch
    assert len(set(np.round(c["cw"], 3))) == nc          # unequal class weights
    assert np.isfinite(c["ref"]["loss"]) and np.isfinite(c["ref"]["dlogits"]).all()
    d = cases.loss_fp32_deviation(i)
    for k, v in d.items():
        assert v <= cases.tol(cases.LOSS_TOL[i][k]), (k, v)


def test_loss_cases_cover_the_issue():
    L = cases.LOSS
    assert {c[0] for c in L} == {1, 5, 1000, 100003} and {c[1] for c in L} == {1, 4, 16} and {c[2] for c in L} == {0.0, 0.5, 1.0}
    assert max(c[3] for c in L) == 80.0
    assert {c[1:3] for c in L if c[0] == 100003} == {(4, 0.5), (16, 0.5)}          # beyond the cap of 256 loss blocks
