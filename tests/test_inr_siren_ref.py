"""The references of the SIREN training tests (tests/inr_siren_ref.py, tests/inr_siren_cases.py), checked without a GPU: the
restated sine against NumPy's fp64 sine rounded once, the fp64 step against the existing SIREN forward, the reference's own
fixture and central differences, and the preconditions that make the exact cases exact."""
import numpy as np
import pytest

import inr_ref as ir
import inr_siren_cases as cases
import inr_siren_ref as sr
import inr_train_cases as tc


def test_restated_sincos_is_the_rounded_fp64_value():
    a = sr.sincos_arguments()
    assert a.size >= 2_000_000 and np.abs(a).max() == 2.0 ** 20
    s, c = sr.sincos32(a)
    x = a.astype(np.float64)
    for what, got, want in (("sin", s, np.sin(x)), ("cos", c, np.cos(x))):
        differ = int((got != want.astype(np.float32)).sum())
        worst = float(sr.ulps(got, want).max())
        print(f"{what}: {differ} of {a.size} differ from float32(np.{what}(float64(a))); worst error {worst:.7f} fp32 ulp")
        assert differ <= a.size // 100000                # at most 1 in 10^5 (the recorded count is 0)
        assert worst <= 1.0
        assert np.abs(got).max() <= 1.0


def test_sincos_outside_the_domain():
    f = np.float32
    edge = f(2.0 ** 20)
    s, c = sr.sincos32(np.array([edge, -edge], f))
    assert np.array_equal(s, np.sin(np.array([2.0 ** 20, -2.0 ** 20])).astype(f)) and np.array_equal(c, np.cos(np.array([2.0 ** 20] * 2)).astype(f))
    beyond = np.array([np.nextafter(edge, f(np.inf)), -np.nextafter(edge, f(np.inf)), 1e10, -3.4028235e38, 3.4028235e38], f)
    s, c = sr.sincos32(beyond)
    assert np.array_equal(s, np.zeros(5, f)) and np.array_equal(c, np.ones(5, f))          # finite, in [-1, 1]: sin = +-0, cos = 1
    s, c = sr.sincos32(np.array([np.nan, np.inf, -np.inf], f))
    assert np.isnan(s).all() and np.isnan(c).all()
    s, c = sr.sincos32(np.array([0.0, -0.0, 1e-45, -1e-45, 1e-30], f))                      # tiny arguments: sin a = a, cos a = 1
    assert np.array_equal(s, np.array([0.0, -0.0, 1e-45, -1e-45, 1e-30], f)) and np.array_equal(c, np.ones(5, f))


@pytest.mark.parametrize("tag,depth", [("s3x256", 3), ("s4x256", 4), ("s4x256w", 4)])
def test_fp64_forward_against_the_reference_fixture(golden_dir, tag, depth):
    """The definition of section 16 (x' = w0 x first) is the notebook's sin(w0 (x W_0) + b_0) up to rounding: against the fixture
    made from the reference's own siren_apply, and against tests/inr_ref.py's forward."""
    s = np.load(golden_dir / "siren.npz")
    layers = [{"W": s[f"{tag}_l{i}_w"], "b": s[f"{tag}_l{i}_b"]} for i in range(depth + 1)]
    want, w0, x = s[f"{tag}_logits"].astype(np.float64), float(s[f"{tag}_w0"]), s[f"{tag}_x"]
    got = sr.forward64(layers, x, w0)
    scale = max(1.0, np.abs(want).max())
    assert np.abs(got - want).max() <= 1e-4 * scale                                        # the fixture is fp32 (REFINED_REL_TOL of test_inr_ref_host)
    assert np.abs(got - ir.forward64(layers, x, ir.KIND_RAW_SIREN, w0)).max() <= 1e-11 * scale
    r = sr.step(layers, x[:64].astype(np.float64), w0, lambda z: ((z * z).mean(), None))
    assert np.abs(r["logits"] - got[:64]).max() <= 1e-12 * scale


def test_gradients_against_central_differences():
    import torch
    rng = np.random.default_rng(5)
    dims, w0, n = [5, 32, 32, 3], 30.0, 40
    layers = sr.siren_layers(rng, dims, w0)
    x = np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.standard_normal((n, 2))], 1)
    labels = rng.integers(0, 3, n)
    cw = [0.5, 1.0, 2.0]
    loss = tc.tr.model_loss(labels, cw, 0.5, 3)
    r = sr.step(layers, x, w0, loss)
    w, b = [np.concatenate([np.asarray(p[k], np.float64).reshape(-1) for p in layers]) for k in ("W", "b")]
    theta = np.concatenate([w, b])
    grad = np.concatenate([g[0].reshape(-1) for g in r["grads"]] + [g[1].reshape(-1) for g in r["grads"]])

    def f(t):
        out, o = [], 0
        for a, c in zip(dims[:-1], dims[1:]):
            out.append({"W": t[o:o + a * c].reshape(a, c)})
            o += a * c
        for p, c in zip(out, dims[1:]):
            p["b"] = t[o:o + c]
            o += c
        z = torch.as_tensor(sr.forward64(out, x, w0))
        return float(loss(z)[0])
    idx = rng.choice(theta.size, 60, replace=False)
    num = tc.tr.central_differences(f, theta, idx, h=1e-6)
    assert np.abs(num - grad[idx]).max() <= 1e-7 * max(1.0, np.abs(grad).max())
    # the fp32 step with the restated sine is the same function: it lands near the fp64 step
    r32 = sr.step(layers, x.astype(np.float32), w0, loss, torch.float32)
    assert tc.tr.deviation(r, r32) < 1e-5


def test_case_lists_cover_what_the_issue_names():
    nets = cases.EXACT
    assert 28 <= len(nets) <= 36
    assert {c["hidden"] for c in nets} == set(cases.HIDDENS) and {c["ind"] for c in nets} == set(cases.INS)
    assert {c["layers"] for c in nets} == set(cases.DEPTHS) and {c["out"] for c in nets} == set(cases.OUTS)
    assert {(c["hidden"], c["ind"]) for c in nets} == {(h, i) for h in cases.HIDDENS for i in cases.INS}
    assert {(c["hidden"], c["layers"]) for c in nets} == {(h, d) for h in cases.HIDDENS for d in cases.DEPTHS}
    assert {c["kind"] for c in nets} == {cases.KIND_SIREN, cases.KIND_RAW_SIREN} and {c["w0"] for c in nets} == {1.0, 30.0}
    assert {c["pstar"] for c in nets} == set(cases.P_STARS) and sum(c["span"] for c in nets) == 1
    assert abs(sum(c["acc"] for c in nets) - len(nets) / 4) <= 1
    assert all(c["kind"] == cases.KIND_RAW_SIREN or 3 <= c["ind"] <= 11 for c in nets)
    for hid in cases.HIDDENS:                            # the heads of one width select consecutive runs: every hidden unit where
        hit, total = np.zeros(hid, bool), 0              # the cases' outputs add up to the width, no unit twice before that
        for i, c in enumerate(nets):
            if c["hidden"] == hid:
                hit |= (cases.exact_case(i)["layers"][-1]["W"] != 0).any(1)
                total += c["out"]
        assert hit.sum() == min(total, hid), hid
        if hid <= 32:
            assert hit.all(), hid
    assert set(cases.E2E_TOL) == set(cases.E2E)
    for t in cases.E2E_TOL.values():
        assert all(0 < cases.tol(v) <= cases.CAP for v in t.values())
    assert cases.E2E_FALL / 1.5 > 1.0


@pytest.mark.parametrize("i", range(len(cases.EXACT)), ids=[cases.exact_id(c) for c in cases.EXACT])
def test_exact_cases_have_single_term_dot_products(i):
    e = cases.exact_case(i)
    c = e["net"]
    for p in e["layers"]:
        assert set(np.unique(p["W"])) <= {0.0, 1.0}
    terms, smallest, largest = sr.single_term(e["layers"], e["x"], c["w0"], e["dlogits"])
    assert terms == 1                                    # every dot product: one non-zero term
    assert smallest >= 2.0 ** -126                       # no denormal sine enters a product
    assert largest <= 2.0 ** 20                          # inside the sine's domain
    if c["span"]:
        assert largest > 2.0 ** 19
    ref = e["ref"]
    assert np.isfinite(ref["logits"]).all() and np.isfinite(ref["gw"]).all() and np.isfinite(ref["gb"]).all()
    assert np.count_nonzero(e["dlogits"].any(1)) == 1 and e["dlogits"][c["pstar"]].all()
    # the restatement is what the fp64 definition rounds to: logits within a few fp32 ulp of the fp64 forward of the fp32 x'
    xs = (np.float32(c["w0"]) * e["x"]).astype(np.float32).astype(np.float64)
    want = sr.forward64(e["layers"], xs, 1.0)
    if not c["span"]:
        assert np.abs(ref["logits"] - want).max() <= 1e-4
