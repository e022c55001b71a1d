"""The Muon restatement (inr_muon_ref.py) against the algorithm's definition, and the preconditions of the exact GPU cases.  No GPU.

  definition      for m = U S V^T the fp64 Newton-Schulz equals U p^(k)(S) V^T with p(s) = c0 s + c1 s^3 + c2 s^5: this pins the
                  restatement independently of any kernel (optax itself is not available to compare with)
  preconditions   every exact case: at most one non-zero term in every sum of every product, no denormal, no overflow
  fixed order     the kernel-order sum of squares equals math.fsum where it must (exact cases) and to rounding elsewhere
"""
import math

import numpy as np
import pytest

import inr_muon_cases as cases
import inr_muon_ref as ref


@pytest.mark.parametrize("shape", [(5, 9), (9, 5), (6, 6), (1, 7), (7, 1)])
@pytest.mark.parametrize("steps", [1, 3, 5])
def test_newton_schulz_is_the_polynomial_of_the_singular_values(shape, steps):
    rng = np.random.default_rng(shape[0] * 100 + shape[1] + steps)
    m = rng.standard_normal(shape)
    h = ref.hp(ns_steps=steps)
    c0, c1, c2 = (float(np.float32(c)) for c in h["ns_coeffs"])
    x0 = m / (np.sqrt((m * m).sum()) + float(np.float32(h["eps"])))
    U, S, Vt = np.linalg.svd(x0, full_matrices=False)
    assert np.all(np.diff(S) < 0) or S.size == 1
    for _ in range(steps):
        S = c0 * S + c1 * S ** 3 + c2 * S ** 5
    want = (U * S) @ Vt
    got = ref.ns(m, h, np.float64)
    assert got.shape == shape and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


def test_newton_schulz_orthogonalises():
    """Five steps with optax's coefficients bring every singular value of a well-conditioned matrix into about [0.68, 1.13]."""
    rng = np.random.default_rng(5)
    for shape in ((16, 48), (48, 16)):
        Q = ref.ns(rng.standard_normal(shape), None, np.float64)
        S = np.linalg.svd(Q, compute_uv=False)
        assert 0.6 < S.min() and S.max() < 1.2, S
    assert not ref.ns(np.zeros((4, 6)), None, np.float32).any()
    assert np.isnan(ref.ns(np.array([[1.0, np.nan], [0.0, 2.0]]), None, np.float32)).all()


def test_step_definition_in_fp64():
    """momentum / apply against the formulas written out with Python floats."""
    h = ref.hp()
    beta = float(np.float32(0.95))
    mu, g, s, t, gs = 0.3, -0.7, 0.5, 4, 0.25
    mu2, mhat = ref.momentum(np.array([mu]), np.array([g]), s, t, gs, h, np.float64)
    gc = g * gs * s
    want_mu = beta * mu + (1 - beta) * gc
    assert mu2[0] == pytest.approx(want_mu, rel=1e-15)
    assert mhat[0] == pytest.approx(beta * want_mu / (1 - beta ** (t + 2)) + (1 - beta) * gc / (1 - beta ** (t + 1)), rel=1e-14)
    _, plain = ref.momentum(np.array([mu]), np.array([g]), s, t, gs, ref.hp(nesterov=False), np.float64)
    assert plain[0] == pytest.approx(want_mu / (1 - beta ** (t + 1)), rel=1e-14)
    w = ref.apply(np.arange(1.0, 13.0), np.ones(12), 0.5, [1, 4, 2], ref.hp(weight_decay=0.25), np.float64)
    wd = 0.25
    assert np.allclose(w[:4], [x - 0.5 * (2.0 + wd * x) for x in (1.0, 2.0, 3.0, 4.0)], rtol=1e-15)      # 1 -> 4: sqrt(4)
    assert np.allclose(w[4:], [x - 0.5 * (1.0 + wd * x) for x in np.arange(5.0, 13.0)], rtol=1e-15)                  # 4 -> 2: max(1, .) = 1
    assert ref.layer_scale(7, 256) == np.float32(math.sqrt(256 / 7)) and ref.layer_scale(256, 4) == np.float32(1.0)


def test_fixed_order_sum():
    rng = np.random.default_rng(3)
    for n in (1, 63, 256, 257, 70000):
        v = rng.standard_normal(n).astype(np.float32)
        exact = math.fsum((v.astype(np.float64) ** 2).tolist())
        assert abs(ref.sumsq_fixed(v) - exact) <= 2.0 ** -52 * n * exact
    for i in range(len(cases.EXACT)):
        for M in ref.split(cases.exact_case(i), cases.EXACT[i]["dims"]):
            assert ref.sumsq_fixed(M) == math.fsum((M.astype(np.float64).reshape(-1) ** 2).tolist())


@pytest.mark.parametrize("ns_steps", cases.EXACT_NS_STEPS)
@pytest.mark.parametrize("i", range(len(cases.EXACT)), ids=[cases.exact_id(c) for c in cases.EXACT])
def test_exact_case_preconditions(i, ns_steps):
    c, m = cases.EXACT[i], cases.exact_case(i)
    tiny, huge = 2.0 ** -126, 2.0 ** 127
    seen = dict(products=0, terms=0)

    def trace(what, lhs, rhs, out):
        if lhs is not None:
            terms = (lhs != 0).astype(np.int64) @ (rhs != 0).astype(np.int64)
            seen["terms"] = max(seen["terms"], int(terms.max()))
            seen["products"] += 1
        mag = np.abs(out[out != 0].astype(np.float64))
        assert np.isfinite(out).all() and (mag.size == 0 or (mag.min() >= tiny and mag.max() < huge)), what
    mats = ref.split(m, c["dims"])
    for l, M in enumerate(mats):
        assert ((M != 0).sum(axis=0) <= 1).all() and ((M != 0).sum(axis=1) <= 1).all()
        nz = np.abs(M[M != 0])
        if l == c.get("zero"):
            assert nz.size == 0
            continue
        assert np.all(np.log2(nz) == np.round(np.log2(nz)))
        if min(M.shape) >= 2:
            assert np.unique(nz).size >= 2                # distinct singular values
        if l in c.get("holes", ()):
            assert (~M.any(axis=1)).any() and (~M.any(axis=0)).any()
        out = ref.ns(M, ref.hp(ns_steps=ns_steps), np.float32, trace)
        x0 = (M.astype(np.float64) / (math.sqrt(ref.sumsq_fixed(M)) + 1e-8))
        mag = np.abs(x0[x0 != 0])
        assert mag.min() >= tiny and ((out != 0) == (M != 0)).all()
    assert seen["terms"] == 1 and seen["products"] > 0


def test_exact_cases_cover_the_stated_shapes():
    ins = {c["dims"][0] for c in cases.EXACT}
    outs = {c["dims"][-1] for c in cases.EXACT}
    hidden = {c["dims"][1] for c in cases.EXACT}
    depths = {len(c["dims"]) - 1 for c in cases.EXACT}
    assert ins == {1, 7, 17, 65, 128} and outs == {1, 4, 16} and hidden == {32, 64, 128, 256} and depths >= {2, 3, 8}
    assert any("zero" in c for c in cases.EXACT) and any("holes" in c for c in cases.EXACT)


def test_recorded_deviations_are_reproduced():
    """The recorded figures are what this machine's NumPy measures, to within the spread between BLAS builds (a factor 2)."""
    for name, dev in cases.measure_ns().items():
        assert 0.5 * cases.NS_DEVIATION[name] <= dev <= 2.0 * cases.NS_DEVIATION[name], (name, dev)
    for key, dev in cases.measure_step().items():
        assert 0.5 * cases.STEP_DEVIATION[key] <= dev <= 2.0 * cases.STEP_DEVIATION[key], (key, dev)
