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
    assert np.array_equal(s, np.zeros(5, f)) and np.array_equal(c, np.ones(5, f))          # finite, in [-1, 1]: sin = +0, cos = 1
    assert not np.signbit(s).any()                       # +0 for the negative arguments too: r = -0 - (-0 P1) = +0
    s, c = sr.sincos32(np.array([np.nan, np.inf, -np.inf], f))
    assert np.isnan(s).all() and np.isnan(c).all()
    s, c = sr.sincos32(np.array([0.0, -0.0, 1e-45, -1e-45, 1e-30], f))                      # tiny arguments: sin a = a, cos a = 1
    want = np.array([0.0, 0.0, 1e-45, -1e-45, 1e-30], f)                                    # but sin(-0) = +0, by the same subtraction
    assert np.array_equal(s, want) and np.array_equal(np.signbit(s), np.signbit(want)) and np.array_equal(c, np.ones(5, f))
    a, s, c = sr.sincos_set("outside")
    fin = np.isfinite(a)
    assert fin.sum() == 10 and (np.abs(a[fin]) > 2.0 ** 20).all() and np.isnan(a).sum() == 4 and np.isinf(a).sum() == 2
    assert np.array_equal(s[fin].view(np.uint32), np.zeros(10, np.uint32)) and np.array_equal(c[fin], np.ones(10, f))
    assert np.isnan(s[~fin]).all() and np.isnan(c[~fin]).all()


def test_bits_differ_sees_what_equality_does_not():
    f = np.float32
    want = np.array([0.0, -0.0, 1.0, np.nan, np.nan, 2.0], f)
    assert sr.bits_differ(want.copy(), want).size == 0
    assert sr.bits_differ(np.array([0.0, -0.0, 1.0, -np.nan, sr._f32([0x7FC12345])[0], 2.0], f), want).size == 0      # NaN payloads and signs are free
    got = np.array([-0.0, 0.0, np.nextafter(f(1), f(2)), 1.0, np.nan, np.nan], f)
    assert sr.bits_differ(got, want).tolist() == [0, 1, 2, 3, 5]          # both signs of zero, one ulp, a missing NaN, a NaN too many


def test_argument_sets_are_what_they_claim():
    assert sr.sincos_set("sweep")[0].size == 3_200_006
    for name, sign in (("top_binade_pos", 1.0), ("top_binade_neg", -1.0)):
        a = sr.sincos_set(name)[0]
        assert a.size == 8_388_609 and a[0] == sign * 2.0 ** 19 and a[-1] == sign * 2.0 ** 20
        assert np.array_equal(np.diff(a.view(np.uint32).astype(np.int64)), np.ones(a.size - 1, np.int64))         # every float between
    q = sr.quadrant_switch_arguments()
    assert q.shape == (2 * sr.QUADRANT_KS, 5) and q.size == 6_675_440 and np.abs(q).max() < 2.0 ** 20
    assert ((sr.QUADRANT_KS - 1) + 0.5) * (np.pi / 2) < 2.0 ** 20 < (sr.QUADRANT_KS + 0.5) * (np.pi / 2)
    k = sr.quadrant_index(q)
    assert ((k.max(1) - k.min(1)) == 1).all()            # the five neighbours of every row fall into two quadrants: 100 % of rows
    assert np.array_equal(k[:sr.QUADRANT_KS].min(1), np.arange(sr.QUADRANT_KS)) and np.array_equal(k[sr.QUADRANT_KS:], -k[:sr.QUADRANT_KS])
    assert (np.diff(q[:sr.QUADRANT_KS], axis=1) > 0).all()
    a = sr.sincos_set("small_and_special")[0]
    bits = a.view(np.uint32)
    den = (bits & 0x7F800000 == 0) & (bits & 0x007FFFFF != 0)
    assert den.sum() == 2 * (len(range(1, 0x800000, 4099)) + 23) and np.signbit(a[a == 0]).tolist() == [False, True]
    assert {float(v) for v in np.abs(a[~den & (a != 0)])} == {2.0 ** e for e in range(-126, 21)} | {float(np.nextafter(np.float32(2.0 ** 20), np.float32(0)))}
    assert np.array_equal(a[a.size // 2:], -a[:a.size // 2])


@pytest.mark.parametrize("name", [n for n in sr.INSIDE_SETS if n != "sweep"])
def test_restated_sincos_on_the_further_sets(name):
    """The whole top binade in both signs, every quadrant switch of the domain, denormals and powers of two: at most 1 result in
    10^5 differs from the rounded fp64 libm value (recorded: 0 in every set), none by more than 1 ulp."""
    a, s, c = sr.sincos_set(name)
    assert (np.abs(a) <= 2.0 ** 20).all()
    sr.assert_libm_figures(name, "restatement", a, s, c)
    tiny = np.abs(a) < 2.0 ** -126
    assert np.array_equal(s[tiny & (a != 0)].view(np.uint32), a[tiny & (a != 0)].view(np.uint32))      # denormals pass through
    assert not np.signbit(s[a == 0]).any() and (c[tiny] == 1).all()


def test_restated_sincos_against_mpmath_at_the_hardest_arguments():
    """Per function, the 1500 arguments of the sweep whose fp64 result lies closest to an fp32 rounding midpoint (where a
    double rounding would show) and the 500 with the smallest |result| (where the reduction's error is relatively largest):
    the restatement must be the 200-bit mpmath value rounded once to fp32."""
    mpmath = pytest.importorskip("mpmath")
    a, s, c = sr.sincos_set("sweep")
    x = a.astype(np.float64)
    with mpmath.workprec(200):
        for what, got, w, fn in (("sin", s, np.sin(x), mpmath.sin), ("cos", c, np.cos(x), mpmath.cos)):
            w32 = w.astype(np.float32)
            dist = 0.5 - np.abs((w - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64))
            idx = np.concatenate([np.argsort(dist, kind="stable")[:1500], np.argsort(np.abs(w), kind="stable")[:500]])
            differ = 0
            for i in idx:
                v = float(mpmath.mpf(mpmath.libmp.mpf_pos(fn(mpmath.mpf(float(a[i])))._mpf_, 24, "n")))          # one rounding, to 24 bits
                assert v == 0.0 or abs(v) >= 2.0 ** -126                                                      # a normal fp32: 24 bits is its width
                differ += int(np.float32(v) != got[i])
            print(f"{what}: {differ} of {idx.size} differ from mpmath rounded once; closest midpoint distance {dist[idx[0]]:.2g} ulp")
            assert differ == 0 and dist[idx[0]] < 1e-6


# ---- the scratch layout ---------------------------------------------------------------------------------------------------------

def _layout_shapes():
    """(dims, n, raw) of every net the new GPU tiers run."""
    out = [(cases.exact_case(i)["dims"], cases.N, c["kind"] == cases.KIND_RAW_SIREN) for i, c in enumerate(cases.EXACT)]
    out += [([c[1]] + [c[2]] * (c[3] - 1) + [c[4]], c[6], c[0] == cases.KIND_RAW_SIREN) for c in cases.BATCH]
    out += [([c["ind"]] + [c["hidden"]] * (c["layers"] - 1) + [c["out"]], cases.HEAD_N, True) for c in cases.HEAD_COVER]
    out += [([17, 64, 64, 4], cases.N, True), (cases.run_dims(), cases.RUN_LONG_MICRO, False)]
    return out


def test_restated_layout_is_the_librarys():
    import ctypes as C
    from mrirt import _lib, inr
    lib = _lib.lib()
    for dims, n, raw in _layout_shapes():
        desc = inr.siren_train_desc(dims, None if raw else dims[0] - 3, 30.0)
        L = sr.siren_layout(dims, n)
        assert L["bytes"] == lib.mrirt_siren_train_scratch_bytes(C.byref(desc), n) > 0, (dims, n)
        relu = _lib.InrDesc()
        relu.kind, relu.numLayers, relu.inDim, relu.hidden, relu.outDim = 2, len(dims) - 1, dims[0], dims[1], dims[-1]
        assert L["offC"] == lib.mrirt_inr_train_scratch_bytes(C.byref(relu), n), (dims, n)        # the cosines start where the ReLU step ends
        assert L["offX"] == lib.mrirt_inr_loss_scratch_bytes(n)
        offs = [L[k] for k in ("offX", "offH", "offDz", "offSlab", "offC", "bytes")]
        assert offs == sorted(offs) and all(o % 256 == 0 for o in offs) and L["act"] >= n * dims[1] * 4
    # the table above inr_train_cases.BATCH_NS: slabs x length (points of the last slab)
    table = {16383: (64, 256, 255), 16384: (64, 256, 256), 16385: (33, 512, 1), 32768: (64, 512, 512), 32769: (33, 1024, 1),
             65536: (64, 1024, 1024), 65537: (33, 2048, 1), 131073: (33, 4096, 1)}
    assert tuple(table) == tc.BATCH_NS
    for n, (count, length, last) in table.items():
        r = sr.slab_ranges(n)
        assert (sr.slabs(n), sr.slab_len(n), r[-1][1] - r[-1][0]) == (count, length, last) and r[-1][1] == n and len(r) == count
    assert (sr.slabs(cases.N), sr.slab_len(cases.N)) == (2, 256) and sr.slabs(cases.HEAD_N) == 1


# ---- the preconditions of the further exact tiers ----------------------------------------------------------------------------------

def test_head_cover_reaches_every_hidden_unit():
    assert len(cases.HEAD_COVER) == 2 + 4 + 8 + 16
    assert {c["w0"] for c in cases.HEAD_COVER} == {1.0, 30.0} and {c["pstar"] for c in cases.HEAD_COVER} == {0, 63, 64}
    for hid in cases.HIDDENS:
        hit = np.zeros(hid, int)
        for i, c in enumerate(cases.HEAD_COVER):
            if c["hidden"] == hid:
                assert (c["ind"], c["layers"], c["out"], c["kind"]) == (17, 3, 16, cases.KIND_RAW_SIREN)
                hit += (cases.head_cover_case(i)["layers"][-1]["W"] != 0).any(1)
        assert (hit == 1).all(), hid                     # every unit of the width, once


@pytest.mark.parametrize("i", range(len(cases.HEAD_COVER)), ids=[cases.exact_id(c) for c in cases.HEAD_COVER])
def test_head_cover_cases_have_single_term_dot_products(i):
    e = cases.head_cover_case(i)
    terms, smallest, largest = sr.single_term(e["layers"], e["x"], e["net"]["w0"], e["dlogits"], e["ref"])
    assert terms == 1 and smallest >= 2.0 ** -126 and largest <= 2.0 ** 20
    assert np.count_nonzero(e["dlogits"].any(1)) == 1 and e["dlogits"][e["net"]["pstar"]].all()
    assert all(np.isfinite(e["ref"][k]).all() for k in ("logits", "gw", "gb"))


@pytest.mark.parametrize("i", range(len(cases.BATCH)), ids=[cases.batch_id(c) for c in cases.BATCH])
def test_batch_cases_have_one_term_per_slab(i):
    e = cases.batch_case(i)
    n, ref = e["n"], e["ref"]
    ranges = sr.slab_ranges(n)
    assert len(ranges) == sr.slabs(n) and e["rows"].size == len(ranges)
    nz = np.flatnonzero(e["dlogits"].any(1))
    assert np.array_equal(nz, e["rows"]) and (e["dlogits"][nz] != 0).all()                  # one row per slab, no zero in it
    smallest, largest = np.inf, 0.0
    for z, (k0, k1) in enumerate(ranges):
        assert k0 <= e["rows"][z] < k1
        assert e["rows"][z] == (k0, k1 - 1, k0 + (k1 - k0) // 2)[z % 3]
        part = dict(ins=[a[k0:k1] for a in ref["ins"]], cos=[a[k0:k1] for a in ref["cos"]])
        terms, s, l = sr.single_term(e["layers"], e["x"][k0:k1], e["w0"], e["dlogits"][k0:k1], part)
        assert terms <= 1, (z, terms)
        smallest, largest = min(smallest, s), max(largest, l)
    assert smallest >= 2.0 ** -126 and largest <= 2.0 ** 20
    assert all(np.isfinite(ref[k]).all() for k in ("logits", "gw", "gb"))
    # every slab adds a non-zero partial to the head's db (and to dW wherever x' and h are non-zero): the order of the sum is under test
    assert len(ranges) >= 33 and np.count_nonzero(ref["gb"][-e["dims"][-1]:]) == e["dims"][-1]
    back = sr.np_step_slabs(e["layers"], e["x"], e["w0"], e["dlogits"], sr.slab_len(n), e["init_w"], e["init_b"], reverse=True,
                            forward=(ref["logits"], ref["ins"], ref["cos"]))
    assert (back["gw"] != ref["gw"]).sum() >= 100 and (back["gb"] != ref["gb"]).sum() >= 4          # the same slabs summed backwards: other bits
    if e["init_w"] is not None:
        assert np.count_nonzero(e["init_w"]) == e["init_w"].size


def test_beyond_the_domain_case_is_what_it_claims():
    e, c = cases.beyond_case(), cases.BEYOND_NET
    cls = cases.beyond_class()
    assert np.bincount(cls).tolist() == [107, 107, 107] and cls[c["pstar"]] == 1
    ax = np.abs(e["x"])
    assert (ax[cls == 0] <= 2.0 ** 20 - 16).all() and (ax[cls == 1] >= 2.0 ** 20 + 16).all() and (ax[cls == 1] <= 2.0 ** 24).all()
    assert (ax[cls == 2] == np.float32(3e38)).all() and np.signbit(e["x"][cls == 2]).any() and not np.signbit(e["x"][cls == 2]).all()
    ref = e["ref"]
    terms, _, largest = sr.single_term(e["layers"], e["x"], c["w0"], e["dlogits"], ref)
    assert terms == 1 and largest > 2.0 ** 127
    h0, c0 = ref["ins"][1], ref["cos"][0]
    assert (h0[cls != 0].view(np.uint32) == 0).all() and (c0[cls != 0] == 1).all()          # beyond the domain: sin = +0, cos = 1
    assert (np.abs(h0[cls == 0]) >= 2.0 ** -126).all()                                      # no denormal sine; the zeros are exact
    assert all(np.isfinite(ref[k]).all() for k in ("logits", "gw", "gb"))
    w0_rows = ref["gw"][:17 * 64].reshape(17, 64)
    assert np.count_nonzero(w0_rows) == 17 * 4           # the gradient went through the units under the head: x'[p*] (x) da_0, cos = 1
    nf = cases.nonfinite_case()
    bad = np.isnan(nf["logits"]).any(1)
    assert np.flatnonzero(bad).tolist() == sorted(nf["rows"]) and np.isnan(nf["logits"][bad]).all()
    assert np.array_equal(nf["logits"][~bad], ref["logits"][~bad])


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
