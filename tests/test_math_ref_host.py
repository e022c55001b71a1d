"""CPU side of the device math primitive tests (tests/test_gpu_math_primitives.py): the references of tests/math_ref.py check
themselves and the oracle's transcendentals; the host helpers the kernels depend on (make_udiv, fill_exp_consts, fill_camera,
prepare()'s refusal of a NaN intensityAlpha) are checked bit for bit through the probe library's host entries; and every
assertion helper the GPU tests use is shown to FAIL on a NumPy emulation of a plausible wrong version, on the GPU tests' own
case lists — so that "the GPU test passes" means something before a GPU has run it."""
import ctypes as C
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import math_cases as cases
import math_probe as probe
import math_ref as R
from oracle import oracle_np as onp

F = np.float32


def _finite(*arrays):
    ok = np.ones(arrays[0].shape, bool)
    for a in arrays:
        ok &= np.isfinite(a)
    return ok


# ---- the references check themselves ------------------------------------------------------------------------------------
def test_denormals_are_on_in_numpy():
    assert F(1e-40) * F(0.5) == F(5e-41) and F(1e-38) / F(16.0) != 0


def test_fma32_equals_fraction_arithmetic():
    rng = np.random.default_rng(1)
    a, b = cases._rand_finite(rng, 3000), cases._rand_finite(rng, 3000)
    with np.errstate(all="ignore"):
        near = (-(a.astype(np.float64) * b.astype(np.float64)) * (1.0 + rng.integers(-3, 4, a.size) * 2.0 ** -24)).astype(np.float32)
        wide = (a.astype(np.float64) * b.astype(np.float64) * rng.uniform(-2, 2, a.size)).astype(np.float32)
    n = 0
    for c in (cases._rand_finite(rng, 3000)[:600], near[:1200], wide[:1200]):
        for aa, bb, cc in zip(a, b, c):
            if not (np.isfinite(float(aa) * float(bb)) and np.isfinite(cc)):
                continue
            got, ref = R.fma32(aa, bb, cc), R.fma32_fraction(aa, bb, cc)
            assert R.bits(got) == R.bits(ref), (aa, bb, cc, got, ref)
            n += 1
    assert n > 2500
    for aa, bb, cc in ((0.0, 1.0, -0.0), (-0.0, 1.0, -0.0), (1.0, 1.0, -1.0), (-1.0, 1.0, 1.0), (1e-30, 1e-30, 0.0), (-1e-30, 1e-30, 0.0)):
        assert R.bits(R.fma32(F(aa), F(bb), F(cc))) == R.bits(R.fma32_fraction(aa, bb, cc)), (aa, bb, cc)


def test_ieee_quotient_and_markstein_emulation_equal_fraction_arithmetic():
    """NumPy's fp32 division is the IEEE quotient, and the vectorised emulation of divu's three instructions is the sequence in
    exact rational arithmetic — on a subsample of the GPU test's own pairs, the ones outside the contract domain included."""
    x, d = cases.divu_cases()
    r, exact = probe.make_udiv(d)
    ok = np.nonzero(_finite(x, d, r) & (d != 0) & (exact != 0))[0]
    pick = ok[np.random.default_rng(2).choice(ok.size, 6000, replace=False)]
    q, m = R.ieee_div(x[pick], d[pick]), R.markstein(x[pick], d[pick], r[pick])
    for j, i in enumerate(pick):
        assert R.bits(q[j]) == R.bits(R.div_fraction(x[i], d[i])), (x[i], d[i])
        ref = R.markstein_fraction(x[i], d[i], r[i])
        assert R.bits(m[j]) == R.bits(ref) or (np.isnan(m[j]) and np.isnan(ref)), (x[i], d[i], m[j], ref)


def test_markstein_sequence_deviates_only_outside_the_contract_domain(capsys):
    """46 000 random pairs over divisors make_udiv marks exact: no mismatch with the IEEE quotient in the mid range; one-ulp errors
    for tiny numerators (the residual underflows); mismatches where the quotient is subnormal; NaN where a finite quotient
    overflows (divu) and the infinity there (divu_data).  Then two million pairs INSIDE the domain: none may differ."""
    rng = np.random.default_rng(46000)

    def pairs(n, xlo, xhi, dlo, dhi):
        def f(lo, hi):
            v = np.ldexp(1.0 + rng.integers(0, 2 ** 23, n) / 2.0 ** 23, rng.integers(lo, hi + 1, n)) * (1 - 2 * rng.integers(0, 2, n))
            return v.astype(np.float32)
        x, d = f(xlo, xhi), f(dlo, dhi)
        r, exact = probe.make_udiv(d)
        k = exact != 0
        return x[k], d[k], r[k], exact[k]

    counts = {}
    for name, rng_ in dict(mid=(-100, 100, -60, 60), tiny_x=(-149, -101, -20, 20), sub_q=(-126, -100, 0, 40), over_q=(100, 127, -40, -1)).items():
        x, d, r, exact = pairs(11500, *rng_)
        with np.errstate(all="ignore"):
            q64 = np.abs(x.astype(np.float64) / d.astype(np.float64))
        keep = {"mid": (q64 >= 2.0 ** -100) & (q64 <= 2.0 ** 100), "tiny_x": np.ones(x.size, bool),
                "sub_q": q64 < 2.0 ** -126, "over_q": q64 >= 2.0 ** 128}[name]
        x, d, r, exact = x[keep], d[keep], r[keep], exact[keep]
        m, q = R.markstein(x, d, r), R.ieee_div(x, d)
        bad = R._mismatch(m, q)
        counts[name] = (int(bad.sum()), int(x.size))
        if name == "mid":
            assert not bad.any()
            assert R.divu_domain(x, d, exact).all()
        else:
            assert bad.any(), name
            assert not (bad & R.divu_domain(x, d, exact)).any(), name
        if name == "tiny_x":
            ulps = np.abs(R.bits(m[bad]).astype(np.int64) - R.bits(q[bad]).astype(np.int64))
            assert ulps.max() == 1 and np.abs(x[bad]).max() < 2.0 ** -100
        if name == "over_q":
            assert np.isinf(q).all() and np.isnan(m).all()
            assert R._mismatch(R.divu_ref(x, d, r, exact, data=True), q).sum() == 0      # divu_data returns the infinity
    with capsys.disabled():
        print("\n[markstein emulation] mismatches / pairs: " + ", ".join(f"{k} {a}/{b}" for k, (a, b) in counts.items()))
    ex = R.markstein(F(3.8867717e-38), F(3.6379784e-12), probe.make_udiv([3.6379784e-12])[0][0])
    assert ex == F(1.06838776e-26) and R.ieee_div(F(3.8867717e-38), F(3.6379784e-12)) == F(1.06838784e-26)
    # inside the domain, boundaries weighted: numerators from 2^-100 up, quotients from 2^-126 to 2^126
    for xlo, xhi, dlo, dhi in ((-100, 127, -126, 126), (-100, -90, -30, 30), (-100, 20, 20, 60), (0, 127, -126, -60)):
        x, d, r, exact = pairs(500000, xlo, xhi, dlo, dhi)
        dom = R.divu_domain(x, d, exact)
        assert dom.sum() > 50000
        assert not (R._mismatch(R.markstein(x, d, r), R.ieee_div(x, d)) & dom).any()


def test_exp_and_pow_references_are_correctly_rounded():
    """The fp64 filter of exp_cr / pow_cr against mpmath for every input of a sample (the premise: libm's fp64 exp and pow are
    within 2^-48 of the truth), and every input the filter itself hands to mpmath."""
    rng = np.random.default_rng(3)
    xe = np.concatenate([rng.choice(cases.exp_full_cases(), 2500), rng.choice(cases.exp_small_cases(), 1500), cases.exp_full_cases()[-32:]])
    R.assert_bits_equal(R.exp_cr(xe), R.exp_mp(xe), "exp_cr vs mpmath", x=xe)
    px, py = cases.pow_cases()
    pick = rng.choice(px.size, 3000, replace=False)
    R.assert_bits_equal(R.pow_cr(px[pick], py[pick]), R.pow_mp(px[pick], py[pick]), "pow_cr vs mpmath", x=px[pick], y=py[pick])
    with mpmath.workprec(R.MP_PREC):
        for x in xe[:400]:
            if np.isfinite(x):
                rel = abs(mpmath.mpf(float(np.exp(np.float64(x)))) / mpmath.exp(mpmath.mpf(float(x))) - 1)
                assert rel < 2.0 ** -50, (x, rel)


def test_the_oracles_exp_and_pow_are_correctly_rounded_on_the_test_inputs():
    """oracle_np._exp / _pow round an fp64 libm value once; that is the correctly rounded fp32 result unless the fp64 value falls on
    the other side of an fp32 rounding boundary than the truth.  Any such input among the GPU tests' inputs is listed."""
    x = np.concatenate([cases.exp_full_cases(), cases.exp_small_cases()])
    with np.errstate(all="ignore"):
        got = onp._exp(x)
    R.assert_bits_equal(got, R.exp_cr(x), "oracle_np._exp vs correctly rounded", x=x)
    px, py = cases.pow_cases()
    with np.errstate(all="ignore"):
        gp = np.power(px.astype(np.float64), py.astype(np.float64)).astype(np.float32)      # _pow with a per-element exponent
        for y in cases.POW_EXPONENTS:
            k = py == F(y)
            assert np.array_equal(onp._pow(px[k], F(y)), gp[k])
    R.assert_bits_equal(gp, R.pow_cr(px, py), "oracle_np._pow vs correctly rounded", x=px, y=py)
    xi = cases.pow_identity_cases()
    with np.errstate(all="ignore"):
        R.assert_bits_equal(onp._pow(xi, F(1.0)), xi, "oracle_np._pow(x, 1)", x=xi)


def test_midpoint_distance_and_the_one_deviation_assert_exp_accepts(monkeypatch):
    """midpoint_distance_ulp64 on values whose distance is known, and every branch of assert_exp's rule: a result that differs from
    the correctly rounded one is accepted only if exp(x) is within one fp64 ulp of an fp32 rounding boundary AND the result is the
    neighbouring fp32; the accepted inputs are returned (and printed)."""
    # exp(0) = 1 sits ON an fp32 value: half an fp32 ulp = 2^28 fp64 ulps from the boundary above, 2^27 from the one below
    assert R.midpoint_distance_ulp64(np.array([0.0], np.float32))[0] == 2.0 ** 28
    d = R.midpoint_distance_ulp64(np.array([1.0, -1.0, 0.5, 88.0], np.float32))
    assert (d > 1e3).all() and (d <= 2.0 ** 28).all()
    x = np.array([1.0, 0.5, -2.0], np.float32)
    ref = R.exp_cr(x)
    up = np.nextafter(ref, np.float32(np.inf))
    with pytest.raises(AssertionError, match="fp64 ulps from"):                      # far from a boundary: a neighbour is still wrong
        R.assert_exp(np.array([ref[0], up[1], ref[2]], np.float32), x, "neighbour, easy input")
    monkeypatch.setattr(R, "midpoint_distance_ulp64", lambda v: np.full(np.asarray(v).size, 0.75))
    listed = R.assert_exp(np.array([ref[0], up[1], ref[2]], np.float32), x, "neighbour, hard input")
    assert len(listed) == 1 and listed[0][0] == 0.5                                 # within an ulp of a boundary, neighbour: accepted, listed
    two = np.nextafter(up, np.float32(np.inf))
    with pytest.raises(AssertionError):                                              # within an ulp, but two fp32 away: rejected
        R.assert_exp(np.array([ref[0], two[1], ref[2]], np.float32), x, "two ulps off, hard input")
    monkeypatch.setattr(R, "midpoint_distance_ulp64", lambda v: np.full(np.asarray(v).size, 1.25))
    with pytest.raises(AssertionError):                                              # a neighbour, but more than an ulp from the boundary
        R.assert_exp(np.array([ref[0], up[1], ref[2]], np.float32), x, "neighbour, 1.25 ulps")
    with pytest.raises(AssertionError):                                              # a NaN / inf input has no such excuse
        R.assert_exp(np.array([0.0], np.float32), np.array([np.nan], np.float32), "exp(NaN) = 0")


def test_clamp_and_half_references():
    nan = F(np.nan)
    assert R.sat_ref(nan) == 0 and not np.signbit(R.sat_ref(nan))
    assert R.bits(R.sat_ref(F(-0.0))) == 0 and R.bits(R.sat_ref(F(0.0))) == 0              # fmaxf(-0, +0) = +0 (-0 < +0)
    assert R.clamp_ref(nan, F(0.5), F(2.0)) == F(0.5) and R.clamp_ref(F(3.0), F(0.5), F(0.5)) == F(0.5)
    assert R.clamp_ref(F(np.inf), F(0.0), F(1.0)) == 1 and R.clamp_ref(F(-np.inf), F(0.0), F(1.0)) == 0
    x, lo, hi = cases.clamp_cases()
    fin = ~np.isnan(x)
    with np.errstate(all="ignore"):
        assert np.array_equal(R.clamp_ref(x, lo, hi)[fin], np.minimum(np.maximum(x, lo), hi)[fin])
        assert np.array_equal(R.sat_ref(cases.sat_cases()), onp._sat(cases.sat_cases()))   # the oracle's saturate, values
    assert R.half_ref(F(65519.996)) == np.float16(65504.0) and np.isinf(R.half_ref(F(65520.0)))
    assert R.half_ref(F(2.0 ** -25)) == 0 and R.half_ref(F(2.0 ** -25 * 1.0000001)) == np.float16(2.0 ** -24)


# ---- host helpers of the library ------------------------------------------------------------------------------------------
def test_make_udiv_reciprocal_and_exact_flag():
    """r == RN(1 / d) bit for bit and ``exact`` as documented (d normal, r normal, significand not all ones) for > 2^16 divisors."""
    d = np.concatenate([cases.divisors(), cases.divisors_in_use()])
    assert d.size >= 2 ** 16
    r, exact = probe.make_udiv(d)
    R.assert_bits_equal(r, R.rn_recip(d), "make_udiv: r vs RN(1/d)", d=d)
    want = R.udiv_exact_documented(d)
    assert np.array_equal(exact, want), d[exact != want][:8]
    # the classes the sweep must contain, each with the flag it must get
    b = R.bits(d)
    expo = (b >> 23) & 0xFF
    assert set(np.unique(expo)) == set(range(256))
    allones = (b & 0x7FFFFF) == 0x7FFFFF
    for name, mask, flag in (("all-ones significand", allones & (expo > 0) & (expo < 255), 0), ("denormal", (expo == 0) & (d != 0), 0),
                             ("zero", d == 0, 0), ("inf", np.isinf(d), 0), ("nan", np.isnan(d), 0),
                             ("reciprocal denormal", np.isfinite(d) & (np.abs(d) > F(2.0 ** 126)), 0),
                             ("power of two", ((b & 0x7FFFFF) == 0) & (expo > 2) & (expo < 252), 1),
                             ("all ones minus one", ((b & 0x7FFFFF) == 0x7FFFFE) & (expo > 2) & (expo < 252), 1),
                             ("in use", np.isin(d, cases.divisors_in_use()) & ~allones, 1)):
        assert mask.sum() >= 1, name
        assert (exact[mask] == flag).all(), name
    with np.errstate(all="ignore"):
        assert (np.isinf(r[(expo == 0) & (np.abs(d) < F(2.0 ** -128)) & (d != 0)])).all()      # the reciprocal overflows
    # 1/d for a sample through exact rational arithmetic
    ok = np.nonzero(np.isfinite(d) & (d != 0))[0][::23]
    for i in ok:
        assert R.bits(r[i]) == R.bits(R.div_fraction(1.0, d[i])), d[i]


def test_fill_exp_consts_are_the_rounded_constants():
    c = probe.exp_consts()
    with mpmath.workprec(400):
        assert c[0] == float(1 / mpmath.log(2))                                      # RN(log2 e)
        ln2 = mpmath.log(2)
        hi, lo = c[1], c[2]
        man, _ = math.frexp(hi)
        assert (int(man * 2 ** 53) & ((1 << 20) - 1)) == 0                           # 33 significant bits: k * ln2hi is exact for |k| < 2^20
        assert lo == float(ln2 - mpmath.mpf(hi))                                     # RN(ln 2 - ln2hi)
        assert abs(mpmath.mpf(hi) + mpmath.mpf(lo) - ln2) <= mpmath.mpf(2) ** -85                     # half an ulp of ln2lo
    for i in range(13):
        assert c[3 + i] == float(Fraction(1, math.factorial(13 - i))), i             # RN(1 / k!), k = 13 .. 1
    # the literal forms of mrirt_device.h use the same values: checked on the device (constants form == literal form everywhere)


def test_fill_camera_equals_the_oracle():
    rng = np.random.default_rng(5)
    eye, U, V, W = (rng.normal(size=3).astype(np.float32) for _ in range(4))
    for fov in cases.FOV_CASES:
        for w, h, k3 in cases.ASPECT_CASES:
            cam = probe.fill_camera(eye, U, V, W, fov, w, h, k3=k3)
            R.assert_camera(cam, fov, w, h, k3=k3, what=f"fill_camera(fov={fov}, {w}x{h}, k3={k3})")
            assert cam["mode"][0] == 0 and cam["width"][0] == w and cam["height"][0] == h
            for name, v in (("eye", eye), ("U", U), ("V", V), ("W", W)):
                assert np.array_equal(cam[name][0], v)
    cam = probe.fill_camera(eye, U, V, W, F(0.8), 17, 33, ext=(1, F(1.1)))
    assert cam["mode"][0] == 1 and cam["orthoHalfHeight"][0] == F(1.1)


def test_k1args_blocks_carry_the_hosts_constants():
    p = cases.composite_cases(False)["params"]
    blocks = probe.fill_k1args(p)
    assert blocks.shape == (p.shape[0], probe.lib().probe_sizeof(1)) and blocks.any()
    # expSmall is set exactly where |intensityAlpha * stepSize| <= 1/8 in fp32: both sides are among the cases
    small = np.abs(p[:, 4] * p[:, 5]) <= F(0.125)
    assert small.any() and (~small).any()


def test_a_nan_intensity_alpha_is_refused_on_the_host():
    """exp_f64_to_f32 clamps its argument with fmax / fmin, which drop a NaN: the device would return exp(-200) = 0 where the
    oracle's (float)exp((double)NaN) is NaN.  The only way a NaN reaches that argument is a NaN intensityAlpha (a NaN val fails
    `val > 0`, a NaN stepSize is refused already), so prepare() refuses it."""
    import mrirt
    from mrirt import params, synth
    lib = mrirt._lib.lib()
    good = synth.brats_scene(32, 64, 64, channels=1)
    dummy = C.c_void_p(0x1000)
    vp = (C.c_void_p * 4)(dummy, None, None, None)
    P = params.brats_params(dict(good, intensityAlpha=float("nan")))
    assert lib.mrirt_render_brats_ex(C.byref(P), None, vp, None, None, dummy, 64, None, None) == -5
    assert lib.mrirt_brats_sample_counts(C.byref(P), None, dummy, None) == -5
    # a camera that is not finite makes NaN rays: refused like the other parameters that are not finite
    for key in ("U", "V", "W"):
        for bad in (float("nan"), float("inf")):
            v = np.array(good[key], dtype=np.float32)
            v[1] = bad
            P = params.brats_params(dict(good, **{key: v}))
            assert lib.mrirt_render_brats_ex(C.byref(P), None, vp, None, None, dummy, 64, None, None) == -5, (key, bad)
    P = params.brats_params(dict(good, fovY=float("nan")))
    assert lib.mrirt_render_brats_ex(C.byref(P), None, vp, None, None, dummy, 64, None, None) == -5


def test_composite_reference_is_the_oracles_inner_step():
    """math_ref.composite_step restates the lines of oracle_np.brats_main between the modality blend and the overlays; here one-pixel
    frames whose ray takes exactly one sample of a linear-ramp volume go through brats_main itself and must give the same colour and
    transmittance — with shading on and off, and with gamma == 1 and != 1, each at least twice."""
    from mrirt import synth
    dims = (4, 4, 4)
    rng = np.random.default_rng(6)
    seen = {}
    for trial in range(24):
        shade, gamma = bool(trial % 2), F((1.0, 0.6, 2.2)[trial % 3])
        val = F(rng.uniform(0.1, 0.9))
        vols = [np.full(64, val * F(1 + m), np.float32) for m in range(4)]
        p = synth.brats_scene(0, 0, 96, dims=dims, image_hw=(1, 1), channels=2 + trial % 2, intensity_alpha=float(rng.uniform(1, 40)))
        p = dict(p, gamma=gamma, ww=F(rng.uniform(0.5, 3.0)), wl=F(rng.uniform(0.2, 1.0)), volWeight=rng.uniform(0.1, 1.0, 4).astype(np.float32))
        ext = dict(synth.SHADE_EXT) if shade else None
        vs = np.asarray(p["voxelSize"], np.float32)
        diag = float(np.linalg.norm(vs * np.array(dims, np.float32)))
        p = dict(p, stepSize=F(diag * 1.01), bgColor=(0.25, 0.25, 0.25))
        out, aux = onp.brats_main(p, vols, None, None, ext, return_aux=True)
        if aux["live_samples"] != 1:
            continue
        en = [int(v) for v in p["volEnabled"]]
        wt = np.asarray(p["volWeight"], np.float32)
        v, wsum = F(0.0), F(0.0)
        for m in range(4):
            if en[m]:
                v = v + vols[m][0] * wt[m]
                wsum = wsum + wt[m]
        e = dict(onp.DEFAULT_EXT)
        e.update(ext or {})
        one = lambda a: np.array([a], np.float32)
        pp = dict(ww=one(p["ww"]), wl=one(p["wl"]), gamma=one(p["gamma"]), wsum=one(wsum), intensityAlpha=one(p["intensityAlpha"]),
                  stepSize=one(p["stepSize"]), ka=one(e["ka"]), kd=one(e["kd"]), ks=one(e["ks"]), gradEps=one(e["gradEps"]),
                  specPow2=one(e["specPow2"]), hx=one(F(0.5) / vs[0]), hy=one(F(0.5) / vs[1]), hz=one(F(0.5) / vs[2]))
        # a constant volume: the lattice gradient is exactly 0, so the shaded sample takes the ka + kd branch
        Cc, T, nl, ns = R.composite_step(pp, one(v), np.zeros((1, 3), np.float32), np.array([[0, 0, 1]], np.float32), one(0.25), one(1.0),
                                         shade=shade)
        assert R.bits(Cc[0]) == R.bits(out[0, 0, 0]) and R.bits(T[0]) == R.bits(aux["T"][0, 0]), (trial, Cc, out[0, 0], T, aux["T"])
        assert ns[0] == aux["shaded_samples"] and T[0] < 1.0
        seen[(shade, bool(gamma != 1))] = seen.get((shade, bool(gamma != 1)), 0) + 1
    for key in ((False, False), (False, True), (True, False), (True, True)):
        assert seen.get(key, 0) >= 2, (key, seen)


# ---- sensitivity: the assertion helpers fail on plausible wrong versions ------------------------------------------------------
def test_divu_helper_fails_without_the_correction_step():
    x, d = cases.divu_cases()
    r, exact = probe.make_udiv(d)
    right = R.divu_ref(x, d, r, exact, data=False)
    dom = R.assert_divu(right, x, d, r, exact, data=False, what="emulated divu")
    assert dom.sum() > x.size // 4
    R.assert_divu(R.divu_ref(x, d, r, exact, data=True), x, d, r, exact, data=True, what="emulated divu_data")
    with np.errstate(all="ignore"):
        wrong = np.where(exact != 0, R.mul32(x, r), R.ieee_div(x, d)).astype(np.float32)    # q = x r, no residual
    with pytest.raises(AssertionError, match="contract domain"):
        R.assert_divu(wrong, x, d, r, exact, data=False, what="x * r")
    # ... also on the divisors in use alone (255 and the bytes, voxel sizes, ww)
    k = np.isin(d, cases.divisors_in_use())
    with pytest.raises(AssertionError, match="contract domain"):
        R.assert_divu(wrong[k], x[k], d[k], r[k], exact[k], data=False, what="x * r, divisors in use")
    # divu_data's select dropped: a NaN where the quotient is an infinity
    with pytest.raises(AssertionError):
        R.assert_divu(right, x, d, r, exact, data=True, what="divu as divu_data")
    # the compiler contracting q + e r differently: residual computed unfused
    with np.errstate(all="ignore"):
        q = R.mul32(x, r)
        unf = np.where(exact != 0, R.fma32(x - q * d, r, q), R.ieee_div(x, d)).astype(np.float32)
    with pytest.raises(AssertionError):
        R.assert_divu(unf, x, d, r, exact, data=False, what="unfused residual")


def test_lerp_helper_fails_on_a_fused_strict_lerp_and_the_cases_are_not_vacuous():
    a, b, t = cases.lerp_cases()
    strict, fast = R.lerp_strict(a, b, t), R.lerp_fast(a, b, t)
    share = float(R._mismatch(strict, fast).mean())
    assert share >= 0.10, share                                   # fused and unfused differ on at least 10 % of the inputs
    with pytest.raises(AssertionError):
        R.assert_bits_equal(fast, strict, "fused lerp as STRICT", a=a, b=b, t=t)
    with pytest.raises(AssertionError):
        R.assert_bits_equal(strict, fast, "unfused lerp as FAST", a=a, b=b, t=t)
    c, f = cases.trilerp_cases()
    ts, tf = R.trilerp(R.lerp_strict, c, f), R.trilerp(R.lerp_fast, c, f)
    assert float(R._mismatch(ts, tf).mean()) >= 0.10
    with pytest.raises(AssertionError):
        R.assert_bits_equal(tf, ts, "fused trilerp as STRICT")


def test_exp_helper_fails_on_a_short_polynomial_and_on_exp_small_out_of_range():
    consts = probe.exp_consts()
    rng = np.random.default_rng(7)
    full = cases.exp_full_cases()
    x = np.concatenate([rng.choice(full[np.isfinite(full)], 1500), full[-14:]])
    x = x[np.isfinite(x)]
    assert not R.assert_exp(R.exp_device_emulation(x, consts), x, "emulated exp")                    # the right version passes
    with pytest.raises(AssertionError):
        R.assert_exp(R.exp_device_emulation(x, consts, steps_short=1), x, "Horner loop one step short")
    xs = rng.choice(cases.exp_small_cases(), 1500)
    xs = xs[cases.exp_small_domain(xs)]
    assert not R.assert_exp(R.exp_device_emulation(xs, consts, small=True), xs, "emulated exp_small")
    with pytest.raises(AssertionError):
        R.assert_exp(R.exp_device_emulation(xs, consts, small=True, steps_short=1), xs, "exp_small one step short")
    # exp_small where it does not belong: visible as soon as x^11 / 11! reaches fp32 resolution
    wide = rng.uniform(-1.0, 1.0, 1500).astype(np.float32)
    with pytest.raises(AssertionError):
        R.assert_exp(R.exp_device_emulation(wide, consts, small=True), wide, "exp_small on |x| <= 1")


def test_what_no_fp32_test_can_see_in_the_exp_polynomials():
    """Two of the wrong versions one would like to catch are NOT wrong in fp32, and the tests say so instead of pretending: the
    LEADING term of either polynomial, and exp_small a few ulps above 1/8, change exp(x) by less than half an fp64 ulp (2^-53
    relative), i.e. they move an fp32 result only where the fp64 value sits within an fp64 ulp of an fp32 rounding boundary —
    the one deviation assert_exp accepts.  Computed exactly here, so that the 1/8 switch is known to be conservative."""
    half_ulp64 = Fraction(1, 2 ** 53)
    r = Fraction(math.log(2) / 2) + Fraction(1, 2 ** 40)                              # |x - k ln2| <= ln2 / 2
    assert r ** 13 / math.factorial(13) < 2 * half_ulp64                             # the full form's leading term: ~1.7e-16
    x = Fraction(1, 8) + 64 * Fraction(1, 2 ** 27)                                    # 64 fp32 ulps above 1/8
    tail = sum(x ** k / math.factorial(k) for k in range(11, 30))
    assert tail < half_ulp64 / 30                                                     # exp_small there: 3e-18
    assert Fraction(1, 8) ** 10 / math.factorial(10) < 3 * half_ulp64                 # exp_small's leading term: ~2.6e-16
    x = np.float32(0.125) + np.arange(1, 65, dtype=np.float32) * np.float32(2.0 ** -27)
    assert not R.assert_exp(R.exp_device_emulation(x, probe.exp_consts(), small=True), x, "exp_small just above 1/8")


def test_half_helper_fails_on_truncation():
    x = cases.half_cases()
    R.assert_half(R.half_ref(x), x, "astype(float16)")
    with pytest.raises(AssertionError):
        R.assert_half(R.half_truncating(x), x, "truncating conversion")
    fin = np.isfinite(x) & (np.abs(x) < 65504)
    t = R.half_truncating(x[fin]).astype(np.float32)
    assert (np.abs(t) <= np.abs(x[fin])).all()


def test_clamp_helper_fails_on_the_wrong_nan_result():
    x, lo, hi = cases.clamp_cases()
    R.assert_clamp(R.clamp_ref(x, lo, hi), x, lo, hi, "fminf(fmaxf())")
    with np.errstate(all="ignore"):
        propagating = np.minimum(np.maximum(x, lo), hi)                               # NaN in, NaN out
    with pytest.raises(AssertionError):
        R.assert_clamp(propagating, x, lo, hi, "NaN-propagating clamp")
    with pytest.raises(AssertionError):
        R.assert_clamp(np.where(np.isnan(x), hi, R.clamp_ref(x, lo, hi)), x, lo, hi, "clamp(NaN) = hi")


def test_camera_helper_fails_on_the_wrong_aspect_ratio():
    eye, U, V, W = (np.eye(3, dtype=np.float32)[k % 3] for k in range(4))
    failed = 0
    for w, h, k3 in cases.ASPECT_CASES:
        cam = probe.fill_camera(eye, U, V, W, F(0.8), w, h, k3=not k3)                # K1's aspect ratio for K3 and vice versa
        try:
            R.assert_camera(cam, F(0.8), w, h, k3=k3, what="swapped aspect")
        except AssertionError:
            failed += 1
    assert failed == sum(1 for w, h, k3 in cases.ASPECT_CASES if h == 0)               # they differ exactly where height < 1
    # the rays themselves: a different aspect ratio moves every off-axis direction
    c = cases.camera_cases()[6]
    ro, rd = R.rays_ref(17, 33, c["fovY"], c["eye"], c["U"], c["V"], c["W"])
    ro2, rd2 = R.rays_ref(33, 17, c["fovY"], c["eye"], c["U"], c["V"], c["W"])
    with pytest.raises(AssertionError):
        R.assert_rays(ro, rd, ro, np.ascontiguousarray(rd2.transpose(1, 0, 2)), "transposed image size")
    assert (rd[:, 8, 0] == 0).all() and (rd[16, :, 1] == 0).all()                      # axis-aligned basis: zero components on the centre lines


def test_probe_is_built_with_the_products_flags():
    import mrirt
    flags = mrirt._lib.HIPCC_FLAGS
    assert "-ffp-contract=off" in flags and "-O3" in flags and "--offload-arch=gfx950" in flags
    so = probe.build()
    assert so.exists() and so.parent.name == "_build"
    src = (probe.SRC).read_text()
    assert "asm" not in src.replace("assembly", "")
