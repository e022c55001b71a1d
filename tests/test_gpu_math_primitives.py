"""The device math primitives of csrc/mrirt_device.h, csrc/brats_device.h and csrc/siren_sincos.h, each run ON ITS OWN through the probe library
(tests/native/math_probe.hip, built with the product's flags) and compared bit for bit with the exact references of
tests/math_ref.py on the case lists of tests/math_cases.py.  No assertion on a STRICT function has a tolerance.  The same
assertion helpers are shown to fail on plausible wrong versions, without a GPU, in tests/test_math_ref_host.py."""
import numpy as np
import pytest

import inr_siren_ref as sr
import math_cases as cases
import math_probe as probe
import math_ref as R

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "needs cuda:0"
    torch.cuda.set_device(0)
    probe.lib()
    yield


# ---- division ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", [False, True], ids=["divu", "divu_data"])
def test_strict_division_is_the_ieee_quotient_on_its_domain_and_the_exact_sequence_everywhere(data):
    x, d = cases.divu_cases()
    r, exact = probe.make_udiv(d)
    got = probe.divu(x, d, strict=True, data=data)
    dom = R.assert_divu(got, x, d, r, exact, data=data, what="M<true>::divu_data" if data else "M<true>::divu")
    assert dom.sum() > x.size // 4
    # the divisors in use lie in the domain with every numerator a frame can produce: bytes over 255 are the IEEE quotients
    with np.errstate(all="ignore"):
        k = (d == F(255.0)) & ~np.signbit(x) & (x <= 255) & (x == np.floor(x))
    assert k.sum() >= 256 and dom[k].all()


def test_fast_division_is_one_rounded_product():
    x, d = cases.divu_cases()
    r, _ = probe.make_udiv(d)
    for data in (False, True):
        R.assert_bits_equal(probe.divu(x, d, strict=False, data=data), R.mul32(x, r), "M<false>::divu vs RN(x r)", x=x, d=d)


# ---- exp --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exp_runs():
    xf, xs = cases.exp_full_cases(), cases.exp_small_cases()
    return dict(xf=xf, xs=xs, ref_f=R.exp_cr(xf), ref_s=R.exp_cr(xs),
                full=[probe.exp(xf, 0), probe.exp(xf, 1)], full_on_small=[probe.exp(xs, 0), probe.exp(xs, 1)],
                small=[probe.exp(xs, 2), probe.exp(xs, 3)])


def test_exp_constants_form_equals_literal_form_everywhere(exp_runs):
    R.assert_bits_equal(exp_runs["full"][0], exp_runs["full"][1], "exp(x, consts) vs exp_lit(x)", x=exp_runs["xf"])
    R.assert_bits_equal(exp_runs["full_on_small"][0], exp_runs["full_on_small"][1], "exp(x, consts) vs exp_lit(x), small x", x=exp_runs["xs"])
    R.assert_bits_equal(exp_runs["small"][0], exp_runs["small"][1], "exp_small(x, consts) vs exp_small_lit(x)", x=exp_runs["xs"])


def test_exp_small_equals_the_full_form_on_its_domain(exp_runs):
    """The host switches between the two per launch (intensityAlpha * stepSize <= 1/8): the switch must never change a frame."""
    xs = exp_runs["xs"]
    k = cases.exp_small_domain(xs)
    assert k.sum() > 2 ** 18 and (~k).sum() >= 128
    R.assert_bits_equal(exp_runs["small"][0][k], exp_runs["full_on_small"][0][k], "exp_small vs exp, |x| <= 1/8", x=xs[k])


def test_exp_is_correctly_rounded(exp_runs):
    """Every form against the correctly rounded value, no input left out (clamp ends, +-0, +-denormal, +-inf, denormal results).  A
    differing input is accepted only with mpmath's proof that exp(x) lies within one fp64 ulp of an fp32 rounding boundary, and
    is printed."""
    for name, got in (("exp", exp_runs["full"][0]), ("exp_lit", exp_runs["full"][1])):
        R.assert_exp(got, exp_runs["xf"], name, ref=exp_runs["ref_f"])
    for name, got in (("exp, small x", exp_runs["full_on_small"][0]), ("exp_small", exp_runs["small"][0]), ("exp_small_lit", exp_runs["small"][1])):
        R.assert_exp(got, exp_runs["xs"], name, ref=exp_runs["ref_s"])
    xf, got = exp_runs["xf"], exp_runs["full"][0]
    den = (exp_runs["ref_f"] > 0) & (exp_runs["ref_f"] < F(1.1754944e-38))
    assert den.sum() > 2 ** 13                                       # the denormal results were really there
    assert got[xf == F(-np.inf)] == 0 and np.isinf(got[xf == F(np.inf)]) and (got[xf == 0] == 1).all()


def test_exp_of_a_nan_is_pinned():
    """Outside the contract: the full forms clamp their argument with fmax / fmin, which drop a NaN, so exp(NaN) = exp(-200) = 0
    where (float)exp((double)NaN) is NaN (prepare() refuses the one parameter that could put a NaN there); exp_small has no
    clamp and returns the NaN."""
    nan = cases._from_bits(np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F800001], np.uint32))
    for form in (0, 1):
        assert np.array_equal(R.bits(probe.exp(nan, form)), np.zeros(4, np.uint32)), form
    for form in (2, 3):
        assert np.isnan(probe.exp(nan, form)).all(), form


# ---- pow --------------------------------------------------------------------------------------------------------------
def test_strict_pow_is_correctly_rounded():
    x, y = cases.pow_cases()
    R.assert_bits_equal(probe.pow_strict(x, y), R.pow_cr(x, y), "M<true>::pow", x=x, y=y)


def test_pow_with_exponent_one_returns_its_argument():
    x = cases.pow_identity_cases()
    got = probe.pow_strict(x, np.ones_like(x))
    assert np.array_equal(R.bits(got), R.bits(x)), x[R.bits(got) != R.bits(x)][:8]        # NaN payloads and signs included


# ---- the SIREN step's sine and cosine ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.SINCOS_SETS))
def test_siren_sincos_has_the_bits_of_its_restatement(name):
    """siren_sincos, one thread per argument, on the argument sets of inr_siren_ref.py: the sweep of the CPU test, every fp32 of
    [2^19, 2^20] in both signs, every quadrant switch of the domain with two neighbours on each side, +-0 / denormals / powers
    of two / the domain's edge, and beyond the domain with infinities and NaNs.  Sine and cosine have the BIT PATTERNS of the
    NumPy restatement (the sign of zero included; NaN exactly where it has one) and, inside the domain, the by-value figures
    of the CPU test hold for the device's own results."""
    a, want_s, want_c = sr.sincos_set(name)
    s, c = probe.siren_sincos(a)
    if name in sr.INSIDE_SETS:
        sr.assert_libm_figures(name, "device", a, s, c)
    for what, got, want in (("sin", s, want_s), ("cos", c, want_c)):
        bad = sr.bits_differ(got, want)
        print(f"device {name} {what}: {bad.size} of {a.size} bit patterns differ from the restatement")
        assert bad.size == 0, (what, bad[:6], a[bad[:6]], got[bad[:6]], want[bad[:6]])
    if name == "outside":
        fin = np.isfinite(a)
        assert (s[fin].view(np.uint32) == 0).all() and (c[fin] == 1).all() and np.isnan(s[~fin]).all() and np.isnan(c[~fin]).all()
    if name == "small_and_special":
        den = (np.abs(a) < F(2.0 ** -126)) & (a != 0)
        assert den.sum() > 4000 and np.array_equal(s[den].view(np.uint32), a[den].view(np.uint32))         # denormals pass through
        assert (s[a == 0].view(np.uint32) == 0).all()                                                    # sin(-0) = +0


# ---- clamp ------------------------------------------------------------------------------------------------------------
def test_clampf_and_satf():
    """clampf, with bounds from memory and with the K3 march's literal bounds, against fminf(fmaxf(x, lo), hi) on every case: +-0,
    +-inf, denormals, values equal to the bounds, lo == hi, and NaN — a quiet NaN gives lo (HLSL's rule), a signalling NaN gives hi
    (IEEE 754-2008 maxNum / minNum; math_ref.clamp_ref).  satf gives 0 for every NaN."""
    x, lo, hi = cases.clamp_cases()
    nan = np.isnan(x)
    assert (nan & R.is_signalling_nan(x)).sum() >= 13 and (nan & ~R.is_signalling_nan(x)).sum() >= 26
    R.assert_clamp(probe.clampf(x, lo, hi), x, lo, hi, "clampf")
    xk = np.concatenate([x, np.array([0.01, 0.25, 0.0099999998, 0.25000003, 0.1], np.float32)])
    R.assert_clamp(probe.clampf_k3(xk), xk, np.full(xk.size, 0.01, np.float32), np.full(xk.size, 0.25, np.float32), "clampf(x, 0.01f, 0.25f)")
    xs = cases.sat_cases()
    assert R.is_signalling_nan(xs).any() and (np.isnan(xs) & ~R.is_signalling_nan(xs)).any()
    R.assert_bits_equal(probe.satf(xs), R.sat_ref(xs), "satf", x=xs)


# ---- lerp -------------------------------------------------------------------------------------------------------------
def test_lerp_strict_is_unfused_and_fast_is_one_fma():
    a, b, t = cases.lerp_cases()
    R.assert_bits_equal(probe.lerp(a, b, t, strict=True), R.lerp_strict(a, b, t), "M<true>::lerp", a=a, b=b, t=t)
    R.assert_bits_equal(probe.lerp(a, b, t, strict=False), R.lerp_fast(a, b, t), "M<false>::lerp", a=a, b=b, t=t)


def test_packed_lerp_equals_the_scalar_one_per_lane():
    a, b, t = cases.lerp_cases()
    n = (a.size // 2) * 2
    a2, b2 = a[:n].reshape(-1, 2), b[:n].reshape(-1, 2)
    t2 = t[:n:2].copy()
    for strict, ref in ((True, R.lerp_strict), (False, R.lerp_fast)):
        got = probe.lerp2(a2, b2, t2, strict=strict)
        R.assert_bits_equal(got, ref(a2, b2, t2[:, None]), f"lerp2<{strict}> vs reference")
        if strict:
            scalar = probe.lerp(a2.reshape(-1), b2.reshape(-1), np.repeat(t2, 2), strict=True).reshape(-1, 2)
            R.assert_bits_equal(got, scalar, "lerp2<true> vs M<true>::lerp per lane")


def test_packed_trilerp_equals_the_scalar_one_and_the_reference():
    c, f = cases.trilerp_cases()
    for strict, ref in ((True, R.lerp_strict), (False, R.lerp_fast)):
        got = probe.trilerp2(c, f, strict=strict)
        want = R.trilerp(ref, c, f)
        R.assert_bits_equal(got[:, :2], want, f"trilerp2<{strict}> vs reference")
        R.assert_bits_equal(got[:, 2:], want, f"trilerp<{strict}> vs reference")
        R.assert_bits_equal(got[:, :2], got[:, 2:], f"trilerp2<{strict}> vs scalar trilerp per lane")


# ---- rays ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.IMAGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_primary_ray_equals_the_oracles_rays(size):
    w, h = size
    for i, c in enumerate(cases.camera_cases()):
        ext = None if c["ortho"] is None else (1, c["ortho"])
        cam = probe.fill_camera(c["eye"], c["U"], c["V"], c["W"], c["fovY"], w, h, ext=ext, k3=c["k3"])
        ro, rd = probe.primary_ray(cam)
        ref_ro, ref_rd = R.rays_ref(w, h, c["fovY"], c["eye"], c["U"], c["V"], c["W"], ortho=c["ortho"], k3=c["k3"])
        R.assert_rays(ro, rd, ref_ro, ref_rd, f"camera {i} at {w}x{h}")


# ---- stores and counters ------------------------------------------------------------------------------------------------
def test_half_store_rounds_to_nearest_even_at_the_right_index():
    x = cases.half_cases()
    rgba = x.reshape(-1, 4)
    for offset in (0, 3):
        buf = probe.store_rgba(rgba, half=True, offset=offset, fill=0xAB)
        R.assert_half(buf[offset:offset + rgba.shape[0]], rgba, f"store_rgba<true> at texel offset {offset}")
        guard = np.full(4, 0xABAB, np.uint16)
        assert (buf[:offset].view(np.uint16) == 0xABAB).all() and np.array_equal(buf[-1].view(np.uint16), guard)
    buf = probe.store_rgba(rgba, half=False, offset=5, fill=0xCD)
    R.assert_bits_equal(buf[5:-1], rgba, "store_rgba<false>")
    assert (buf[:5].view(np.uint32) == 0xCDCDCDCD).all() and (buf[-1].view(np.uint32) == 0xCDCDCDCD).all()


def test_wave_count_add_is_the_uint64_sum():
    for name, v in cases.wave_count_cases().items():
        assert probe.wave_count(v) == int(v.astype(np.uint64).sum()), name


# ---- one sample's cell ------------------------------------------------------------------------------------------------------
def test_strict_locate_equals_the_oracles_cell_and_fractions():
    """o + t d, the voxel-size quotient, the clamp, the floor and the fraction against the oracle's (p - volMin) / voxelSize,
    min(max()), floor and c - floor(c)."""
    c = cases.locate_cases()
    q, cell, f = probe.locate(c["params"], c["sel"], c["ro"], c["rd"], c["t"], strict=True)
    p = c["params"][c["sel"]]
    rq, rcell, rf = R.locate_ref(p[:, 0:3], p[:, 3:6], p[:, 6:9], c["ro"], c["rd"], c["t"])
    assert (rq < 0).mean() > 0.005 and (rq > p[:, 6:9] - 1).mean() > 0.005 and (rf == 0).mean() > 0.02     # both clamps, lattice planes
    R.assert_bits_equal(q, rq, "locate: pIdx")
    assert np.array_equal(cell, rcell), np.nonzero(cell != rcell)[0][:8]
    R.assert_bits_equal(f, rf, "locate: fractions")


# ---- one compositing step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shade,gamma1", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "shade", "plain-gamma1", "shade-gamma1"])
def test_strict_composite_equals_the_oracles_step(shade, gamma1):
    c = cases.composite_cases(gamma1)
    combo = probe.COMBOS.index((True, shade, gamma1))
    out, cnt = probe.composite(combo, c["params"], c["sel"], c["v"], c["g"], c["rd"], c["c0"], c["t0"])
    p = {k: c["params"][c["sel"], i] for i, k in enumerate(probe.K1_FIELDS)}
    C, T, n_live, n_shaded = R.composite_step(p, c["v"], c["g"], c["rd"], c["c0"], c["t0"], shade=shade)
    # the cases are what they claim to be
    changed = T != c["t0"]
    assert 0.3 < changed.mean() < 0.99 and (C == c["c0"]).any()
    small = np.abs(p["intensityAlpha"] * p["stepSize"]) <= F(0.125)
    assert 0.1 < small.mean() < 0.9
    for ch in range(3):
        R.assert_bits_equal(out[:, ch], C, f"composite C{ch}", v=c["v"], sel=c["sel"])
    R.assert_bits_equal(out[:, 3], T, "composite T", v=c["v"], sel=c["sel"])
    assert np.array_equal(cnt[:, 0].astype(np.uint32), n_live) and np.array_equal(cnt[:, 1].astype(np.uint32), n_shaded)


@pytest.mark.parametrize("shade,gamma1", [(False, False), (True, True)], ids=["plain", "shade-gamma1"])
def test_fast_composite_runs_and_counts(shade, gamma1):
    """FAST's transcendentals (v_exp_f32, v_log_f32, v_rcp_f32) have no derivable per-sample bound (their bar stays the frame-level
    one); what is exact is the sample counter, and that a saturated sample stays finite and inside [0, T]."""
    c = cases.composite_cases(gamma1)
    out, cnt = probe.composite(probe.COMBOS.index((False, shade, gamma1)), c["params"], c["sel"], c["v"], c["g"], c["rd"], c["c0"], c["t0"])
    assert (cnt[:, 0] == 1).all() and np.isfinite(out).all()
    assert (out[:, 3] <= c["t0"]).all() and (out[:, 3] >= 0).all()
