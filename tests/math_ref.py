"""Exact CPU references for the device math primitives (csrc/mrirt_device.h, csrc/brats_device.h) and the assertion
helpers tests/test_gpu_math_primitives.py applies to the device's results.  TEST INFRASTRUCTURE, CPU only.

  division      the IEEE quotient is NumPy's fp32 ``/`` (denormals on), cross-checked with ``fractions.Fraction``
  Markstein     q = RN(x r); e = fma(-q, d, x); fma(e, r, q) with an EXACT fp32 FMA (``fma32``: the fp64 product is exact, the sum
                is rounded to odd in fp64, then once to fp32), cross-checked with the same sequence in ``Fraction`` arithmetic
  exp, pow      correctly rounded to fp32: NumPy's fp64 value decides wherever every value within 2^-48 of it rounds to the
                same fp32 (libm's fp64 exp / pow are good to < 1 ulp = 2^-53; the host test checks that premise against
                mpmath on a sample), and mpmath at 160 bits decides the rest; ``*_mp`` are mpmath for every input
  lerp          unfused fp32 in the written order (STRICT), one exact FMA (FAST)
  clampf, satf  fminf(fmaxf(x, lo), hi): a quiet NaN x gives lo (HLSL saturate(NaN) = 0), a signalling one hi (IEEE 754-2008
                maxNum / minNum); -0 < +0; saturate gives 0 for every NaN
  half          ``astype(np.float16)`` (round to nearest even)
  rays          oracle_np.make_primary / make_ortho
  composite     one sample of oracle_np.brats_main's inner step, with oracle_np's own helpers
"""
from __future__ import annotations

from fractions import Fraction

import mpmath
import numpy as np

from oracle import oracle_np as onp

F = np.float32
U32 = np.uint32


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def from_bits(b) -> np.ndarray:
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def _quiet(fn):
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    wrapped.__name__ = fn.__name__
    wrapped.__doc__ = fn.__doc__
    return wrapped


# ---- exact rounding of a rational to fp32 ---------------------------------------------------------------------------
def round_fraction_to_f32(v: Fraction) -> np.float32:
    """RN-even of an exact rational to fp32: denormals, and overflow to inf at 2^128 - 2^103."""
    if v == 0:
        return F(0.0)
    sign, a = (-1.0, -v) if v < 0 else (1.0, v)
    e = _floor_log2(a)                           # 2^e <= a < 2^(e+1)
    q = max(e, -126) - 23                        # exponent of the last place
    scaled = a / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    if n * Fraction(2) ** q >= Fraction(2) ** 128:
        return F(sign * np.inf)
    return F(sign * float(n) * 2.0 ** q) if q >= -1000 else F(0.0)


def div_fraction(x, d) -> np.float32:
    """The IEEE quotient of two finite fp32 numbers, d != 0, through exact rational arithmetic (sign of zero included)."""
    x, d = F(x), F(d)
    if x == 0:
        return F(-0.0) if (np.signbit(x) != np.signbit(d)) else F(0.0)
    r = round_fraction_to_f32(Fraction(float(x)) / Fraction(float(d)))
    if r == 0:
        return F(-0.0) if (np.signbit(x) != np.signbit(d)) else F(0.0)
    return r


@_quiet
def ieee_div(x, d) -> np.ndarray:
    return np.asarray(x, dtype=np.float32) / np.asarray(d, dtype=np.float32)


@_quiet
def mul32(a, b) -> np.ndarray:
    return np.asarray(a, dtype=np.float32) * np.asarray(b, dtype=np.float32)


# ---- exact fp32 FMA ---------------------------------------------------------------------------------------------------
@_quiet
def fma32(a, b, c) -> np.ndarray:
    """RN(a * b + c) in fp32 with ONE rounding, for arrays.  a * b is exact in fp64 (48 bits); TwoSum gives the sum's rounding
    error exactly; the fp64 sum is then moved to the round-to-odd value, from which one rounding to fp32 (24 bits, or fewer for
    a denormal result: at least two bits narrower than fp64) equals the rounding of the exact sum."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float32) for v in (a, b, c)))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0.0)
    sb = np.ascontiguousarray(s).view(np.int64).copy()
    toward_zero = fix & ((err > 0.0) != (s > 0.0))          # the exact sum is smaller in magnitude than s: truncate first
    sb[toward_zero] -= 1
    sb[fix] |= 1
    return sb.view(np.float64).astype(np.float32)


def _floor_log2(a: Fraction) -> int:
    e = a.numerator.bit_length() - a.denominator.bit_length()
    return e - 1 if Fraction(2) ** e > a else e


def mul32_fraction(a, b) -> np.float32:
    a, b = F(a), F(b)
    v = Fraction(float(a)) * Fraction(float(b))
    if v == 0:
        return F(-0.0) if np.signbit(a) != np.signbit(b) else F(0.0)
    return round_fraction_to_f32(v)


def fma32_fraction(a, b, c) -> np.float32:
    """RN(a b + c) for finite fp32 a, b, c through exact rational arithmetic."""
    a, b, c = (F(v) for v in (a, b, c))
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:
        # an exact zero is -0 only as the sum of two negative zeros; a cancellation gives +0 in round-to-nearest
        both_zero = (a == 0 or b == 0) and c == 0
        return F(-0.0) if (both_zero and (np.signbit(a) != np.signbit(b)) and np.signbit(c)) else F(0.0)
    return round_fraction_to_f32(v)


# ---- Markstein division ---------------------------------------------------------------------------------------------
def markstein(x, d, r) -> np.ndarray:
    """M<true>::divu's three instructions, exactly."""
    q = mul32(x, r)
    e = fma32(-q, d, x)
    return fma32(e, r, q)


def markstein_fraction(x, d, r) -> np.float32:
    """The same sequence for one finite triple in Fraction arithmetic (each step rounded exactly).  Where q = RN(x r) overflows,
    e = -q d + x is an infinity of the sign opposite to q's (d r > 0) and e r + q is inf - inf = NaN, as on the hardware."""
    x, d, r = F(x), F(d), F(r)
    q = mul32_fraction(x, r)
    if not np.isfinite(q):
        return F(np.nan)
    e = fma32_fraction(-q, d, x)
    return fma32_fraction(e, r, q)


@_quiet
def divu_ref(x, d, r, exact, *, data: bool) -> np.ndarray:
    """What M<true>::divu (data=False) / divu_data (data=True) computes, bit for bit, for ANY input: the IEEE quotient where
    make_udiv said exact == 0, else the exact emulation of the sequence (divu_data: q itself when q is not finite)."""
    x, d, r = (np.asarray(v, dtype=np.float32) for v in (x, d, r))
    exact = np.asarray(exact) != 0
    m = markstein(x, d, r)
    if data:
        q = mul32(x, r)
        m = np.where(np.abs(q) < np.inf, m, q)
    return np.where(exact, m, ieee_div(x, d)).astype(np.float32)


# The contract domain of the exact path: make_udiv's exact == 1 (d and RN(1/d) normal, significand of d
# not all ones) and the numerator is a zero, or |x| >= 2^-100 with 2^-126 <= |x / d| <= 2^126.  One zero is outside: x = -0 over
# d > 0 gives +0 (q = -0, e = fma(+0, d, -0) = +0, fma(+0, r, -0) = +0) where the IEEE quotient is -0.  Why these bounds: the residual
# e = x - q d is a multiple of 2^(ex - 47) and must be representable (ex >= -102); q and the quotient must be normal for
# "q is within one ulp of x / d" to hold; and x r must not overflow.
X_MIN = F(2.0 ** -100)
Q_MIN = F(2.0 ** -126)
Q_MAX = F(2.0 ** 126)


@_quiet
def divu_domain(x, d, exact) -> np.ndarray:
    x, d = (np.asarray(v, dtype=np.float32) for v in (x, d))
    q = np.abs(x.astype(np.float64) / d.astype(np.float64))
    ok = (np.abs(x) >= X_MIN) & (q >= np.float64(Q_MIN)) & (q <= np.float64(Q_MAX)) & np.isfinite(x)
    zero = (x == 0) & ~(np.signbit(x) & (d > 0))
    return (np.asarray(exact) != 0) & (zero | ok)


def rn_recip(d) -> np.ndarray:
    """RN(1 / d) for every fp32 d (NumPy's IEEE division; inf for +-0, +-0 for inf, NaN for NaN)."""
    return ieee_div(F(1.0), d)


def udiv_exact_documented(d) -> np.ndarray:
    """``exact`` as mrirt_device.h documents it: d normal, RN(1/d) normal, significand of d not all ones."""
    d = np.asarray(d, dtype=np.float32)
    b = bits(d)
    r = rn_recip(d)

    def normal(v):
        e = (bits(v) >> 23) & 0xFF
        return (e != 0) & (e != 0xFF)
    return (normal(d) & normal(r) & ((b & 0x7FFFFF) != 0x7FFFFF)).astype(np.uint32)


# ---- correctly rounded exp / pow --------------------------------------------------------------------------------------
MP_PREC = 160


def _mpf_to_f32(v) -> np.float32:
    if mpmath.isnan(v):
        return F(np.nan)
    if mpmath.isinf(v):
        return F(np.inf) if v > 0 else F(-np.inf)
    sign, man, exp, bc = v._mpf_
    if man == 0:
        return F(0.0)
    if exp + bc > 200:                                   # far beyond fp32: no huge rationals
        return F(-np.inf) if sign else F(np.inf)
    if exp + bc < -200:
        return F(-0.0) if sign else F(0.0)
    fr = Fraction(int(man)) * (Fraction(2) ** int(exp))
    return round_fraction_to_f32(-fr if sign else fr)


def _mp_arg(x):
    x = float(x)
    if np.isnan(x):
        return mpmath.mpf("nan")
    if np.isinf(x):
        return mpmath.mpf("inf") if x > 0 else mpmath.mpf("-inf")
    return mpmath.mpf(x)


def exp_mp(x) -> np.ndarray:
    """Correctly rounded fp32 exp of every fp32 x, mpmath only."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    out = np.empty(x.size, dtype=np.float32)
    with mpmath.workprec(MP_PREC):
        for i, v in enumerate(x):
            out[i] = _mpf_to_f32(mpmath.exp(_mp_arg(v)))
    return out


def pow_mp(x, y) -> np.ndarray:
    """Correctly rounded fp32 pow(x, y) for x >= 0 (or NaN), mpmath only; pow(0, y > 0) = 0, pow(x, 0) = 1."""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float32).reshape(-1), np.asarray(y, dtype=np.float32).reshape(-1))
    out = np.empty(x.size, dtype=np.float32)
    with mpmath.workprec(MP_PREC):
        for i, (a, b) in enumerate(zip(x, y)):
            if np.isnan(a) or np.isnan(b):
                out[i] = np.nan
            elif a == 0:
                out[i] = 0.0 if b > 0 else (1.0 if b == 0 else np.inf)
            else:
                out[i] = _mpf_to_f32(mpmath.power(_mp_arg(a), _mp_arg(b)))
    return out


_FILTER = 2.0 ** -48


@_quiet
def _round_with_filter(y64, hard_fn):
    lo = (y64 * (1.0 - _FILTER)).astype(np.float32)
    hi = (y64 * (1.0 + _FILTER)).astype(np.float32)
    out = y64.astype(np.float32)
    hard = ~((bits(lo) == bits(hi)) | (np.isnan(lo) & np.isnan(hi)))
    idx = np.nonzero(hard)[0]
    if idx.size:
        out[idx] = hard_fn(idx)
    return out, idx


@_quiet
def exp_cr(x, *, return_hard=False):
    """Correctly rounded fp32 exp (NaN for NaN).  See the module docstring for the fp64 filter."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    out, idx = _round_with_filter(np.exp(x.astype(np.float64)), lambda i: exp_mp(x[i]))
    return (out, idx) if return_hard else out


@_quiet
def pow_cr(x, y, *, return_hard=False):
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float32).reshape(-1), np.asarray(y, dtype=np.float32).reshape(-1))
    out, idx = _round_with_filter(np.power(x.astype(np.float64), y.astype(np.float64)), lambda i: pow_mp(x[i], y[i]))
    return (out, idx) if return_hard else out


def midpoint_distance_ulp64(x) -> np.ndarray:
    """For each fp32 x: the distance from exp(x) (mpmath) to the nearest fp32 rounding boundary (the midpoint of two neighbouring
    fp32 values, denormals and the overflow threshold included), in units of the fp64 ulp of exp(x)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    out = np.empty(x.size, dtype=np.float64)
    with mpmath.workprec(MP_PREC):
        for i, v in enumerate(x):
            e = mpmath.exp(_mp_arg(min(max(float(v), -150.0), 150.0)))
            sign, man, ex, _ = e._mpf_
            val = Fraction(int(man)) * Fraction(2) ** int(ex)
            b2 = _floor_log2(val)
            ulp32 = Fraction(2) ** (max(b2, -126) - 23)
            k = val / ulp32
            n = k.numerator // k.denominator
            mid = (n + Fraction(1, 2)) * ulp32
            ulp64 = Fraction(2) ** (max(b2, -1022) - 52)
            out[i] = float(abs(val - mid) / ulp64)
    return out


# ---- exact emulation of the device's exp (IEEE fp64 fma / rint / ldexp assumed) -------------------------------------
def _fma64(a, b, c) -> float:
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def exp_device_emulation(x, consts, *, small=False, steps_short=0) -> np.ndarray:
    """exp_f64_to_f32 / exp_small_f64_to_f32 for finite fp32 x with the constants of fill_exp_consts (log2e, ln2hi, ln2lo, c[13]);
    ``steps_short`` drops that many of the LAST Horner steps (the wrong version of the sensitivity test)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    log2e, ln2hi, ln2lo = (float(v) for v in consts[:3])
    c = [float(v) for v in consts[3:16]]
    out = np.empty(x.size, dtype=np.float32)
    for i, xf in enumerate(x):
        v = float(xf)
        if small:
            k, r, start = 0.0, v, 3
        else:
            v = min(max(v, -200.0), 100.0)
            k = float(np.rint(v * log2e))
            r = _fma64(-k, ln2lo, _fma64(-k, ln2hi, v))
            start = 0
        coef = c[start + 1:] + [1.0]
        coef = coef[:len(coef) - steps_short]
        p = c[start]
        for cc in coef:
            p = _fma64(p, r, cc)
        with np.errstate(all="ignore"):
            out[i] = np.float32(np.ldexp(p, int(k)))
    return out


# ---- lerp -------------------------------------------------------------------------------------------------------------
@_quiet
def lerp_strict(a, b, t) -> np.ndarray:
    a, b, t = (np.asarray(v, dtype=np.float32) for v in (a, b, t))
    return a + t * (b - a)


@_quiet
def lerp_fast(a, b, t) -> np.ndarray:
    a, b, t = (np.asarray(v, dtype=np.float32) for v in (a, b, t))
    return fma32(t, b - a, a)


def trilerp(lerp, c, f) -> np.ndarray:
    """c: (n, 8, L) corners 000, 100, 010, 110, 001, 101, 011, 111; f: (n, 3) -> (n, L), sampleLinear's nesting order."""
    fx, fy, fz = (f[:, k:k + 1] for k in range(3))
    return lerp(lerp(lerp(c[:, 0], c[:, 1], fx), lerp(c[:, 2], c[:, 3], fx), fy),
                lerp(lerp(c[:, 4], c[:, 5], fx), lerp(c[:, 6], c[:, 7], fx), fy), fz)


# ---- clamp ------------------------------------------------------------------------------------------------------------
def _order_key(x) -> np.ndarray:
    b = bits(x).astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7FFFFFFF) - 1, b)       # monotone in the value, -0 below +0


def fmaxf(a, b) -> np.ndarray:
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32))
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(_order_key(a) >= _order_key(b), a, b))).astype(np.float32)


def fminf(a, b) -> np.ndarray:
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32))
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(_order_key(a) <= _order_key(b), a, b))).astype(np.float32)


def is_signalling_nan(x) -> np.ndarray:
    b = bits(x)
    return ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0) & ((b & 0x00400000) == 0)


def clamp_ref(x, lo, hi) -> np.ndarray:
    """fminf(fmaxf(x, lo), hi) with IEEE 754-2008's maxNum / minNum: a quiet NaN x is the missing operand (the result is lo: HLSL's
    rule); a signalling NaN makes maxNum return a quiet NaN, which minNum then drops (the result is hi)."""
    x, lo, hi = np.broadcast_arrays(*(np.asarray(v, dtype=np.float32) for v in (x, lo, hi)))
    return np.where(is_signalling_nan(x), hi, fminf(fmaxf(x, lo), hi)).astype(np.float32)


def sat_ref(x) -> np.ndarray:
    """HLSL saturate: 0 for every NaN (the clamp modifier), else clamp to [0, 1]."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isnan(x), F(0.0), fminf(fmaxf(x, F(0.0)), F(1.0))).astype(np.float32)


# ---- half -------------------------------------------------------------------------------------------------------------
@_quiet
def half_ref(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float32).astype(np.float16)


@_quiet
def half_truncating(x) -> np.ndarray:
    """The wrong version of the sensitivity test: round toward zero."""
    x = np.asarray(x, dtype=np.float32)
    h = x.astype(np.float16)
    over = np.isfinite(h) & (np.abs(h.astype(np.float32)) > np.abs(x))
    hb = h.view(np.uint16).copy()
    hb[over] -= 1
    out = hb.view(np.float16)
    big = np.isinf(h) & np.isfinite(x)
    return np.where(big, np.copysign(np.float16(65504.0), h), out).astype(np.float16)


# ---- rays -------------------------------------------------------------------------------------------------------------
def rays_ref(width, height, fovY, eye, U, V, W, *, ortho=None, k3=False):
    """ro, rd of shape (height, width, 3) from the oracle's own ray generation."""
    with np.errstate(all="ignore"):
        if ortho is None:
            (ox, oy, oz), d = onp.make_primary(width, height, fovY, eye, U, V, W, k3_aspect=k3)
            o = [np.full((height, width), v, np.float32) for v in (ox, oy, oz)]
        else:
            o, d = onp.make_ortho(width, height, ortho, eye, U, V, W)
    ro = np.stack([np.broadcast_to(v, (height, width)) for v in o], axis=-1).astype(np.float32)
    rd = np.stack([np.broadcast_to(v, (height, width)) for v in d], axis=-1).astype(np.float32)
    return ro, rd


def camera_ref(fovY, width, height, *, k3=False):
    """(invTanHalf, tanHalf, aspect) as the oracle computes them: (float)tan((double)(0.5f * fovY)); K1 / K2 divide the width by
    max(1, height), K3 by the height itself."""
    th = onp._tan(F(0.5) * F(fovY))
    dimx, dimy = F(width), F(height)
    with np.errstate(all="ignore"):
        aspect = dimx / dimy if k3 else dimx / max(F(1.0), dimy)
        return F(1.0) / th, th, F(aspect)


# ---- one sample's cell ------------------------------------------------------------------------------------------------------
@_quiet
def locate_ref(vol_min, voxel, dims, ro, rd, t):
    """oracle_np.brats_main's sample position and sampleLinear's cell, per element: p = o + t d; q = (p - volMin) / voxelSize;
    c = min(max(q, 0), float(dims) - 1.001f); cell = floor(c); f = c - floor(c).  All (n, 3) but t (n,)."""
    f = lambda a: np.asarray(a, dtype=np.float32)
    vol_min, voxel, ro, rd = f(vol_min), f(voxel), f(ro), f(rd)
    p = ro + f(t)[:, None] * rd
    q = (p - vol_min) / voxel
    c = np.minimum(np.maximum(q, F(0.0)), f(dims) - F(1.001))
    fl = np.floor(c)
    return q.astype(np.float32), fl.astype(np.uint32), (c - fl).astype(np.float32)


# ---- one compositing step -----------------------------------------------------------------------------------------------
@_quiet
def composite_step(p, v, g, rd, c0, t0, *, shade: bool):
    """One sample of oracle_np.brats_main's inner step (the lines between the blend of the modalities and the label overlays),
    per element.  p: dict of per-element fp32 arrays named as math_probe.K1_FIELDS.  Returns C (n,), T (n,), nLive, nShaded."""
    f = lambda a: np.asarray(a, dtype=np.float32)
    v, c0, t0 = f(v), f(c0), f(t0)
    ww, wl, gamma, wsum, ia, step = (f(p[k]) for k in ("ww", "wl", "gamma", "wsum", "intensityAlpha", "stepSize"))
    one = F(1.0)
    v = np.where(wsum > 0, v / wsum, v)
    val = onp._sat((v - (wl - ww * F(0.5))) / ww)
    val = np.power(val.astype(np.float64), gamma.astype(np.float64)).astype(np.float32)      # oracle_np._pow, per-element gamma
    pos = val > 0
    a = val * ia
    alpha = one - onp._exp(-a * step)
    if shade:
        g, rd = f(g), f(rd)
        gx, gy, gz = g[:, 0] * f(p["hx"]), g[:, 1] * f(p["hy"]), g[:, 2] * f(p["hz"])
        glen = np.sqrt(onp._dot3(gx, gy, gz, gx, gy, gz))
        ok = glen > f(p["gradEps"])
        safe = np.where(ok, glen, one)
        ndl = np.fmin(np.abs(onp._dot3(gx, gy, gz, rd[:, 0], rd[:, 1], rd[:, 2])) / safe, one)
        spec = ndl.copy()
        n2 = f(p["specPow2"]).astype(np.int64)
        for k in range(int(n2.max()) if n2.size else 0):
            spec = np.where(n2 > k, spec * spec, spec)
        shd = np.where(ok, (f(p["ka"]) + f(p["kd"]) * ndl) + f(p["ks"]) * spec, f(p["ka"]) + f(p["kd"]))
        emis = val * shd
    else:
        emis = val
    contrib = (alpha * t0) * emis
    C = np.where(pos, c0 + contrib, c0).astype(np.float32)
    T = np.where(pos, t0 * (one - alpha), t0).astype(np.float32)
    n_live = np.ones(v.size, dtype=np.uint32)
    n_shaded = (pos & shade).astype(np.uint32)
    return C, T, n_live, n_shaded


# =======================================================================================================================
# assertion helpers (the GPU tests apply them to the device's results; the host sensitivity test applies them to NumPy
# emulations of plausible wrong versions and requires them to fail)
# =======================================================================================================================
def _mismatch(got, ref) -> np.ndarray:
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gb, rb = np.ascontiguousarray(got).view(u), np.ascontiguousarray(ref).view(u)
    both_nan = np.isnan(got) & np.isnan(ref) if got.dtype.kind == "f" else np.zeros(got.shape, bool)
    return (gb != rb) & ~both_nan


def assert_bits_equal(got, ref, what: str, **inputs) -> None:
    """Bit equality (sign of zero included; any NaN equals any NaN), with the first mismatches and their inputs in the message."""
    bad = np.nonzero(_mismatch(got, ref).reshape(-1))[0]
    if bad.size:
        g, r = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
        lines = []
        for i in bad[:8]:
            ins = ", ".join(f"{k}={np.asarray(a).reshape(-1)[i % np.asarray(a).size]!r}" for k, a in inputs.items())
            lines.append(f"  [{i}] got {g[i]!r} ref {r[i]!r} ({ins})")
        raise AssertionError(f"{what}: {bad.size} of {g.size} differ\n" + "\n".join(lines))


def assert_divu(got, x, d, r, exact, *, data: bool, what: str):
    """Inside the contract domain: the IEEE quotient, bit for bit.  Everywhere: the exact emulation of the sequence (which pins the
    behaviour outside the domain and shows that the compiler kept the three instructions).  Returns the domain mask."""
    x, d, r = (np.asarray(v, dtype=np.float32).reshape(-1) for v in (x, d, r))
    dom = divu_domain(x, d, exact)
    if data:
        dom = dom | ((np.asarray(exact).reshape(-1) != 0) & ~np.isfinite(x))        # +-inf and NaN numerators: the IEEE result too
    q = ieee_div(x, d)
    g = np.asarray(got, dtype=np.float32).reshape(-1)
    assert_bits_equal(g[dom], q[dom], what + " vs IEEE quotient (contract domain)", x=x[dom], d=d[dom])
    inexact = np.asarray(exact).reshape(-1) == 0
    assert_bits_equal(g[inexact], q[inexact], what + " vs IEEE quotient (exact == 0)", x=x[inexact], d=d[inexact])
    assert_bits_equal(g, divu_ref(x, d, r, exact, data=data), what + " vs the exact emulation of the sequence", x=x, d=d)
    return dom


def assert_exp(got, x, what: str, ref=None):
    """Bit equality with the correctly rounded exp.  An input where the result differs is accepted only if mpmath shows exp(x)
    within one fp64 ulp of an fp32 rounding boundary (the device rounds a < 1-ulp fp64 value once); those inputs are returned
    and printed."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    ref = exp_cr(x) if ref is None else ref
    bad = np.nonzero(_mismatch(np.asarray(got, dtype=np.float32).reshape(-1), ref))[0]
    listed = []
    for i in bad:
        if not np.isfinite(x[i]):
            raise AssertionError(f"{what}: exp({x[i]!r}) = {got[i]!r}, correctly rounded {ref[i]!r}")
        dist = float(midpoint_distance_ulp64(x[i:i + 1])[0])
        g1 = np.asarray(got).reshape(-1)[i]
        near = abs(int(bits(g1)[()]) - int(bits(ref[i])[()])) == 1
        if not (dist <= 1.0 and near):
            raise AssertionError(f"{what}: exp({x[i]!r}) = {g1!r}, correctly rounded {ref[i]!r}; exp(x) is {dist:.3g} fp64 ulps from "
                                 f"the nearest fp32 rounding boundary ({bad.size} mismatches in all)")
        listed.append((float(x[i]), float(g1), float(ref[i]), dist))
    for item in listed:
        print(f"{what}: x={item[0]!r} device {item[1]!r} correctly rounded {item[2]!r}: exp(x) is {item[3]:.3g} fp64 ulp from a boundary")
    return listed


def assert_half(got, x, what: str) -> None:
    assert_bits_equal(np.asarray(got, dtype=np.float16), half_ref(x), what, x=x)


def assert_clamp(got, x, lo, hi, what: str) -> None:
    assert_bits_equal(np.asarray(got, dtype=np.float32), clamp_ref(x, lo, hi), what, x=x, lo=lo, hi=hi)


def assert_rays(ro, rd, ref_ro, ref_rd, what: str) -> None:
    assert_bits_equal(ro, ref_ro, what + ": ro")
    assert_bits_equal(rd, ref_rd, what + ": rd")


def assert_camera(cam, fovY, width, height, *, k3: bool, what: str) -> None:
    inv, th, aspect = camera_ref(fovY, width, height, k3=k3)
    assert_bits_equal(cam["tanHalf"], np.array([th], np.float32), what + ": tanHalf")
    assert_bits_equal(cam["invTanHalf"], np.array([inv], np.float32), what + ": invTanHalf")
    assert_bits_equal(cam["aspect"], np.array([aspect], np.float32), what + ": aspect")
