"""Inputs shared by tests/test_math_ref_host.py (reference self-checks, sensitivity) and tests/test_gpu_math_primitives.py.
Every list is seeded, at most 2^20 elements, and built once per session (functools.lru_cache): treat the arrays as read-only."""
from __future__ import annotations

import functools

import numpy as np

F = np.float32


def _from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def _rand_bits(rng, n):
    return _from_bits(rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))


def _rand_finite(rng, n):
    f = _rand_bits(rng, n + n // 64 + 64)
    return f[np.isfinite(f)][:n]


def _ulps_around(v, k):
    """Every fp32 within k ulps of v (v > 0 or v < 0), in bit order."""
    b = int(np.array([v], np.float32).view(np.uint32)[0])
    return _from_bits(np.arange(b - k, b + k + 1, dtype=np.int64).astype(np.uint32))


# ---- divisors -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def divisors() -> np.ndarray:
    """>= 2^16 divisors: random bits over every exponent, powers of two, all-ones and all-ones-minus-one significands at every
    exponent, denormals, +-0, inf, NaN, and divisors whose reciprocal is denormal (|d| > 2^126) or overflows (|d| < 2^-128)."""
    rng = np.random.default_rng(20250)
    e = np.arange(0, 256, dtype=np.uint32)                     # every exponent field, denormal (0) and inf / NaN (255) included
    per = 256
    mant = rng.integers(0, 2 ** 23, (256, per), dtype=np.uint32)
    sign = rng.integers(0, 2, (256, per), dtype=np.uint32) << 31
    rand = _from_bits((sign | (e[:, None] << 23) | mant).reshape(-1))
    special = []
    for s in (0, 0x80000000):
        special.append(_from_bits(s | (e << 23)))                               # powers of two (and +-0, +-inf)
        special.append(_from_bits(s | (e << 23) | 0x7FFFFF))                    # significand all ones (and the largest denormal, a NaN)
        special.append(_from_bits(s | (e << 23) | 0x7FFFFE))                    # all ones minus one
        special.append(_from_bits(s | (e << 23) | 0x000001))
    edge = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, 2.0 ** -127, 2.0 ** -128,
                     2.0 ** -128 * 1.5, 2.9387359e-39, 2.938736e-39, 2.0 ** 126, 2.0 ** 126 * 1.0000001, 2.0 ** 127, 3.4028235e38,
                     1.7014117e38, 1.7014118e38, 8.507059e37, 8.50706e37], dtype=np.float32)
    return np.concatenate([rand, *special, edge, -edge]).astype(np.float32)


@functools.lru_cache(None)
def divisors_in_use() -> np.ndarray:
    """The divisors the renderers pass: K2's 255; voxel sizes (1/240, 1/155, 0.9375-style NIfTI zooms); sums of volWeight in slot
    order; window widths from 1e-3 to 1e3."""
    rng = np.random.default_rng(20251)
    vox = [1.0 / 240.0, 1.0 / 155.0, 2.0 / 240.0, 0.9375, 1.0, 0.5, 1.2, 0.8, 0.4688, 3.0, 0.00390625]
    w = rng.uniform(0.0, 1.0, (256, 4)).astype(np.float32)
    sums = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    sums = np.concatenate([sums, w[:, 0] + w[:, 1], np.array([1.0, 2.0, 3.0, 4.0, F(0.3) + F(0.7), F(0.1) * 3, 0.99999994], np.float32)])
    ww = np.concatenate([np.logspace(-3, 3, 1024).astype(np.float32), np.array([0.5, 0.7, 0.8, 1.0, 1.1, 2.0, 0.99999994, 1e-3, 1e3], np.float32)])
    zs = rng.uniform(0.05, 400.0, 256).astype(np.float32)                                   # z-score sigmas of a dataset
    return np.concatenate([np.array([255.0], np.float32), np.array(vox, np.float32), sums.astype(np.float32), ww, zs])


@functools.lru_cache(None)
def divu_cases():
    """(x, d): every divisor of divisors() and divisors_in_use() against random-bit numerators, +-0, +-inf, NaN, numerators with
    subnormal quotients, |x| < 2^-100, and quotients at the overflow threshold; the bytes 0..255 over 255.  < 2^20 pairs."""
    rng = np.random.default_rng(20252)
    ds = np.concatenate([divisors(), divisors_in_use()])
    n = ds.size
    xs, dd = [], []

    def add(x, d):
        x, d = np.broadcast_arrays(np.asarray(x, np.float32), np.asarray(d, np.float32))
        xs.append(x.reshape(-1).copy()); dd.append(d.reshape(-1).copy())
    add(_rand_bits(rng, n * 3).reshape(n, 3), ds[:, None])                                # random bits (inf / NaN among them)
    for v in (0.0, -0.0, np.inf, -np.inf, np.nan, 3.4028235e38):
        add(np.full(n, v, np.float32), ds)
    with np.errstate(all="ignore"):
        d64 = ds.astype(np.float64)
        for lo, hi in ((-151, -124), (124, 129), (-30, 30)):                              # quotient exponents: subnormal, overflow, mid
            q = np.ldexp(1.0 + rng.integers(0, 2 ** 23, (n, 1)) / 2.0 ** 23, rng.integers(lo, hi + 1, (n, 1)))
            q = q * (1 - 2 * rng.integers(0, 2, (n, 1)))
            add((q * d64[:, None]).astype(np.float32), ds[:, None])
        tiny = np.ldexp(1.0 + rng.integers(0, 2 ** 23, (n, 1)) / 2.0 ** 23, rng.integers(-149, -98, (n, 1))).astype(np.float32)
        add(tiny * (1 - 2 * rng.integers(0, 2, (n, 1))).astype(np.float32), ds[:, None])   # |x| < 2^-98, denormals included
    add(np.arange(256, dtype=np.float32), F(255.0))
    add(np.arange(256, dtype=np.float32) * F(257.0), F(65535.0))
    x, d = np.concatenate(xs), np.concatenate(dd)
    assert x.size <= 2 ** 20
    return x, d


# ---- exp ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def exp_full_cases() -> np.ndarray:
    rng = np.random.default_rng(20253)
    spread = rng.uniform(-110.0, 90.0, 2 ** 18).astype(np.float32)
    denorm = rng.uniform(-104.0, -87.0, 2 ** 14).astype(np.float32)                         # the result is an fp32 denormal
    edge = np.array([-200.0, 100.0, -200.00002, 100.00001, -199.99998, 99.99999, -1e30, 1e30, -3.4028235e38, 3.4028235e38, 0.0, -0.0,
                     1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, np.inf, -np.inf, 88.72283, 88.72284, 88.722847, -87.33655, -103.27893,
                     -103.97208, -103.972084, -104.0, 1.0, -1.0, 0.6931472, -0.6931472, 0.34657359, -0.34657359], dtype=np.float32)
    return np.concatenate([spread, denorm, edge])


@functools.lru_cache(None)
def exp_small_cases() -> np.ndarray:
    """2^18 arguments in [-1/8, 1/8], every fp32 within 64 ulps of +-1/8 (both sides) and of 0 (the 64 smallest denormals of each
    sign and +-0)."""
    rng = np.random.default_rng(20254)
    u = rng.uniform(-0.125, 0.125, 2 ** 17).astype(np.float32)
    logu = (np.exp(rng.uniform(np.log(1e-12), np.log(0.125), 2 ** 17)) * rng.choice([-1.0, 1.0], 2 ** 17)).astype(np.float32)
    near0 = _from_bits(np.arange(0, 65, dtype=np.uint32))
    return np.concatenate([u, logu, _ulps_around(0.125, 64), _ulps_around(-0.125, 64), near0, -near0])


def exp_small_domain(x) -> np.ndarray:
    return np.abs(np.asarray(x, dtype=np.float32)) <= F(0.125)


# ---- pow ----------------------------------------------------------------------------------------------------------------
POW_EXPONENTS = (0.45, 0.6, 1.8, 2.2, 5.0)


@functools.lru_cache(None)
def pow_cases():
    rng = np.random.default_rng(20255)
    x1 = np.concatenate([rng.uniform(0.0, 1.0, 2 ** 12).astype(np.float32),
                         np.exp(rng.uniform(np.log(1e-45), 0.0, 2 ** 11)).astype(np.float32),
                         np.array([0.0, 1.0, 1e-45, 1.1754942e-38, 1.17549435e-38, 0.99999994, 0.5, 0.25], np.float32),
                         np.arange(256, dtype=np.float32) / F(255.0)])
    xs = [np.tile(x1, len(POW_EXPONENTS))]
    ys = [np.repeat(np.array(POW_EXPONENTS, np.float32), x1.size)]
    xs.append(rng.uniform(0.0, 1.0, 2 ** 15).astype(np.float32))
    ys.append(rng.uniform(0.1, 8.0, 2 ** 15).astype(np.float32))
    return np.concatenate(xs), np.concatenate(ys)


@functools.lru_cache(None)
def pow_identity_cases() -> np.ndarray:
    """y == 1: x must come back bit for bit, whatever it is."""
    rng = np.random.default_rng(20256)
    return np.concatenate([_rand_bits(rng, 2 ** 14), np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, -0.5, 1e-45, -1e-45], np.float32),
                           _from_bits(np.array([0x7FC00001, 0xFFC12345, 0x7F800001], np.uint32))])


# ---- clamp --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def clamp_cases():
    """(x, lo, hi) with lo <= hi and lo = +0 wherever a bound is a zero (the kernels clamp to [0, hi] only).  NaN, +-0, +-inf,
    denormals, values equal to the bounds, lo == hi."""
    rng = np.random.default_rng(20257)
    sp = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.0, -1.0, 0.99999994,
                   1.0000001, 0.5, 238.999, 239.0, 154.0, 153.999, 3.4028235e38, -3.4028235e38], np.float32)
    bounds = [(0.0, 1.0), (0.0, 238.999), (0.0, 154.0), (0.0, 0.0), (1.0, 1.0), (0.5, 0.5), (1e-45, 1e-45), (0.0, np.inf), (-1.0, 1.0),
              (-np.inf, np.inf), (0.25, 0.75), (-3.0, -2.0), (0.0, 1e-45)]
    xs, los, his = [], [], []
    rnd = np.concatenate([_rand_bits(rng, 2048), rng.uniform(-2.0, 300.0, 2048).astype(np.float32)])
    for lo, hi in bounds:
        x = np.concatenate([sp, np.array([lo, hi], np.float32), rnd])
        xs.append(x); los.append(np.full(x.size, lo, np.float32)); his.append(np.full(x.size, hi, np.float32))
    return np.concatenate(xs), np.concatenate(los), np.concatenate(his)


@functools.lru_cache(None)
def sat_cases() -> np.ndarray:
    x, lo, hi = clamp_cases()
    return x[(lo == 0.0) & (hi == 1.0)]


# ---- lerp ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def lerp_cases():
    """(a, b, t): intensities and gradients as the march blends them (t = a fraction in [0, 1)), plus signed wide-range values."""
    rng = np.random.default_rng(20258)
    n = 2 ** 16
    a = np.concatenate([rng.uniform(0.0, 1.0, n), rng.normal(0.0, 50.0, n)]).astype(np.float32)
    b = np.concatenate([rng.uniform(0.0, 1.0, n), rng.normal(0.0, 50.0, n)]).astype(np.float32)
    t = np.concatenate([rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)]).astype(np.float32)
    sp = np.array([0.0, -0.0, 1.0, 0.99999994, 1e-45, 0.5], np.float32)
    A, B, T = (g.reshape(-1) for g in np.meshgrid(sp, sp, sp, indexing="ij"))
    return np.concatenate([a, A]), np.concatenate([b, B]), np.concatenate([t, T])


@functools.lru_cache(None)
def trilerp_cases():
    """c: (n, 8, 2), f: (n, 3)."""
    rng = np.random.default_rng(20259)
    n = 2 ** 15
    c = rng.uniform(0.0, 1.0, (n, 8, 2)).astype(np.float32)
    c[n // 2:] = rng.normal(0.0, 30.0, (n - n // 2, 8, 2)).astype(np.float32)
    f = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    f[:8] = np.array([[x, y, z] for x in (0.0, 0.99999994) for y in (0.0, 0.99999994) for z in (0.0, 0.99999994)], np.float32)
    return c, f


# ---- cameras ------------------------------------------------------------------------------------------------------------
IMAGE_SIZES = ((1, 1), (17, 33), (1024, 3))          # (width, height)


@functools.lru_cache(None)
def camera_cases():
    """dicts: eye, U, V, W, fovY, ortho (None or the half height), k3 (the K3 aspect ratio).  Random orthonormal-ish bases and two
    axis-aligned ones (zero direction components)."""
    rng = np.random.default_rng(20260)
    out = []
    for i in range(6):
        m = np.linalg.qr(rng.normal(size=(3, 3)))[0].astype(np.float32)
        out.append(dict(eye=rng.uniform(-3, 3, 3).astype(np.float32), U=m[0], V=m[1], W=m[2],
                        fovY=F(rng.uniform(0.2, 2.4)), ortho=None if i % 3 else F(rng.uniform(0.3, 2.0)), k3=(i % 2 == 1)))
    I = np.eye(3, dtype=np.float32)
    out.append(dict(eye=np.array([0.0, 0.0, 2.5], np.float32), U=I[0], V=I[1], W=-I[2], fovY=F(0.8726646), ortho=None, k3=False))
    out.append(dict(eye=np.array([1.5, 0.0, 0.0], np.float32), U=I[2], V=I[1], W=-I[0], fovY=F(1.0471976), ortho=F(1.1), k3=False))
    out.append(dict(eye=np.array([0.0, -2.0, 0.0], np.float32), U=I[0], V=I[2], W=I[1], fovY=F(0.5), ortho=None, k3=True))
    return out


FOV_CASES = tuple(F(v) for v in (0.2, 0.5, 0.8726646, 1.0471976, 1.5707964, 2.4, 3.0, 3.1415925, 1e-3))
# fill_camera's aspect ratio, host only: (width, height, k3).  A height of 0 is the one place where K1 / K2 (width / max(1,
# height)) and K3 (width / height) differ; no frame can have it, the field is still computed.
ASPECT_CASES = ((1, 1, False), (17, 33, False), (1024, 3, False), (17, 33, True), (1024, 3, True), (640, 0, False), (640, 0, True))


# ---- half ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def half_cases() -> np.ndarray:
    """fp32 inputs: every finite half; every midpoint of two neighbouring halves and one fp32 ulp either side of it; 65504 ..
    65520 and beyond; half denormals and below; +-0, +-inf, NaN."""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)           # every finite half >= 0
    nxt = np.concatenate([h[1:], np.array([65536.0], np.float32)])                           # the value after 65504 would be 65536
    mid = ((h.astype(np.float64) + nxt.astype(np.float64)) * 0.5).astype(np.float32)         # exact in fp32 (12 bits)
    below, above = np.nextafter(mid, F(0.0)), np.nextafter(mid, F(np.inf))
    extra = np.array([65504.0, 65505.0, 65519.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e5, 3.4028235e38, np.inf, np.nan, 2.0 ** -24,
                      2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.0 ** -26, 1e-45, 0.0], np.float32)
    pos = np.concatenate([h, mid, below, above, extra])
    x = np.concatenate([pos, -pos])
    return np.concatenate([x, np.zeros((-x.size) % 4, np.float32)])                           # whole RGBA texels: padded, nothing cut


# ---- wave counters -------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def wave_count_cases():
    rng = np.random.default_rng(20261)
    big = rng.integers(0, 2 ** 24 + 1, 1000 * 64 + 37, dtype=np.uint64).astype(np.uint32)    # ~1000 waves, a partial last workgroup
    big[64 * 10:64 * 14] = 0                                                                # all-zero waves
    big[-37:] = 2 ** 24
    return dict(random=big, zeros=np.zeros(256 * 3 + 5, np.uint32), one_lane=np.array([2 ** 24], np.uint32),
                full=np.full(64 * 256, 2 ** 24, np.uint32))


# ---- composite ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def composite_cases(gamma1: bool):
    """P launch-constant blocks (math_probe.K1_FIELDS order) and 2^16 samples that pick one each: ww / wl with both saturation ends
    and tfLo == 0; gamma (1 for the GAMMA1 kernels); volWeight sums, exactly 1 included; alpha dt on both sides of 1/8; gradient
    lengths on both sides of gradEps; specPow2 0..6; T in [0.01, 1]."""
    rng = np.random.default_rng(20262 + int(gamma1))
    P, n = 512, 2 ** 16
    ww = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), P)).astype(np.float32)
    ww[:8] = np.array([0.5, 0.7, 0.8, 1.0, 1.1, 2.0, 0.99999994, 1.9999999], np.float32)
    wl = (rng.uniform(-0.2, 1.2, P) * np.maximum(ww, 1.0)).astype(np.float32)
    wl[::4] = ww[::4] * F(0.5)                                                             # tfLo == 0 exactly
    gamma = np.ones(P, np.float32) if gamma1 else rng.choice(np.array([0.45, 0.6, 1.0, 1.8, 2.2, 5.0], np.float32), P)
    if not gamma1:
        gamma[1::7] = rng.uniform(0.1, 8.0, gamma[1::7].size).astype(np.float32)
    w = rng.uniform(0.0, 1.0, (P, 4)).astype(np.float32)
    wsum = (((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]).astype(np.float32)
    wsum[::3] = 1.0
    wsum[1::9] = 0.0                                                                       # no modality enabled: no division
    step = np.exp(rng.uniform(np.log(1e-3), np.log(0.05), P)).astype(np.float32)
    adt = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), P))                                # alpha * dt, both sides of 1/8
    adt[:6] = [0.125, 0.1249999, 0.1250001, 0.12, 0.13, 1.0]
    ia = (adt / step).astype(np.float32)
    ka, kd, ks = (rng.uniform(0.0, 1.0, P).astype(np.float32) for _ in range(3))
    eps = rng.choice(np.array([1e-6, 1e-3, 0.0, 0.5], np.float32), P)
    spec = rng.integers(0, 7, P).astype(np.float32)
    h = (0.5 / rng.uniform(0.004, 1.2, (P, 3))).astype(np.float32)
    params = np.stack([ww, wl, gamma, wsum, ia, step, ka, kd, ks, eps, spec, h[:, 0], h[:, 1], h[:, 2]], axis=1).astype(np.float32)
    sel = rng.integers(0, P, n)
    sel[:P] = np.arange(P)
    # v so that (v / wsum - tfLo) / ww covers [-0.25, 1.25]: both saturation ends and the ramp
    u = rng.uniform(-0.25, 1.25, n)
    u[::16] = rng.choice([0.0, 1.0], u[::16].size)
    tflo = (wl - ww * F(0.5)).astype(np.float64)
    s = np.where(wsum[sel] > 0, wsum[sel], 1.0).astype(np.float64)
    v = ((u * ww[sel] + tflo[sel]) * s).astype(np.float32)
    g = (rng.normal(0.0, 1.0, (n, 3)) * np.exp(rng.uniform(np.log(1e-9), np.log(10.0), (n, 1)))).astype(np.float32)
    g[::32] = 0.0
    rd = rng.normal(size=(n, 3))
    rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(np.float32)
    c0 = rng.uniform(0.0, 1.0, n).astype(np.float32)
    t0 = rng.uniform(0.01, 1.0, n).astype(np.float32)
    return dict(params=params, sel=sel, v=v, g=g, rd=rd, c0=c0, t0=t0)


# ---- locate ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def locate_cases():
    """P volumes (volMin, voxelSize, dims: the voxel sizes in use and random ones, dims 2 .. 512) and 2^16 samples each picking
    one: positions spread from two voxels outside the box to two voxels beyond it (both clamps), exactly on lattice planes
    (fraction 0), just below them, and at the upper clamp dims - 1.001."""
    rng = np.random.default_rng(20263)
    P, n = 256, 2 ** 16
    vox = np.exp(rng.uniform(np.log(0.004), np.log(1.2), (P, 3))).astype(np.float32)
    vox[:4] = np.array([[1 / 240, 1 / 240, 1 / 155], [0.9375, 0.9375, 1.2], [1.0, 1.0, 1.0], [0.00390625, 0.5, 0.4688]], np.float32)
    dims = rng.integers(2, 513, (P, 3)).astype(np.float32)
    dims[:4] = np.array([[240, 240, 155], [2, 2, 2], [512, 512, 512], [3, 17, 33]], np.float32)
    vmin = (-(vox * dims) * rng.uniform(0.0, 1.0, (P, 3))).astype(np.float32)
    vmin[2] = 0.0
    params = np.concatenate([vmin, vox, dims], axis=1).astype(np.float32)
    sel = rng.integers(0, P, n)
    sel[:P] = np.arange(P)
    u = rng.uniform(-2.0, 2.0, (n, 3)) + rng.uniform(0.0, 1.0, (n, 3)) * dims[sel]                 # target index-space position
    u[::8] = np.round(u[::8])                                                                      # lattice planes
    u[1::8] = np.nextafter(np.round(u[1::8]).astype(np.float32), np.float32(-1e9))
    u[2::64] = dims[sel[2::64]] - 1.001
    target = (vmin[sel] + u * vox[sel]).astype(np.float64)
    rd = rng.normal(size=(n, 3))
    rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(np.float32)
    t = rng.uniform(0.0, 4.0, n).astype(np.float32)
    ro = (target - t[:, None].astype(np.float64) * rd).astype(np.float32)
    return dict(params=params, sel=sel, ro=ro, rd=rd, t=t)
