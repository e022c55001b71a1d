"""NumPy restatements of the case preparation: what csrc/prep.hip must give bit for bit.  Each one is pinned to
its source (np.percentile, volume.normalize_intensity, scipy.ndimage.gaussian_filter, an fp64 evaluation) by
tests/test_prep_host.py; the GPU tests compare the kernels with these."""
import numpy as np

f32 = np.float32
NAN_KEY = 0xFFFFFFFF
MAX_RADIUS = 16


# --- keys ------------------------------------------------------------------------------------------------------------------
def key(bits: int) -> int:
    """Order-preserving uint32 key of fp32 bits: -0.0 and +0.0 one key, every NaN the largest."""
    bits &= 0xFFFFFFFF
    if (bits & 0x7FFFFFFF) > 0x7F800000:
        return NAN_KEY
    if bits == 0x80000000:
        bits = 0
    return (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits | 0x80000000


def key_inverse(k: int) -> int:
    if k == NAN_KEY:
        return 0x7FC00000
    return k & 0x7FFFFFFF if k & 0x80000000 else ~k & 0xFFFFFFFF


def keys(vol: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(vol, dtype=np.float32).reshape(-1).view(np.uint32).copy()
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    b[b == 0x80000000] = 0
    k = np.where(b & 0x80000000 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = NAN_KEY
    return k


def select_bin(hist, rank):
    """(bin, remaining rank) of the element of 0-based rank `rank` in a histogram."""
    before = 0
    for b, c in enumerate(hist):
        if rank - before < c or b == len(hist) - 1:
            return b, rank - before
        before += c


# --- percentile ------------------------------------------------------------------------------------------------------------
def rank(n: int, q: float):
    """(k, g): np.percentile's fp32 index for n fp32 values."""
    qq = f32(q) / f32(100)
    v = f32(n - 1) * qq
    k = int(np.floor(v))
    g = f32(v - f32(k))
    if k > n - 1:
        k, g = n - 1, f32(0)
    return k, g


def lerp(a, b, g):
    a, b, g = f32(a), f32(b), f32(g)
    with np.errstate(all="ignore"):
        d = f32(b - a)
        if g < f32(0.5):
            return f32(a + f32(d * g))
        return f32(b - f32(d * f32(f32(1) - g)))


def order_stats(vol: np.ndarray, q: float):
    s = np.sort(np.asarray(vol, dtype=np.float32).ravel())
    k, g = rank(s.size, q)
    return s[k], s[min(k + 1, s.size - 1)], g


def percentile(vol: np.ndarray, q: float) -> np.float32:
    v = np.asarray(vol, dtype=np.float32).ravel()
    if np.isnan(v).any():
        return f32(np.nan)
    a, b, g = order_stats(v, q)
    return lerp(a, b, g)


def window(vol: np.ndarray, percentiles=(1.0, 99.5)) -> np.ndarray:
    """The device record { lo, hi, span, min, max, p_lo, p_hi, 0 }."""
    v = np.asarray(vol, dtype=np.float32).ravel()
    p_lo, p_hi = percentile(v, percentiles[0]), percentile(v, percentiles[1])
    with np.errstate(all="ignore"):
        mn, mx = v.min(), v.max()
        lo, hi = p_lo, p_hi
        if hi <= lo:
            lo, hi = mn, mx
        d = float(hi) - float(lo)
    span = f32(d if d > 1e-6 else 1e-6)
    return np.array([lo, hi, span, mn, mx, p_lo, p_hi, 0], dtype=np.float32)


def normalize(vol: np.ndarray, rec: np.ndarray) -> np.ndarray:
    v = np.asarray(vol, dtype=np.float32)
    with np.errstate(all="ignore"):
        q = ((v - f32(rec[0])) / f32(rec[2])).astype(np.float32)
        q = np.where(q < 0, f32(0), q)
        q = np.where(q > 1, f32(1), q)
    return q.astype(np.float32)


def flatten_xyz(v: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.transpose(v, (2, 1, 0)).reshape(-1))


def window_scratch_bytes(n: int) -> int:
    def al(x):
        return (x + 255) // 256 * 256
    if n < 1 or n > 2**31 - 1:
        return 0
    blocks = min(max(-(-n // 4096), 1), 512)
    return 256 + al(8 * blocks) + 4096 + 4096 * blocks


# --- z-score ---------------------------------------------------------------------------------------------------------------
def zscore_stats(vol: np.ndarray):
    """(mu32, sigma32, count) from fp64 sums over the non-zero voxels."""
    v = np.asarray(vol, dtype=np.float32).ravel()
    x = v[v != 0].astype(np.float64)
    if x.size == 0:
        return f32(0), f32(0), 0
    mu = x.sum() / x.size
    var = ((x - mu) ** 2).sum() / x.size
    return f32(mu), f32(np.sqrt(var)), int(x.size)


def zscore_apply(vol: np.ndarray, mu32, sigma32, count) -> np.ndarray:
    v = np.asarray(vol, dtype=np.float32)
    if count == 0:
        return v.copy()
    with np.errstate(all="ignore"):
        return ((v - f32(mu32)) / f32(f32(sigma32) + f32(1e-6))).astype(np.float32)


def zscore_f64(vol: np.ndarray) -> np.ndarray:
    """The z-scored volume evaluated in fp64 throughout (the yardstick of the host's own fp32 error)."""
    v = np.asarray(vol, dtype=np.float64)
    x = v[v != 0]
    if x.size == 0:
        return v
    return (v - x.mean()) / (x.std() + 1e-6)


# --- Gaussian --------------------------------------------------------------------------------------------------------------
def gaussian_weights(sigma: float) -> np.ndarray:
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, int(4 sigma + 0.5)) in NumPy fp64."""
    sigma = float(sigma)
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


def reflect(i: int, n: int) -> int:
    m = i % (2 * n)
    return m if m < n else 2 * n - 1 - m


def gaussian_pass(a: np.ndarray, w: np.ndarray, axis: int) -> np.ndarray:
    r = (len(w) - 1) // 2
    n = a.shape[axis]
    x = np.moveaxis(a, axis, 0).astype(np.float64)
    idx = np.arange(n)

    def at(j):
        return x[[reflect(int(i) + j, n) for i in idx]]
    t = x * w[r]
    for j in range(-r, 0):
        t = t + (at(j) + at(-j)) * w[j + r]
    return np.moveaxis(t.astype(np.float32), 0, axis)


def gaussian_filter(a: np.ndarray, sigma: float = None, weights: np.ndarray = None) -> np.ndarray:
    w = gaussian_weights(sigma) if weights is None else np.asarray(weights, dtype=np.float64)
    out = np.ascontiguousarray(a, dtype=np.float32)
    for axis in range(out.ndim):
        out = gaussian_pass(out, w, axis)
    return np.ascontiguousarray(out)


def same(a, b) -> bool:
    """array_equal with NaN matching NaN and -0.0 == +0.0."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))
