"""References for the coordinate-injection INR (csrc/inr_inject.hip): the definition of include/mrirt.h
restated in NumPy.  No GPU.

  net_shape        input widths and the [h | coords | mods] splits of every layer
  features32 / 64  the Fourier projection: fp32 operation by operation with the restated STRICT sine / cosine
                   (inr_siren_ref.sincos32), and in fp64 with np.sin / np.cos
  matmul32         x W as the MFMA sums it: products added in increasing k from +0, one rounding per step
  forward32 / 64   the network, with the restated dropout masks when asked
  keep_mask        the library's mask rule on the restated Philox of inr_loop_ref
  uncertainty32/64 softmax per sample, mean in sample order, entropy
  forward_int      the integer tier: 8 x the logits of a net whose every value is a multiple of 1/8, in int64
  boundary_weights the boundary map by brute force (exact integer squared distances)
  selection_net    one non-zero power of two per weight column
"""
import numpy as np

import inr_loop_ref as lref
import inr_siren_ref as sref

TWO_PI32 = np.float32(6.2831855)


def net_shape(F, M, widths, coord_layers=(), mod_layers=()):
    """[(in, split, splitM, out)] per layer: columns k < split are h, split <= k < splitM coords, the rest mods."""
    L = len(widths)
    out = []
    for l, w in enumerate(widths):
        prev = F if l == 0 else widths[l - 1]
        cj = 0 < l < L - 1 and l in coord_layers
        mj = l == 0 or (0 < l < L - 1 and l in mod_layers)
        split_m = prev + (3 if cj else 0)
        out.append((split_m + (M if mj else 0), prev, split_m, w))
    return out


def bits(coord_layers, mod_layers, L):
    """The two bit sets of MrirtInjectDesc; indices the layer loop never reaches (0 and >= L - 1) are dropped, as the loader drops them."""
    c = sum(1 << l for l in set(coord_layers) if 0 < l < L - 1)
    m = sum(1 << l for l in set(mod_layers) if 0 < l < L - 1)
    return c, m


def features32(B, coords):
    B, c = np.asarray(B, np.float32), np.asarray(coords, np.float32)
    with np.errstate(all="ignore"):
        u = (c + np.float32(1.0)) * np.float32(0.5)
        p = ((u[:, 0:1] * B[None, :, 0]) + (u[:, 1:2] * B[None, :, 1])) + (u[:, 2:3] * B[None, :, 2])
        a = TWO_PI32 * p
    s, k = sref.sincos32(a)
    return np.concatenate([s, k], 1).astype(np.float32)


def features64(B, coords):
    B, c = np.asarray(B, np.float64), np.asarray(coords, np.float64)
    a = 2.0 * np.pi * (((c + 1.0) / 2.0) @ B.T)
    return np.concatenate([np.sin(a), np.cos(a)], 1)


def matmul32(x, W):
    """acc <- float32(acc + x[:, k] W[k]) for k ascending from +0: the product is exact in fp64, so with one non-zero term per
    sum this is the single fp32 product bit for bit (and 0 * inf, 0 * NaN poison a row as they do on the device)."""
    x, W = np.asarray(x, np.float32), np.asarray(W, np.float32)
    acc = np.zeros((x.shape[0], W.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for k in range(W.shape[0]):
            acc = (acc.astype(np.float64) + x[:, k:k + 1].astype(np.float64) * W[k][None, :].astype(np.float64)).astype(np.float32)
    return acc


def threshold(keep):
    return int(np.floor(float(np.float32(keep)) * 4294967296.0))


def keep_mask(seed, i, s, l, width, keep):
    """bool [len(i)][width]: element (i, l, j) of sample s is kept iff its Philox word < floor(keep 2^32); keep == 1 keeps all."""
    i = np.asarray(i, np.uint64)
    if np.float32(keep) == np.float32(1.0):
        return np.ones((i.size, width), bool)
    seed = int(seed) & (2 ** 64 - 1)
    groups = (width + 3) // 4
    ii = np.repeat(i, groups)
    g = np.tile(np.arange(groups, dtype=np.uint64), i.size)
    r = lref.philox4x32_10((ii & np.uint64(lref.MASK), ii >> np.uint64(32), 256 * int(s) + int(l), g), (seed & lref.MASK, seed >> 32))
    words = np.stack(r, 1).reshape(i.size, groups * 4)[:, :width]
    return words.astype(np.uint64) < np.uint64(threshold(keep))


def _layer_input(h, coords, mods, shape):
    n_in, split, split_m, _ = shape
    parts = [h]
    if split_m > split:
        parts.append(coords)
    if n_in > split_m:
        parts.append(mods)
    return np.concatenate(parts, 1) if len(parts) > 1 else h


def _forward(params, coords, mods, coord_layers, mod_layers, dropout, index0, dtype):
    """dropout: None or dict(seed, keep, s)."""
    f32 = dtype == np.float32
    Ws = [np.asarray(p["W"], dtype) for p in params["mlp"]]
    bs = [np.asarray(p["b"], dtype) for p in params["mlp"]]
    coords = np.asarray(coords, np.float32)
    n = coords.shape[0]
    mods = np.asarray(mods, np.float32).reshape(n, -1)
    F, M = 2 * np.asarray(params["fourier"]["B"]).shape[0], mods.shape[1]
    shapes = net_shape(F, M, [w.shape[1] for w in Ws], coord_layers, mod_layers)
    h = features32(params["fourier"]["B"], coords) if f32 else features64(params["fourier"]["B"], coords)
    c, m = coords.astype(dtype), mods.astype(dtype)
    i = np.arange(n, dtype=np.uint64) + np.uint64(index0)
    with np.errstate(all="ignore"):
        for l, (W, b, shape) in enumerate(zip(Ws, bs, shapes)):
            assert W.shape == (shape[0], shape[3]), (l, W.shape, shape)
            x = _layer_input(h, c, m, shape)
            z = (matmul32(x, W) if f32 else x @ W) + b[None, :]
            if l == len(Ws) - 1:
                return z
            h = np.where(z <= 0, dtype(0), z)                      # jnp.maximum(z, 0): -0 -> +0, a NaN stays
            if dropout is not None and np.float32(dropout["keep"]) != np.float32(1.0):
                kept = keep_mask(dropout["seed"], i, dropout["s"], l, shape[3], dropout["keep"])
                scale = np.float32(1.0) / np.float32(dropout["keep"])
                h = np.where(kept, h * dtype(scale), dtype(0))


def forward32(params, coords, mods, coord_layers=(1, 2, 3), mod_layers=(2,), dropout=None, index0=0):
    return _forward(params, coords, mods, coord_layers, mod_layers, dropout, index0, np.float32)


def forward64(params, coords, mods, coord_layers=(1, 2, 3), mod_layers=(2,), dropout=None, index0=0):
    return _forward(params, coords, mods, coord_layers, mod_layers, dropout, index0, np.float64)


def argmax(z):
    """np.argmax: the first index of the maximum, a NaN counting as the maximum."""
    return np.argmax(z, axis=1).astype(np.int16)


def softmax32(z):
    """point_softmax of csrc/inr_device.h: d = z - max, p = exp d, s = the sum in class order, p *= 1 / s."""
    z = np.asarray(z, np.float32)
    with np.errstate(all="ignore"):
        d = z - np.max(z, axis=1, keepdims=True)                   # fmaxf drops a NaN; the tolerance tier holds none
        p = np.exp(d).astype(np.float32)
        s = np.zeros(z.shape[0], np.float32)
        for k in range(z.shape[1]):
            s = s + p[:, k]
        return p * (np.float32(1.0) / s)[:, None]


def entropy32(sum_p, S):
    mean = sum_p / np.float32(S)
    h = np.zeros(mean.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for k in range(mean.shape[1]):
            h = h + mean[:, k] * np.log(mean[:, k] + np.float32(1e-10)).astype(np.float32)
    return -h, mean


def uncertainty32(params, coords, mods, coord_layers, mod_layers, seed, keep, S, sample0=0, index0=0):
    acc = None
    for s in range(S):
        p = softmax32(forward32(params, coords, mods, coord_layers, mod_layers, dict(seed=seed, keep=keep, s=sample0 + s), index0))
        acc = p if acc is None else acc + p
    return entropy32(acc, S)


def uncertainty64(params, coords, mods, coord_layers, mod_layers, seed, keep, S, sample0=0, index0=0):
    acc = 0.0
    for s in range(S):
        z = forward64(params, coords, mods, coord_layers, mod_layers, dict(seed=seed, keep=keep, s=sample0 + s), index0)
        e = np.exp(z - z.max(1, keepdims=True))
        acc = acc + e / e.sum(1, keepdims=True)
    mean = acc / S
    return -(mean * np.log(mean + 1e-10)).sum(1), mean


def grid_coords(hwd):
    """sample_coord over the C-order voxels of [H][W][D]: ((float)i / (float)(E - 1)) * 2 - 1, each operation rounded to fp32."""
    ax = [(np.arange(e, dtype=np.float32) / np.float32(e - 1)) * np.float32(2.0) - np.float32(1.0) for e in hwd]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float32)


def volume_mods(mods):
    """[M][H][W][D] -> [H W D][M], the notebook's transpose."""
    mods = np.asarray(mods, np.float32)
    return np.ascontiguousarray(mods.reshape(mods.shape[0], -1).T)


# ---- integer tier ------------------------------------------------------------------------------------------------------------
def forward_int(params, coords8, mods, coord_layers, mod_layers):
    """8 x logits in int64 for B = 0 (sin +0, cos 1), coords = coords8 / 8, integer mods, weights and biases; and the largest
    |partial sum| bound of any layer (in units of 1/8): the fp32 sums are exact while it stays below 2^24."""
    Ws = [np.asarray(p["W"]).astype(np.int64) for p in params["mlp"]]
    bs = [np.asarray(p["b"]).astype(np.int64) for p in params["mlp"]]
    half = np.asarray(params["fourier"]["B"]).shape[0]
    n = coords8.shape[0]
    m8 = np.asarray(mods).astype(np.int64).reshape(n, -1) * 8
    c8 = np.asarray(coords8).astype(np.int64)
    h = np.concatenate([np.zeros((n, half), np.int64), np.full((n, half), 8, np.int64)], 1)
    shapes = net_shape(2 * half, m8.shape[1], [w.shape[1] for w in Ws], coord_layers, mod_layers)
    bound = 0
    for l, (W, b, shape) in enumerate(zip(Ws, bs, shapes)):
        x = _layer_input(h, c8, m8, shape)
        bound = max(bound, int((np.abs(x) @ np.abs(W) + 8 * np.abs(b)[None, :]).max()))
        z = x @ W + 8 * b[None, :]
        if l == len(Ws) - 1:
            return z, bound
        h = np.maximum(z, 0)


# ---- boundary weights ----------------------------------------------------------------------------------------------------------
def boundary_weights(seg, num_classes=4):
    """float32(max_c 1 / (1 + sqrt(d2_c))) with d2_c the exact integer squared distance to class c, by brute force; 0 without one."""
    seg = np.asarray(seg)
    pts = np.stack(np.meshgrid(*[np.arange(e) for e in seg.shape], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    out = np.zeros(pts.shape[0], np.float64)
    flat = seg.reshape(-1)
    for c in range(1, num_classes):
        q = pts[flat == c]
        if q.shape[0] == 0:
            continue
        d2 = np.full(pts.shape[0], np.iinfo(np.int64).max, np.int64)
        for i in range(0, q.shape[0], 256):
            d2 = np.minimum(d2, ((pts[:, None, :] - q[None, i:i + 256, :]) ** 2).sum(-1).min(1))
        out = np.maximum(out, 1.0 / (1.0 + np.sqrt(d2.astype(np.float64))))
    return out.astype(np.float32).reshape(seg.shape)


# ---- nets ----------------------------------------------------------------------------------------------------------------------
def selection_net(rng, F, M, widths, coord_layers, mod_layers, shift=0, bias=True):
    """One non-zero power of two (2^-2 .. 2^2, either sign) per weight column.  Column j of a layer picks input order[(j +
    shift) % in], where order lists the injected rows first (last row first), then the h rows: a layer narrower than its
    input still reaches its coordinates and modalities, and the shift moves the window over h."""
    mlp, rows = [], []
    for n_in, split, _, out in net_shape(F, M, widths, coord_layers, mod_layers):
        order = list(range(n_in - 1, split - 1, -1)) + list(range(split))
        W = np.zeros((n_in, out), np.float32)
        r = [order[(j + shift) % n_in] for j in range(out)]
        W[r, np.arange(out)] = (np.float32(2.0) ** rng.integers(-2, 3, out)).astype(np.float32) * rng.choice(np.float32([-1, 1]), out)
        b = rng.normal(0, 0.5, out).astype(np.float32) if bias else np.zeros(out, np.float32)
        mlp.append({"W": W, "b": b})
        rows.append(r)
    B = rng.normal(0, 5.0, (F // 2, 3)).astype(np.float32)
    return {"fourier": {"B": B}, "mlp": mlp}, rows


def glorot_net(rng, F, M, widths, coord_layers, mod_layers, bias=0.1):
    mlp = []
    for n_in, _, _, out in net_shape(F, M, widths, coord_layers, mod_layers):
        lim = np.sqrt(6.0 / (n_in + out))
        mlp.append({"W": rng.uniform(-lim, lim, (n_in, out)).astype(np.float32), "b": rng.normal(0, bias, out).astype(np.float32)})
    return {"fourier": {"B": rng.normal(0, 5.0, (F // 2, 3)).astype(np.float32)}, "mlp": mlp}


def integer_net(rng, F, M, widths, coord_layers, mod_layers, density=0.3):
    mlp = []
    for n_in, _, _, out in net_shape(F, M, widths, coord_layers, mod_layers):
        W = (rng.integers(-1, 2, (n_in, out)) * (rng.random((n_in, out)) < density)).astype(np.float32)
        mlp.append({"W": W, "b": rng.integers(-2, 3, out).astype(np.float32)})
    return {"fourier": {"B": np.zeros((F // 2, 3), np.float32)}, "mlp": mlp}


def flat(params):
    w = np.concatenate([np.asarray(p["W"], np.float32).reshape(-1) for p in params["mlp"]])
    b = np.concatenate([np.asarray(p["b"], np.float32).reshape(-1) for p in params["mlp"]])
    return w, b


def same_bits(a, b):
    """Equal bit patterns, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
