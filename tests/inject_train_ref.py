"""References for the coordinate-injection INR's training step (csrc/inr_inject_train.hip): the
definition of include/mrirt.h restated.  No GPU.

  forward_saved32 / 64   inject_ref's forward, keeping the features, every post-dropout activation and every pre-activation
  slab_len, slab_sum32   the split-n slabs: inside a slab the k-ordered chain of inject_ref.matmul32, the slabs added 0, 1, 2, ..
  backward32             the backward, fp32 operation by operation
  grads64                torch CPU autograd in fp64 of the same function with the restated masks, and the bound's A terms
  backward_int           the integer tier in int64
  two_stage_lr           cell 11 of notebooks/improved.ipynb, restated
"""
import numpy as np

import inject_ref as ref

TWO_PI32 = ref.TWO_PI32
DOMAIN = np.float32(1048576.0)


def slab_len(n):
    length = 256
    while (n + length - 1) // length > 64:
        length *= 2
    return length


def _masks(shapes, index, dropout):
    """Per hidden layer: None (no mask) or (kept bool [n][width], scale fp32)."""
    if dropout is None or np.float32(dropout["keep"]) == np.float32(1.0):
        return [None] * (len(shapes) - 1)
    scale = np.float32(1.0) / np.float32(dropout["keep"])
    return [(ref.keep_mask(dropout["seed"], index, dropout["s"], l, shapes[l][3], dropout["keep"]), scale) for l in range(len(shapes) - 1)]


def _unpack(params, coords, mods):
    coords = np.asarray(coords, np.float32)
    n = coords.shape[0]
    mods = np.asarray(mods, np.float32).reshape(n, -1)
    F, M = 2 * np.asarray(params["fourier"]["B"]).shape[0], mods.shape[1]
    return coords, mods, n, F, M


def _forward_saved(params, coords, mods, coord_layers, mod_layers, dropout, index, dtype):
    f32 = dtype == np.float32
    Ws = [np.asarray(p["W"], dtype) for p in params["mlp"]]
    bs = [np.asarray(p["b"], dtype) for p in params["mlp"]]
    coords, mods, n, F, M = _unpack(params, coords, mods)
    index = np.arange(n, dtype=np.uint64) if index is None else np.asarray(index, np.uint64)
    shapes = ref.net_shape(F, M, [w.shape[1] for w in Ws], coord_layers, mod_layers)
    masks = _masks(shapes, index, dropout)
    feat = ref.features32(params["fourier"]["B"], coords) if f32 else ref.features64(params["fourier"]["B"], coords)
    c, m = coords.astype(dtype), mods.astype(dtype)
    h, hs, zs = feat, [], []
    with np.errstate(all="ignore"):
        for l, (W, b, shape) in enumerate(zip(Ws, bs, shapes)):
            x = ref._layer_input(h, c, m, shape)
            z = (ref.matmul32(x, W) if f32 else x @ W) + b[None, :]
            zs.append(z)
            if l == len(Ws) - 1:
                return dict(feat=feat, h=hs, z=zs, logits=z, shapes=shapes, masks=masks)
            h = np.where(z <= 0, dtype(0), z)
            if masks[l] is not None:
                h = np.where(masks[l][0], h * dtype(masks[l][1]), dtype(0))
            hs.append(h)


def forward_saved32(params, coords, mods, coord_layers, mod_layers, dropout=None, index=None):
    return _forward_saved(params, coords, mods, coord_layers, mod_layers, dropout, index, np.float32)


def forward_saved64(params, coords, mods, coord_layers, mod_layers, dropout=None, index=None):
    return _forward_saved(params, coords, mods, coord_layers, mod_layers, dropout, index, np.float64)


def slab_sum32(x, dz, old=None):
    """sum_p x[p][i] dz[p][j] -> [in][out]: slab z over the points [z len, (z + 1) len) as the chain sums it, then old (or +0) +
    slab 0 + slab 1 + ..., one fp32 rounding per addition."""
    x, dz = np.asarray(x, np.float32), np.asarray(dz, np.float32)
    n = x.shape[0]
    length = slab_len(n)
    slabs = (n + length - 1) // length
    # every slab's chain at once; the last slab is padded with +0 rows, as the kernel's k tail is: a chain that starts at +0
    # never holds -0, so adding +0 * +0 changes nothing
    xp = np.zeros((slabs * length, x.shape[1]), np.float64)
    dp = np.zeros((slabs * length, dz.shape[1]), np.float64)
    xp[:n], dp[:n] = x, dz
    xp, dp = xp.reshape(slabs, length, -1), dp.reshape(slabs, length, -1)
    acc = np.zeros((slabs, x.shape[1], dz.shape[1]), np.float32)
    total = np.zeros((x.shape[1], dz.shape[1]), np.float32) if old is None else np.asarray(old, np.float32).reshape(x.shape[1], dz.shape[1]).copy()
    with np.errstate(all="ignore"):
        for k in range(min(length, n)):
            acc = (acc.astype(np.float64) + xp[:, k, :, None] * dp[:, k, None, :]).astype(np.float32)
        for z in range(slabs):
            total = total + acc[z]
    return total


def angles32(B, coords):
    """c01 and a = 2 pi32 p exactly as features32 forms them."""
    B, c = np.asarray(B, np.float32), np.asarray(coords, np.float32)
    with np.errstate(all="ignore"):
        u = (c + np.float32(1.0)) * np.float32(0.5)
        p = ((u[:, 0:1] * B[None, :, 0]) + (u[:, 1:2] * B[None, :, 1])) + (u[:, 2:3] * B[None, :, 2])
        return u, TWO_PI32 * p


def backward32(params, coords, mods, coord_layers, mod_layers, dlogits, dropout=None, index=None, old=None, saved=None):
    """{"B", "W": [...], "b": [...], "dz": [dz_0 .. dz_{L-1}], "dF", "g"}; old: {"B", "W", "b"} to accumulate onto."""
    sv = saved or forward_saved32(params, coords, mods, coord_layers, mod_layers, dropout, index)
    Ws = [np.asarray(p["W"], np.float32) for p in params["mlp"]]
    coords, mods, n, F, M = _unpack(params, coords, mods)
    L, half = len(Ws), F // 2
    ones = np.ones((n, 1), np.float32)
    dz = np.asarray(dlogits, np.float32)
    gW, gb, dzs = [None] * L, [None] * L, [None] * L
    with np.errstate(all="ignore"):
        for l in range(L - 1, -1, -1):
            dzs[l] = dz
            shape = sv["shapes"][l]
            x = ref._layer_input(sv["feat"] if l == 0 else sv["h"][l - 1], coords, mods, shape)
            o = None if old is None else np.concatenate([np.asarray(old["W"][l], np.float32), np.asarray(old["b"][l], np.float32)[None, :]], 0)
            s = slab_sum32(np.concatenate([x, ones], 1), dz, o)
            gW[l], gb[l] = s[:-1], s[-1]
            dh = ref.matmul32(dz, Ws[l][:shape[1]].T)
            if l == 0:
                dF = dh
                break
            if sv["masks"][l - 1] is not None:
                dh = dh * sv["masks"][l - 1][1]
            dz = np.where(sv["h"][l - 1] > 0, dh, np.float32(0)).astype(np.float32)
        c01, a = angles32(params["fourier"]["B"], coords)
        sn, cs = sv["feat"][:, :half], sv["feat"][:, half:]
        g = (dF[:, :half] * cs) - (dF[:, half:] * sn)
        g = np.where(np.abs(a) <= DOMAIN, g, np.float32(0)).astype(np.float32)
        gB = TWO_PI32 * slab_sum32(g, c01)
        if old is not None:
            gB = np.asarray(old["B"], np.float32) + gB
    return dict(B=gB.astype(np.float32), W=gW, b=gb, dz=dzs, dF=dF, g=g)


def grads64(params, coords, mods, coord_layers, mod_layers, dlogits, dropout=None, index=None):
    """torch CPU autograd in fp64 of sum(logits * dlogits) with the restated masks: {"B", "W", "b"}, and "A": the absolute
    sums |x_l|^T |dz_l| (sum_p |dz_l| for the biases, the absolute closed form for B) the tolerance tier scales its bound by;
    "z": the hidden pre-activations."""
    import torch
    coords, mods, n, F, M = _unpack(params, coords, mods)
    index = np.arange(n, dtype=np.uint64) if index is None else np.asarray(index, np.uint64)
    t = lambda v: torch.tensor(np.asarray(v, np.float64), dtype=torch.float64)
    B = t(params["fourier"]["B"]).requires_grad_(True)
    Ws = [t(p["W"]).requires_grad_(True) for p in params["mlp"]]
    bs = [t(p["b"]).requires_grad_(True) for p in params["mlp"]]
    shapes = ref.net_shape(F, M, [int(w.shape[1]) for w in Ws], coord_layers, mod_layers)
    masks = _masks(shapes, index, dropout)
    c, m = t(coords), t(mods)
    ang = 2.0 * np.pi * (((c + 1.0) / 2.0) @ B.T)
    h = torch.cat([torch.sin(ang), torch.cos(ang)], 1)
    xs, zs = [], []
    for l, shape in enumerate(shapes):
        parts = [h] + ([c] if shape[2] > shape[1] else []) + ([m] if shape[0] > shape[2] else [])
        x = torch.cat(parts, 1) if len(parts) > 1 else h
        xs.append(x)
        z = x @ Ws[l] + bs[l]
        z.retain_grad()
        zs.append(z)
        if l == len(shapes) - 1:
            break
        h = torch.relu(z)
        if masks[l] is not None:
            h = torch.where(torch.tensor(masks[l][0]), h * float(masks[l][1]), torch.zeros((), dtype=torch.float64))
    (zs[-1] * t(dlogits)).sum().backward()
    dzs = [z.grad.numpy() for z in zs]                      # dz_l = d/dz_l
    A_W = [np.abs(x.detach().numpy()).T @ np.abs(dz) for x, dz in zip(xs, dzs)]
    A_b = [np.abs(dz).sum(0) for dz in dzs]
    half = F // 2
    dF = dzs[0] @ Ws[0].detach().numpy()[:F].T
    a = ang.detach().numpy()
    absg = np.abs(dF[:, :half] * np.cos(a)) + np.abs(dF[:, half:] * np.sin(a))
    A_B = 2.0 * np.pi * (absg.T @ np.abs((coords.astype(np.float64) + 1.0) / 2.0))
    return dict(B=B.grad.numpy(), W=[w.grad.numpy() for w in Ws], b=[b.grad.numpy() for b in bs], A=dict(B=A_B, W=A_W, b=A_b),
                z=[z.detach().numpy() for z in zs[:-1]])


def relative_deviation(got, g64):
    """max over every gradient element of |got - g64| / A (elements with A == 0 must agree exactly)."""
    worst = 0.0
    for key in ("B", "W", "b"):
        gs, rs, As = ([got[key]], [g64[key]], [g64["A"][key]]) if key == "B" else (got[key], g64[key], g64["A"][key])
        for g, r, A in zip(gs, rs, As):
            d = np.abs(np.asarray(g, np.float64) - r)
            assert np.all(d[A == 0] == 0)
            if np.any(A > 0):
                worst = max(worst, float((d[A > 0] / A[A > 0]).max()))
    return worst


def near_kink(z64s, rel=2e-5):
    """bool [n]: points with a hidden pre-activation |z| < rel rms(z) of its layer (the ReLU's side is not decided in fp32)."""
    bad = np.zeros(z64s[0].shape[0], bool)
    for z in z64s:
        bad |= (np.abs(z) < rel * np.sqrt(np.mean(z * z))).any(1)
    return bad


# ---- integer tier --------------------------------------------------------------------------------------------------------------
def backward_int(params, coords8, mods, coord_layers, mod_layers, dlogits, dropout=None, index=None):
    """B = 0 (s = +0, k = 1), coords = coords8 / 8, integer mods, weights, biases and dlogits, keep in {1, 1/2, 1/4}: everything
    in int64.  {"W8": 8 dW, "b": db, "dz": [dz_l], "dF", "B16": 16 sum_p g c01, "h8": 8 h_l, "logits8", "bound": the largest
    sum of absolute terms of any dot product (forward in units of 1/8, dW in 1/8, dB in 1/16): all fp32 sums are exact while
    it stays below 2^24}."""
    Ws = [np.asarray(p["W"]).astype(np.int64) for p in params["mlp"]]
    bs = [np.asarray(p["b"]).astype(np.int64) for p in params["mlp"]]
    half = np.asarray(params["fourier"]["B"]).shape[0]
    assert not np.any(np.asarray(params["fourier"]["B"]))
    c8 = np.asarray(coords8).astype(np.int64)
    n = c8.shape[0]
    m8 = np.asarray(mods).astype(np.int64).reshape(n, -1) * 8
    index = np.arange(n, dtype=np.uint64) if index is None else np.asarray(index, np.uint64)
    shapes = ref.net_shape(2 * half, m8.shape[1], [w.shape[1] for w in Ws], coord_layers, mod_layers)
    masks = _masks(shapes, index, dropout)
    scale = [1 if mk is None else int(mk[1]) for mk in masks]
    assert all(s in (1, 2, 4) for s in scale)
    h = np.concatenate([np.zeros((n, half), np.int64), np.full((n, half), 8, np.int64)], 1)
    xs, hs, bound = [], [], 0
    for l, (W, b, shape) in enumerate(zip(Ws, bs, shapes)):
        x = ref._layer_input(h, c8, m8, shape)
        xs.append(x)
        bound = max(bound, int((np.abs(x) @ np.abs(W) + 8 * np.abs(b)[None, :]).max()))
        z = x @ W + 8 * b[None, :]
        if l == len(Ws) - 1:
            logits8 = z
            break
        h = np.maximum(z, 0)
        if masks[l] is not None:
            h = np.where(masks[l][0], h * scale[l], 0)
        bound = max(bound, int(h.max(initial=0)))
        hs.append(h)
    dz = np.asarray(dlogits).astype(np.int64)
    L = len(Ws)
    W8, db, dzs = [None] * L, [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        dzs[l] = dz
        W8[l], db[l] = xs[l].T @ dz, dz.sum(0)
        bound = max(bound, int((np.abs(xs[l]).T @ np.abs(dz)).max()), int(np.abs(dz).sum(0).max()))
        Wt = Ws[l][:shapes[l][1]].T
        dh = dz @ Wt
        bound = max(bound, int((np.abs(dz) @ np.abs(Wt)).max()))
        if l == 0:
            break
        dz = np.where(hs[l - 1] > 0, dh * scale[l - 1], 0)
        bound = max(bound, int(np.abs(dz).max(initial=0)))
    g = dh[:, :half]                                              # (dF_s * 1) - (dF_c * +0)
    c16 = c8 + 8                                                  # c01 = (c + 1) / 2 in units of 1/16
    bound = max(bound, int((np.abs(g).T @ np.abs(c16)).max()))
    return dict(W8=W8, b=db, dz=dzs, dF=dh, B16=g.T @ c16, h8=hs, logits8=logits8, bound=bound)


def dB_of_int(B16):
    """float32(2 pi32 . exact sum): the product of two fp32 numbers is exact in fp64, rounded once."""
    return (float(TWO_PI32) * (B16.astype(np.float64) / 16.0)).astype(np.float32)


# ---- schedule ------------------------------------------------------------------------------------------------------------------
def two_stage_lr(t, s1, s2, lr1, lr2, warm, floor):
    """Cell 11's formula at step t in Python floats: a linear warm-up to lr1 over `warm` steps, a linear blend lr1 -> lr2 up to
    step s1, then lr2 -> floor over s2 steps.  The last branch divides by s2: with s2 == 0 it is undefined from s1 on."""
    if t < warm:
        return lr1 * (t / warm)
    if t < s1:
        u = (t - warm) / (s1 - warm)
        return lr1 * (1.0 - u) + lr2 * u
    u = (t - s1) / s2
    return lr2 * (1.0 - u) + floor * u


# ---- scratch -------------------------------------------------------------------------------------------------------------------
def scratch_layout(F, M, widths, coord_layers, mod_layers, n, loss_bytes):
    """Byte offsets of the step's scratch regions as include/mrirt.h states them: {"feat", "h": [...], "dz": [ping, pong], "dF",
    "c01", "slab", "bytes"}; loss_bytes = mrirt_inr_loss_scratch_bytes(n).  dz_{l-1} (l >= 1) lies in dz[(L - l) & 1]."""
    al = lambda v: (v + 255) & ~255
    shapes = ref.net_shape(F, M, widths, coord_layers, mod_layers)
    out = {"feat": loss_bytes, "h": []}
    at = loss_bytes + al(4 * n * F)
    for w in widths[:-1]:
        out["h"].append(at)
        at += al(4 * n * w)
    dz = al(4 * n * max(widths[:-1]))
    out["dz"] = [at, at + dz]
    out["dF"] = at + 2 * dz
    out["c01"] = out["dF"] + al(4 * n * F)
    out["slab"] = out["c01"] + al(4 * n * 3)
    elems = max(max((s[0] + 1) * s[3] for s in shapes), 3 * F // 2)
    out["bytes"] = out["slab"] + al(4 * min((n + 255) // 256, 64) * elems)
    return out
