"""References for the INR training loop (csrc/inr_optim.hip): the definitions of DESIGN.md section 15 restated in NumPy.  No GPU.

  philox4x32_10   Philox4x32-10 (Salmon et al., SC'11) on uint32 arrays
  sample          the sampler: (case, x, y, z) of every point of a micro-batch, then coords / feats / labels
  lr_schedule     optax.warmup_cosine_decay_schedule(0, peak, warmup, decay_steps, end) in fp64
  gnorm / clip_factor / adamw_update   clip_by_global_norm + adamw, in a chosen dtype (float32 = the kernel's bits)
  train           the loop on the CPU (torch autograd of inr_train_ref for the gradients), fp64 or fp32, on the sampler's batches

``python tests/inr_loop_ref.py`` measures the trajectory tolerance and the spare factor recorded in inr_loop_cases.py.
"""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 1e-4


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints), key: two ints -> four uint32 arrays."""
    c = [np.asarray(v, np.uint64) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def mulhi32(r, m):
    return ((np.asarray(r, np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def draw(seed, batch_index, n, ncases, hwd):
    """(case, x, y, z) int64 arrays of the n points of micro-batch ``batch_index``."""
    seed, b = int(seed) & (2 ** 64 - 1), int(batch_index) & (2 ** 64 - 1)
    i = np.arange(n, dtype=np.uint64)
    r = philox4x32_10((i, b & MASK, b >> 32, 0), (seed & MASK, seed >> 32))
    return mulhi32(r[0], ncases), mulhi32(r[1], hwd[0]), mulhi32(r[2], hwd[1]), mulhi32(r[3], hwd[2])


def sample(cases, seed, batch_index, n):
    """coords (n, 3) fp32, feats (n, M) fp32, labels (n,) int32 — and the drawn indices."""
    hwd = cases[0]["seg"].shape
    cs, x, y, z = draw(seed, batch_index, n, len(cases), hwd)
    coords = np.stack([(v.astype(np.float32) / np.float32(e - 1)) * np.float32(2.0) - np.float32(1.0) for v, e in zip((x, y, z), hwd)], 1)
    mods = np.stack([np.asarray(c["mods"], np.float32) for c in cases])
    seg = np.stack([np.asarray(c["seg"]) for c in cases])
    feats = mods[cs, :, x, y, z].astype(np.float32).reshape(n, mods.shape[1])
    labels = seg[cs, x, y, z].astype(np.int32)
    return coords.astype(np.float32), feats, labels, (cs, x, y, z)


def lr_schedule(peak, end, warmup, decay_steps, t):
    T = decay_steps - warmup
    if T <= 0:
        raise ValueError("decay_steps must exceed warmup")
    if t < warmup:
        return peak * t / warmup
    u = min(t - warmup, T) / T
    a = end / peak
    return peak * ((1.0 - a) * 0.5 * (1.0 + math.cos(math.pi * u)) + a)


def gnorm(gw, gb, gscale=1.0):
    """sqrt(sum (g gscale)^2) with the scaling in fp32 and an exactly rounded fp64 sum (math.fsum of exact squares)."""
    g = np.concatenate([np.asarray(gw, np.float32).reshape(-1), np.asarray(gb, np.float32).reshape(-1)]) * np.float32(gscale)
    g = g.astype(np.float64)
    return math.sqrt(math.fsum((g * g).tolist()))


def clip_factor(norm, clip, dtype=np.float32):
    """s of the definition: evaluated in fp64, rounded once; 1 without clipping (clip <= 0 or +inf)."""
    if not (clip > 0.0 and math.isfinite(clip)):
        return dtype(1.0)
    if not math.isfinite(norm):
        return dtype(np.nan)
    return dtype(1.0 if norm < clip else clip / norm)


def adamw_update(p, mu, nu, grad, s, lr, t, gscale=1.0, b1=B1, b2=B2, eps=EPS, wd=WD, dtype=np.float32):
    """Update number t + 1, elementwise in ``dtype`` in the order of the definition.  The hyper-parameters are first rounded
    to ``dtype`` (what the C struct holds); 1 - b, 1 - b^(t+1) are evaluated in fp64 from those and rounded.  Returns (p, mu, nu)."""
    d = dtype
    b1d, b2d = float(d(b1)), float(d(b2))
    omb1, omb2 = d(1.0 - b1d), d(1.0 - b2d)
    c1, c2 = d(1.0 - math.pow(b1d, float(t + 1))), d(1.0 - math.pow(b2d, float(t + 1)))
    p, mu, nu = np.asarray(p, d), np.asarray(mu, d), np.asarray(nu, d)
    with np.errstate(all="ignore"):
        g = np.asarray(grad, d) * d(gscale)
        gc = g * d(s)
        mu = d(b1) * mu + omb1 * gc
        nu = d(b2) * nu + (omb2 * gc) * gc
        mh, nh = mu / c1, nu / c2
        upd = mh / (np.sqrt(nh) + d(eps)) + d(wd) * p
        p = p - d(lr) * upd
    assert p.dtype == d and mu.dtype == d and nu.dtype == d
    return p, mu, nu


def flat(layers, dtype=np.float32):
    return (np.concatenate([np.asarray(p["W"], dtype).reshape(-1) for p in layers]),
            np.concatenate([np.asarray(p["b"], dtype).reshape(-1) for p in layers]))


def unflat(w, b, dims):
    out, wo, bo = [], 0, 0
    for a, c in zip(dims[:-1], dims[1:]):
        out.append({"W": w[wo:wo + a * c].reshape(a, c), "b": b[bo:bo + c]})
        wo, bo = wo + a * c, bo + c
    return out


def train(layers, cases, cfg, steps, dtype_name="float64", order_seed=None, first_step=0, want_z=False):
    """The loop of the definition on the CPU: per step ``accum`` micro-batches from ``sample`` (optionally each in a random
    order: the sums over the batch then run in another order), gradients by torch autograd in ``dtype``, their sum scaled by
    1 / accum, clipped and applied by ``adamw_update`` in ``dtype``.  cfg: dict(K, classes, micro, accum, seed, cw, dw, peak,
    end, warmup, decay_steps, clip).  Returns dict(w, b flat, losses [steps][accum], z = the hidden pre-activations of the last
    micro-batch when asked)."""
    import torch
    import inr_train_ref as tr
    tdt = getattr(torch, dtype_name)
    ndt = getattr(np, dtype_name)
    dims = [layers[0]["W"].shape[0]] + [p["W"].shape[1] for p in layers]
    w, b = flat(layers, ndt)
    mu_w, mu_b, nu_w, nu_b = np.zeros_like(w), np.zeros_like(b), np.zeros_like(w), np.zeros_like(b)
    rng = np.random.default_rng(order_seed) if order_seed is not None else None
    losses, z = [], None
    for k in range(steps):
        t = first_step + k
        gw, gb, row = np.zeros_like(w), np.zeros_like(b), []
        for a in range(cfg["accum"]):
            coords, feats, labels, _ = sample(cases, cfg["seed"], t * cfg["accum"] + a, cfg["micro"])
            if rng is not None:
                perm = rng.permutation(cfg["micro"])
                coords, feats, labels = coords[perm], feats[perm], labels[perm]
            x = tr.build_input(coords, feats if feats.shape[1] else None, cfg["K"], tdt).numpy()
            r = tr.step(unflat(w, b, dims), x, tr.model_loss(labels, cfg["cw"], cfg["dw"], cfg["classes"]), tdt)
            gw = gw + np.concatenate([g[0].reshape(-1) for g in r["grads"]]).astype(ndt)
            gb = gb + np.concatenate([g[1].reshape(-1) for g in r["grads"]]).astype(ndt)
            row.append(r["loss"])
            z = r["z"][:-1]
        losses.append(row)
        gs = ndt(1.0) / ndt(cfg["accum"])
        g = np.concatenate([gw, gb]) * gs
        norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        s = clip_factor(norm, cfg["clip"], ndt)
        lr = lr_schedule(cfg["peak"], cfg["end"], cfg["warmup"], cfg["decay_steps"], t)
        w, mu_w, nu_w = adamw_update(w, mu_w, nu_w, gw, s, lr, t, gs, dtype=ndt)
        b, mu_b, nu_b = adamw_update(b, mu_b, nu_b, gb, s, lr, t, gs, dtype=ndt)
    out = dict(w=w, b=b, losses=np.asarray(losses, np.float64), dims=dims)
    if want_z:
        out["z"] = z
    return out


def layer_deviation(got, ref):
    """Worst |p - p_ref| / max |p_ref| over the layers' weight and bias arrays."""
    worst = 0.0
    for key in ("w", "b"):
        for g, r in zip(unflat_key(got, key), unflat_key(ref, key)):
            worst = max(worst, float(np.abs(np.asarray(g, np.float64) - r).max() / max(np.abs(r).max(), 1e-300)))
    return worst


def unflat_key(res, key):
    dims, arr, out, o = res["dims"], np.asarray(res[key], np.float64), [], 0
    for a, c in zip(dims[:-1], dims[1:]):
        size = a * c if key == "w" else c
        out.append(arr[o:o + size])
        o += size
    return out


def loss_deviation(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


if __name__ == "__main__":                               # the measurements recorded in inr_loop_cases.py
    import pathlib
    import sys
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
    import inr_loop_cases as cases
    c = cases.traj_case()
    ref = train(c["layers"], c["cases"], c["cfg"], cases.TRAJ_STEPS, "float64", want_z=True)
    near = max(float((np.abs(z) < 2e-5 * np.sqrt(np.mean(z * z))).any(1).mean()) for z in ref["z"])
    print("trajectory: step-%d hidden pre-activations within 2e-5 rms of 0 on %.3f %% of the points" % (cases.TRAJ_STEPS, 100 * near))
    worst_p, worst_l = 0.0, 0.0
    for order in range(5):
        got = train(c["layers"], c["cases"], c["cfg"], cases.TRAJ_STEPS, "float32", order_seed=100 + order)
        worst_p = max(worst_p, layer_deviation(got, ref))
        worst_l = max(worst_l, loss_deviation(got["losses"], ref["losses"]))
    print("trajectory: 8 x worst fp32 deviation over five orders: params %.3g losses %.3g" % (8 * worst_p, 8 * worst_l))
    e = cases.e2e_case()
    r = train(e["layers"], e["cases"], e["cfg"], e["steps"], "float64")
    per_step = r["losses"].mean(1)
    print("train_inr case: fp64 mean of the first 5 losses %.4f, of the last 5 %.4f, factor %.3f" %
          (per_step[:5].mean(), per_step[-5:].mean(), per_step[:5].mean() / per_step[-5:].mean()))
