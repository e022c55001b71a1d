"""NumPy restatement of Muon as include/mrirt.h states it (Jordan et al. 2024; optax's scale_by_muon /
orthogonalize_via_newton_schulz with its defaults).  optax and jax are not available where this was written, so nothing here
was compared with optax itself: the restatement is pinned against the algorithm's own definition (test_inr_muon_ref.py).  No GPU.

  sumsq_fixed   the fp64 sum of squares in the order of muon_norm_kernel (256 strided partial sums, folded by halves per 64,
                the four wave sums in order)
  ns            Newton-Schulz of one matrix in ``dtype`` in the stated order of roundings; ``trace`` sees every product
  momentum, apply, layer_scale     the element-wise parts of one update
  step          one whole update of a network (weights: Muon, biases: inr_loop_ref.adamw_update) around a given NS
  train         the loop of inr_loop_ref.train / inr_siren_ref.train with this update
"""
import math

import numpy as np

BETA, NESTEROV, NS_STEPS, NS_COEFFS, EPS, WEIGHT_DECAY = 0.95, True, 5, (3.4445, -4.7750, 2.0315), 1e-8, 0.0
BIAS = dict(b1=0.9, b2=0.999, eps=1e-8, wd=0.0)
THREADS = 256


def hp(beta=BETA, nesterov=NESTEROV, ns_steps=NS_STEPS, ns_coeffs=NS_COEFFS, eps=EPS, weight_decay=WEIGHT_DECAY):
    return dict(beta=beta, nesterov=bool(nesterov), ns_steps=int(ns_steps), ns_coeffs=tuple(ns_coeffs), eps=eps, weight_decay=weight_decay)


def sumsq_fixed(m):
    """fp64 sum of the squares of m's elements (flat, row-major) in the kernel's order."""
    v = np.asarray(m, np.float64).reshape(-1)
    pad = (-v.size) % THREADS
    rows = np.concatenate([v * v, np.zeros(pad)]).reshape(-1, THREADS)        # adding +0 changes nothing
    acc = np.zeros(THREADS)
    for r in rows:                                       # thread t: elements t, t + 256, ... in order
        acc = acc + r
    lanes = acc.reshape(THREADS // 64, 64).copy()
    o = 32
    while o:
        lanes[:, :o] = lanes[:, :o] + lanes[:, o:2 * o]
        o //= 2
    t = 0.0
    for w in range(THREADS // 64):
        t = t + lanes[w, 0]
    return float(t)


def ns(m, h=None, dtype=np.float32, trace=None):
    """NS(m) for m (in, out).  The struct's hyper-parameters are fp32: they are rounded to that first, whatever ``dtype``."""
    h = h or hp()
    d = dtype
    m = np.asarray(m, d)
    c0, c1, c2 = (d(np.float32(c)) for c in h["ns_coeffs"])
    with np.errstate(all="ignore"):
        denom = math.sqrt(sumsq_fixed(m)) + float(np.float32(h["eps"])) if not np.isnan(m).any() else float("nan")
        X = (m.astype(np.float64) / denom).astype(d)
        transposed = m.shape[0] > m.shape[1]
        if transposed:
            X = X.T
        for _ in range(h["ns_steps"]):
            A = np.matmul(X, X.T)
            AA = np.matmul(A, A)
            p1, p2 = c1 * A, c2 * AA
            B = p1 + p2
            BX = np.matmul(B, X)
            p0 = c0 * X
            Xn = p0 + BX
            if trace is not None:
                trace("X X^T", X, X.T, A); trace("A A", A, A, AA); trace("B X", B, X, BX)
                trace("elementwise", None, None, np.stack([v.reshape(-1) for v in (p1, p2, B)]))
                trace("elementwise", None, None, np.stack([v.reshape(-1) for v in (p0, Xn)]))
            X = Xn
        assert X.dtype == d
    return np.ascontiguousarray(X.T if transposed else X)


def split(flat, dims):
    out, o = [], 0
    for a, b in zip(dims[:-1], dims[1:]):
        out.append(np.asarray(flat[o:o + a * b]).reshape(a, b))
        o += a * b
    assert o == np.asarray(flat).size
    return out


def ns_flat(m_flat, dims, h=None, dtype=np.float32):
    """mrirt_muon_orthogonalize: every layer's matrix, flat layout in, flat layout out."""
    return np.concatenate([ns(M, h, dtype).reshape(-1) for M in split(np.asarray(m_flat, dtype), dims)])


def layer_scale(a, b, dtype=np.float32):
    return dtype(math.sqrt(max(1.0, float(b) / float(a))))


def momentum(mu, g, s, t, gscale, h, dtype=np.float32):
    """(mu', m^) of update number t + 1."""
    d = dtype
    beta = float(np.float32(h["beta"]))
    omb, c1, c2 = d(1.0 - beta), d(1.0 - math.pow(beta, float(t) + 1.0)), d(1.0 - math.pow(beta, float(t) + 2.0))
    with np.errstate(all="ignore"):
        gc = (np.asarray(g, d) * d(gscale)) * d(s)
        mu = d(np.float32(h["beta"])) * np.asarray(mu, d) + omb * gc
        mhat = d(np.float32(h["beta"])) * (mu / c2) + omb * (gc / c1) if h["nesterov"] else mu / c1
    assert mu.dtype == d and mhat.dtype == d
    return mu, mhat


def apply(w, O, lr, dims, h, dtype=np.float32):
    d = dtype
    scale = np.concatenate([np.full(a * b, layer_scale(a, b, d), d) for a, b in zip(dims[:-1], dims[1:])])
    with np.errstate(all="ignore"):
        w = np.asarray(w, d)
        out = w - d(np.float32(lr)) * (scale * np.asarray(O, d) + d(np.float32(h["weight_decay"])) * w)
    assert out.dtype == d
    return out


def step(w, b, gw, gb, mu_w, mu_b, nu_b, dims, s, lr, t, gscale, h=None, dtype=np.float32, ns_of=None, bias=None):
    """One update.  ``ns_of(mhat_flat) -> O_flat``: the orthogonalisation to wrap (default: ns_flat in ``dtype``).
    Returns dict(w, b, mu_w, mu_b, nu_b, mhat)."""
    import inr_loop_ref as lr_ref
    h, bias = h or hp(), dict(BIAS, **(bias or {}))
    mu_w, mhat = momentum(mu_w, gw, s, t, gscale, h, dtype)
    O = ns_of(mhat) if ns_of is not None else ns_flat(mhat, dims, h, dtype)
    w = apply(w, O, lr, dims, h, dtype)
    b, mu_b, nu_b = lr_ref.adamw_update(b, mu_b, nu_b, gb, s, float(np.float32(lr)), t, gscale, b1=bias["b1"], b2=bias["b2"], eps=bias["eps"],
                                        wd=bias["wd"], dtype=dtype)
    return dict(w=w, b=b, mu_w=mu_w, mu_b=mu_b, nu_b=nu_b, mhat=mhat)


def train(layers, cases, cfg, steps, dtype_name="float64", h=None):
    """inr_loop_ref.train (cfg without "w0") or inr_siren_ref.train (cfg with it) with the Muon update.  Returns dict(w, b,
    losses [steps][accum], dims)."""
    import torch
    import inr_loop_ref as lr_ref
    import inr_siren_ref as sr
    import inr_train_ref as tr
    tdt, ndt = getattr(torch, dtype_name), getattr(np, dtype_name)
    dims = [layers[0]["W"].shape[0]] + [p["W"].shape[1] for p in layers]
    w, b = lr_ref.flat(layers, ndt)
    mu_w, mu_b, nu_b = np.zeros_like(w), np.zeros_like(b), np.zeros_like(b)
    losses = []
    for t in range(steps):
        gw, gb, row = np.zeros_like(w), np.zeros_like(b), []
        for a in range(cfg["accum"]):
            coords, feats, labels, _ = lr_ref.sample(cases, cfg["seed"], t * cfg["accum"] + a, cfg["micro"])
            loss_of = tr.model_loss(labels, cfg["cw"], cfg["dw"], cfg["classes"])
            if "w0" in cfg:
                r = sr.step(lr_ref.unflat(w, b, dims), sr.input_matrix(coords, feats if feats.shape[1] else None), cfg["w0"], loss_of, tdt)
            else:
                r = tr.step(lr_ref.unflat(w, b, dims), tr.build_input(coords, feats if feats.shape[1] else None, cfg["K"], tdt).numpy(), loss_of, tdt)
            gw = gw + np.concatenate([g[0].reshape(-1) for g in r["grads"]]).astype(ndt)
            gb = gb + np.concatenate([g[1].reshape(-1) for g in r["grads"]]).astype(ndt)
            row.append(r["loss"])
        losses.append(row)
        gs = ndt(1.0) / ndt(cfg["accum"])
        norm = float(np.sqrt(np.sum((np.concatenate([gw, gb]) * gs).astype(np.float64) ** 2)))
        s = lr_ref.clip_factor(norm, cfg["clip"], ndt)
        rate = lr_ref.lr_schedule(cfg["peak"], cfg["end"], cfg["warmup"], cfg["decay_steps"], t)
        r = step(w, b, gw, gb, mu_w, mu_b, nu_b, dims, s, rate, t, gs, h, ndt)
        w, b, mu_w, mu_b, nu_b = r["w"], r["b"], r["mu_w"], r["mu_b"], r["nu_b"]
    return dict(w=w, b=b, losses=np.asarray(losses, np.float64), dims=dims)
