"""Reference of the soft prediction overlay and its backward pass (mrirt_render_brats_soft / _backward).  TEST INFRASTRUCTURE ONLY.

The ray set-up, t0 / t1, the running t and the samples' index-space positions, cells and fractions are taken in fp32 exactly as
the oracle takes them (oracle/oracle_np.py's helpers through brats_grad_ref.py); values, transfer function, the soft event
(include/mrirt.h) and the compositing loop then run in torch — float64 with CPU autograd for the reference proper, and once more
in float32 (``dtype=torch.float32``: the soft event's alpha and c still come from fp64 and are rounded once, as the definition
says) for the reference's OWN fp32 deviation, which sets the GPU tolerances.  ``closed_form`` evaluates the formulas of
include/mrirt.h per sample on the forward's records and also yields A, the same expression with every term replaced by its
absolute value and G . R by |G| . (|C_final| + |C_after|): the scale the gradient comparisons are relative to.
"""
from types import SimpleNamespace

import numpy as np
import torch

import brats_grad_ref as gref
from oracle import oracle_np as onp

F = np.float32
DRAWN = 8


def geometry(case):
    """Rays of the case and the whole-ray sample numbering: counts[p] = steps of ray p in [t0, t1) with the march's own running
    fp32 sum (mrirt_brats_sample_counts), no early termination."""
    p, ext = case["params"], case["ext"]
    o, d, t0, t1, live, bmin, vs = gref._rays(p, ext)
    step = F(p["stepSize"])
    counts = np.zeros(o[0].size, np.int64)
    t = t0.copy()
    idx = np.nonzero(live)[0]
    while idx.size:
        idx = idx[t[idx] < t1[idx]]
        counts[idx] += 1
        t[idx] = t[idx] + step
    return SimpleNamespace(o=o, d=d, t0=t0, t1=t1, live=live, bmin=bmin, vs=vs, counts=counts)


def make_offsets(counts, mode):
    """(offsets int64 [pixels], rows): "natural" = exclusive prefix sum in pixel order (what the package computes); "reversed" =
    the rays laid out from the LAST pixel to the first, three gap rows in front and two between consecutive rays."""
    if mode == "natural":
        ends = np.cumsum(counts)
        return (ends - counts).astype(np.int64), int(ends[-1]) if counts.size else 0
    off = np.zeros(counts.size, np.int64)
    cur = 3
    for pix in range(counts.size - 1, -1, -1):
        off[pix] = cur
        cur += int(counts[pix]) + 2
    return off, cur


def soft_event(z, lut, D):
    """z: (n, C) float64 torch.  Returns (p, sigma, has, alpha, c) in float64 (alpha, c are 0 where there is no event)."""
    C = z.shape[1]
    Kc = min(C, DRAWN)
    p = torch.softmax(z, dim=1)
    w = torch.from_numpy(lut[:Kc, 3].astype(np.float64))
    rgb = torch.from_numpy(lut[:Kc, :3].astype(np.float64))
    pk = p[:, 1:Kc]
    sigma = (pk * w[1:]).sum(1)
    E = (pk * w[1:]).unsqueeze(2).mul(rgb[1:].unsqueeze(0)).sum(1)
    has = sigma > 0
    ss = torch.where(has, sigma, torch.ones_like(sigma))
    alpha = torch.where(has, 1 - torch.exp(-ss * D), torch.zeros_like(sigma))
    c = torch.where(has[:, None], E / ss[:, None], torch.zeros_like(E))
    return p, sigma, has, alpha, c


def forward(case, data, logits=None, dtype=torch.float64, record=False, geo=None):
    """The frame: C (H*W, 3) torch tensor of ``dtype`` (with a graph when ``logits`` requires grad).  ``logits``: torch (rows, C) of
    any float dtype (default: the case's fp32 logits); the soft event is always evaluated from them in float64.  ``record``: also
    the per-step records ``closed_form`` and the margin test need, and the number of composited samples."""
    p, ext = case["params"], case["ext"]
    X, Y, Z = case["dims"]
    D = dtype
    nD = np.float64 if D == torch.float64 else np.float32
    en = [int(v) for v in p["volEnabled"]]
    vols = [None if v is None else torch.from_numpy(v.astype(nD)) for v in data["vols"]]
    if logits is None:
        logits = torch.from_numpy(np.array(data["logits"]))           # (a copy: the case's arrays are read-only)
    z_all = logits.to(torch.float64)
    off = data["offsets"]
    ww, wl, ia, gamma = (float(F(p[k])) for k in ("ww", "wl", "intensityAlpha", "gamma"))
    wt = [float(F(v)) for v in p["volWeight"]]
    wsum = F(0.0)
    for m in range(4):
        if en[m]:
            wsum = wsum + F(p["volWeight"][m])
    wsum = float(wsum)
    step = F(p["stepSize"])
    dt = float(step)
    Dp = dt * 1.5
    ert = float(F(ext.get("ertThreshold", 0.01)))
    lut = np.asarray(p["lutColorAlpha"], np.float32).reshape(8, 4)
    g = geo or geometry(case)
    o, d, t1, bmin, vs = g.o, g.d, g.t1, g.bmin, g.vs
    n = o[0].size
    Cc_all = torch.tensor(np.asarray(p["bgColor"], np.float32).astype(nD)).repeat(n, 1)
    T_all = torch.ones(n, dtype=D)
    t = g.t0.copy()
    idx = np.nonzero(g.live)[0]
    k = np.zeros(n, np.int64)
    steps, composited = [], 0
    while idx.size:
        Tn = T_all.detach().numpy()[idx].astype(np.float64)
        go = (t[idx] < t1[idx]) & (Tn > ert)
        margin_T = np.abs(Tn - ert) / ert
        margin_t = np.abs(t[idx].astype(np.float64) - t1[idx]) / np.spacing(np.abs(t1[idx])).astype(np.float64)
        idx = idx[go]
        if not idx.size:
            if record:
                steps.append(SimpleNamespace(idx=idx, margin_T=margin_T, margin_t=margin_t, empty=True))
            break
        composited += idx.size
        tt = t[idx]
        q = [((o[a][idx] + tt * d[a][idx]) - bmin[a]) / vs[a] for a in range(3)]
        (ix, fx), (iy, fy), (iz, fz) = gref._cell(q[0], X), gref._cell(q[1], Y), gref._cell(q[2], Z)
        base = ix + iy * X + iz * X * Y
        offs = [0, 1, X, X + 1, X * Y, X * Y + 1, X * Y + X, X * Y + X + 1]
        f = [torch.from_numpy(a.astype(nD)) for a in (fx, fy, fz)]
        cw = [(f[0] if b & 1 else 1 - f[0]) * (f[1] if b & 2 else 1 - f[1]) * (f[2] if b & 4 else 1 - f[2]) for b in range(8)]
        v = torch.zeros(idx.size, dtype=D)
        for m in range(4):
            if en[m]:
                v = v + sum(cw[b] * vols[m][torch.from_numpy(base + offs[b])] for b in range(8)) * wt[m]
        if wsum > 0:
            v = v / wsum
        u = (v - (wl - ww * 0.5)) / ww
        inside = (u > 0) & (u < 1)
        us = torch.where(inside, u, torch.full_like(u, 0.5))
        val = torch.where(inside, torch.exp(gamma * torch.log(us)), (u >= 1).to(D))
        pos = val > 0
        alpha = 1 - torch.exp(-val * ia * dt)
        Tc, Cc = T_all[idx], Cc_all[idx]
        Cc = torch.where(pos[:, None], Cc + (alpha * Tc * val)[:, None], Cc)
        Tc = torch.where(pos, Tc * (1 - alpha), Tc)
        if int(p["showSeg"]):
            l = onp._sample_label(data["labels"], q[0], q[1], q[2], X, Y, Z).astype(np.int64)
            okl = (l > 0) & (l < 8)
            col = lut[np.where(okl, l, 0)]
            al = torch.from_numpy(np.where(okl, (onp._ONE - onp._exp(-col[:, 3] * step)), F(0.0)).astype(nD))   # the host-made fp32 opacity
            Cc = Cc + (al * Tc)[:, None] * torch.from_numpy(col[:, :3].astype(nD))
            Tc = Tc * (1 - al)
        rows = off[idx] + k[idx]
        pz, sigma, has, a64, c64 = soft_event(z_all[torch.from_numpy(rows)], lut, Dp)
        Tb = Tc
        aD, cD = a64.to(D), c64.to(D)                                  # fp32: each rounded once
        Cc = Cc + (aD * Tc)[:, None] * cD
        Tc = Tc * (1 - aD)
        Cc_all = Cc_all.index_put((torch.from_numpy(idx),), Cc)
        T_all = T_all.index_put((torch.from_numpy(idx),), Tc)
        t[idx] = tt + step
        k[idx] += 1
        if record:
            steps.append(SimpleNamespace(idx=idx, rows=rows, p=pz.detach().numpy(), sigma=sigma.detach().numpy(), has=has.numpy(),
                                         alpha=a64.detach().numpy(), c=c64.detach().numpy(), T=Tb.detach().numpy().astype(np.float64),
                                         C_after=Cc.detach().numpy().astype(np.float64), margin_T=margin_T, margin_t=margin_t,
                                         empty=False))
    if record:
        return Cc_all, SimpleNamespace(steps=steps, composited=composited, Dp=Dp, lut=lut, geo=g,
                                       C_final=Cc_all.detach().numpy().astype(np.float64))
    return Cc_all


def loss(C, G):
    g = torch.from_numpy(np.asarray(G, np.float64).reshape(-1, 4)[:, :3]).to(C.dtype)
    return (C * g).sum()


def autograd(case, data, geo=None):
    """(dlogits float64 (rows, C), frame (H*W, 3) float64) by torch autograd of the float64 forward."""
    z = torch.from_numpy(data["logits"].astype(np.float64)).requires_grad_(True)
    C = forward(case, data, z, geo=geo)
    L = loss(C, data["G"])
    if L.requires_grad:
        L.backward()
    return (np.zeros(z.shape) if z.grad is None else z.grad.numpy().copy()), C.detach().numpy()


def closed_form(case, data, dtype=np.float64, geo=None):
    """The formulas of include/mrirt.h per sample on the records of the forward run in ``dtype``.  ``dtype=float32``: the ray state
    (T, C_after, C_final) is the fp32 forward's and the chain itself runs in fp32 — the reference's own fp32 error.
    Returns dlogits and A, both float64 (rows, C) (rows no event writes are zeros), the frame, and the records."""
    D = dtype
    Cfr, rec = forward(case, data, dtype=torch.float64 if D is np.float64 else torch.float32, record=True, geo=geo)
    rows_total, Cn = data["logits"].shape
    Kc = min(Cn, DRAWN)
    dl = np.zeros((rows_total, Cn), np.float64)
    A = np.zeros((rows_total, Cn), np.float64)
    G = np.asarray(data["G"], np.float64).reshape(-1, 4)[:, :3].astype(D)
    w = rec.lut[:Kc, 3].astype(D)
    rgb = rec.lut[:Kc, :3].astype(D)
    Dp = D(rec.Dp)
    Cf = rec.C_final.astype(D)
    samples = []
    for s in rec.steps:
        if s.empty or not s.has.any():
            continue
        h = s.has
        g, T, al, c, sg, p = G[s.idx][h], s.T.astype(D)[h], s.alpha.astype(D)[h], s.c.astype(D)[h], s.sigma.astype(D)[h], s.p.astype(D)[h]
        Ca, Cfi = s.C_after.astype(D)[h], Cf[s.idx][h]
        R = Cfi - Ca
        gR = (g * R).sum(1)
        gc = (g * c).sum(1)
        om = D(1) - al
        dA = om * T * gc - gR
        Ta = T * al
        gk = g @ (w[:, None] * rgb).T                                  # (n, Kc): w_k G . rgb_k
        dp = w[None, :] * Dp * dA[:, None] + Ta[:, None] * (gk - w[None, :] * gc[:, None]) / sg[:, None]
        dp[:, 0] = 0
        mean = (p[:, :Kc] * dp).sum(1)
        full = np.zeros((g.shape[0], Cn), D)
        full[:, :Kc] = dp
        dl[s.rows[h]] = (p * (full - mean[:, None])).astype(np.float64)
        # A: every term by its absolute value, G . R by |G| . (|C_final| + |C_after|)
        ag = np.abs(g.astype(np.float64))
        T6, al6, sg6, p6 = T.astype(np.float64), al.astype(np.float64), sg.astype(np.float64), p.astype(np.float64)
        w6, rgb6 = rec.lut[:Kc, 3].astype(np.float64), rec.lut[:Kc, :3].astype(np.float64)
        gca = (ag * np.abs(c.astype(np.float64))).sum(1)
        gRa = (ag * (np.abs(Cfi.astype(np.float64)) + np.abs(Ca.astype(np.float64)))).sum(1)
        dAa = (1 - al6) * T6 * gca + gRa
        gka = ag @ (w6[:, None] * np.abs(rgb6)).T
        dpa = w6[None, :] * rec.Dp * dAa[:, None] + (T6 * al6)[:, None] * (gka + w6[None, :] * gca[:, None]) / sg6[:, None]
        dpa[:, 0] = 0
        meana = (p6[:, :Kc] * dpa).sum(1)
        fulla = np.zeros((g.shape[0], Cn))
        fulla[:, :Kc] = dpa
        A[s.rows[h]] = p6 * (fulla + meana[:, None])
        samples.append(np.concatenate([s.rows[h][:, None].astype(np.float64), T6[:, None], g.astype(np.float64), gR.astype(np.float64)[:, None]], 1))
    return SimpleNamespace(dlogits=dl, A=A, frame=Cfr.detach().numpy().astype(np.float64), rec=rec,
                           samples=np.concatenate(samples) if samples else np.zeros((0, 6)))


# --- the end-to-end composition: MLP + render, float64 autograd to the weights --------------------------------------------------
def mlp_inputs(case, data, geo=None):
    """(coords (rows, 3), feats (rows, 4)) fp32 of every march sample at its row (oracle_np.inr_sample_inputs: what
    mrirt_brats_emit_samples writes), rows no sample owns are zeros."""
    p = case["params"]
    X, Y, Z = case["dims"]
    g = geo or geometry(case)
    rows_total = data["rows"]
    coords = np.zeros((rows_total, 3), np.float32)
    feats = np.zeros((rows_total, 4), np.float32)
    step = F(p["stepSize"])
    t = g.t0.copy()
    idx = np.nonzero(g.live)[0]
    k = np.zeros(g.counts.size, np.int64)
    while idx.size:
        idx = idx[t[idx] < g.t1[idx]]
        if not idx.size:
            break
        tt = t[idx]
        q = [((g.o[a][idx] + tt * g.d[a][idx]) - g.bmin[a]) / g.vs[a] for a in range(3)]
        c, f = onp.inr_sample_inputs(data["vols"], (X, Y, Z), data["zmu"], data["zsigma"], q[0], q[1], q[2])
        rows = data["offsets"][idx] + k[idx]
        coords[rows], feats[rows] = c, f
        t[idx] = tt + step
        k[idx] += 1
    return coords, feats


def apply_net(net, Ws, bs, coords, feats):
    """Logits of the network in the dtype of Ws: net = ("siren", w0) on x = (coords, feats), or ("fourier", K) on
    build_input(coords, feats, K) (inr/inr/model.py:11-50)."""
    D = Ws[0].dtype
    c, f = coords.to(D), feats.to(D)
    if net[0] == "siren":
        h = torch.cat([c, f], 1)
        for i, (W, b) in enumerate(zip(Ws[:-1], bs[:-1])):
            z = h @ W
            h = torch.sin(float(net[1]) * z + b) if i == 0 else torch.sin(z + b)
        return h @ Ws[-1] + bs[-1]
    K = int(net[1])
    freqs = torch.arange(1, K + 1, dtype=D)
    ang = c[:, :, None] * freqs[None, None, :] * np.pi
    x = torch.cat([c, torch.cat([torch.sin(ang), torch.cos(ang)], -1).reshape(c.shape[0], -1), f], 1)
    h = x
    for W, b in zip(Ws[:-1], bs[:-1]):
        h = torch.relu(h @ W + b)
    return h @ Ws[-1] + bs[-1]


def weight_abs_scale(net, Ws, bs, coords, feats, A_logits):
    """A of grad_w / grad_b: the backward pass of the network with every term replaced by its absolute value, started from the
    render's A per logit (float64)."""
    D = torch.float64
    Ws, bs = [W.detach().to(D) for W in Ws], [b.detach().to(D) for b in bs]
    c, f = coords.to(D), feats.to(D)
    acts, slopes = [], []
    if net[0] == "siren":
        h = torch.cat([c, f], 1)
        for i, (W, b) in enumerate(zip(Ws[:-1], bs[:-1])):
            acts.append(h)
            s = float(net[1]) if i == 0 else 1.0
            pre = s * (h @ W) + b
            slopes.append((torch.cos(pre).abs(), abs(s)))
            h = torch.sin(pre)
    else:
        K = int(net[1])
        freqs = torch.arange(1, K + 1, dtype=D)
        ang = c[:, :, None] * freqs[None, None, :] * np.pi
        h = torch.cat([c, torch.cat([torch.sin(ang), torch.cos(ang)], -1).reshape(c.shape[0], -1), f], 1)
        for W, b in zip(Ws[:-1], bs[:-1]):
            acts.append(h)
            pre = h @ W + b
            slopes.append(((pre > 0).to(D), 1.0))
            h = torch.relu(pre)
    acts.append(h)
    delta = torch.from_numpy(A_logits)
    Aw, Ab = [None] * len(Ws), [None] * len(Ws)
    for i in range(len(Ws) - 1, -1, -1):
        if i < len(Ws) - 1:
            delta = delta * slopes[i][0]                               # |d act / d pre|
            Ab[i] = delta.sum(0)
            Aw[i] = (acts[i].abs().T @ delta) * slopes[i][1]
        else:
            Ab[i] = delta.sum(0)
            Aw[i] = acts[i].abs().T @ delta
        delta = (delta * (slopes[i][1] if i < len(Ws) - 1 else 1.0)) @ Ws[i].abs().T
    return [a.numpy() for a in Aw], [a.numpy() for a in Ab]


def end_to_end(case, data, net, layers, dtype=torch.float64, geo=None, coords=None, feats=None):
    """grad_w / grad_b (lists of float64 arrays) and the frame of L = sum G . C through MLP + render, by autograd in ``dtype``."""
    g = geo or geometry(case)
    if coords is None:
        coords, feats = mlp_inputs(case, data, g)
    Ws = [torch.from_numpy(np.asarray(p["W"], np.float64)).to(dtype).requires_grad_(True) for p in layers]
    bs = [torch.from_numpy(np.asarray(p["b"], np.float64)).to(dtype).requires_grad_(True) for p in layers]
    logits = apply_net(net, Ws, bs, torch.from_numpy(coords), torch.from_numpy(feats))
    C = forward(case, data, logits, dtype=dtype, geo=g)
    L = loss(C, data["G"])
    if L.requires_grad:
        L.backward()
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy().astype(np.float64)
    return [zero(W) for W in Ws], [zero(b) for b in bs], C.detach().numpy().astype(np.float64), logits.detach()


def fit_loop(cases, views, teacher, start, net, steps, rate, dtype_name="float64"):
    """The fitting loop of mrirt.inr.fit_views on the CPU in ``dtype``: targets rendered from ``teacher``, per step the sum over
    the views of mean((frame - target)^2), gradients by autograd, one AdamW update (inr_loop_ref.adamw_update: no clipping, no
    weight decay, constant rate).  Returns the loss of every step before its update."""
    import inr_loop_ref as loop
    tdt, ndt = getattr(torch, dtype_name), getattr(np, dtype_name)
    geos = [geometry(c) for c in cases]
    inputs = [mlp_inputs(c, d, g) for c, d, g in zip(cases, views, geos)]

    def frames(layers, grad):
        Ws = [torch.from_numpy(np.asarray(p["W"], np.float64)).to(tdt).requires_grad_(grad) for p in layers]
        bs = [torch.from_numpy(np.asarray(p["b"], np.float64)).to(tdt).requires_grad_(grad) for p in layers]
        out = []
        for c, d, g, (co, fe) in zip(cases, views, geos, inputs):
            out.append(forward(c, d, apply_net(net, Ws, bs, torch.from_numpy(co), torch.from_numpy(fe)), dtype=tdt, geo=g))
        return out, Ws, bs
    with torch.no_grad():
        targets = [f.detach() for f in frames(teacher, False)[0]]
    dims = [start[0]["W"].shape[0]] + [p["W"].shape[1] for p in start]
    w, b = loop.flat(start, ndt)
    mu_w, mu_b, nu_w, nu_b = np.zeros_like(w), np.zeros_like(b), np.zeros_like(w), np.zeros_like(b)
    losses = []
    for step in range(steps):
        fr, Ws, bs = frames(loop.unflat(w, b, dims), True)
        L = sum(((f - t) ** 2).mean() for f, t in zip(fr, targets))
        L.backward()
        gw = np.concatenate([W.grad.numpy().reshape(-1) for W in Ws])
        gb = np.concatenate([x.grad.numpy().reshape(-1) for x in bs])
        w, mu_w, nu_w = loop.adamw_update(w, mu_w, nu_w, gw, 1.0, rate, step, wd=0.0, dtype=ndt)
        b, mu_b, nu_b = loop.adamw_update(b, mu_b, nu_b, gb, 1.0, rate, step, wd=0.0, dtype=ndt)
        losses.append(float(L.detach()))
    return losses
