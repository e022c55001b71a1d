"""fp64 reference of the K1 backward pass (mrirt_render_brats_backward).  TEST INFRASTRUCTURE ONLY.

The ray set-up, t0 / t1, the running t and the samples' index-space positions, cells and fractions are taken in fp32 exactly as
the oracle takes them (oracle/oracle_np.py: the same helpers and the same expressions); values, transfer function and the
compositing loop then run in float64 — with torch CPU autograd for the gradients of L = sum G . C, and once more as the closed
form of include/mrirt.h / csrc/brats_grad.h, which also yields A, the sum of the ABSOLUTE per-sample contributions (per voxel for
the grids, one number per transfer-function scalar): the scale the comparisons are relative to.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import oracle_np as onp

F = np.float32


def _rays(params, ext):
    """origins, directions, t0, t1, live — brats_rt.slang:91-109 in the oracle's fp32 (oracle_np.brats_main)."""
    Wd, Hd = int(params["imageSize"][0]), int(params["imageSize"][1])
    X, Y, Z = (int(v) for v in params["dims"])
    bmin = onp._vec3(params["volMin"])
    vs = onp._vec3(params["voxelSize"])
    bmax = tuple(bmin[k] + vs[k] * F(d) for k, d in enumerate((X, Y, Z)))
    if int(ext.get("cameraMode", 0)) == 0:
        o, d = onp.make_primary(Wd, Hd, params["fovY"], params["eye"], params["U"], params["V"], params["W"])
        o = [np.full((Hd, Wd), v, np.float32) for v in o]
    else:
        o, d = onp.make_ortho(Wd, Hd, ext["orthoHalfHeight"], params["eye"], params["U"], params["V"], params["W"])
    o = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in o]
    d = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in d]
    eps = F(1e-6)
    tmin = np.full(o[0].size, -np.inf, np.float32)
    tmax = np.full(o[0].size, np.inf, np.float32)
    for k in range(3):
        r = onp._ONE / np.where(np.abs(d[k]) < eps, eps, d[k])
        ta, tb = (bmin[k] - o[k]) * r, (bmax[k] - o[k]) * r
        tmin = np.maximum(tmin, np.minimum(ta, tb))
        tmax = np.minimum(tmax, np.maximum(ta, tb))
    nearT, farT = F(params["nearT"]), F(params["farT"])
    hit = tmax >= np.maximum(tmin, onp._ZERO)
    t0 = np.maximum(tmin, max(onp._ZERO, nearT)).astype(np.float32)
    t1 = (np.minimum(tmax, farT) if farT > 0 else tmax).astype(np.float32)
    return o, d, t0, t1, hit & ~(t1 <= t0), bmin, vs


def _cell(q, n):
    c = np.minimum(np.maximum(q, onp._ZERO), F(n) - F(1.001))
    fl = np.floor(c)
    return fl.astype(np.int64), (c - fl).astype(np.float32)


def forward(case, data, vols=None, tf=None, record=False):
    """The frame in float64: C (H*W, 3) torch tensor (with a graph when vols / tf require grad).  ``vols``: four float64 torch
    tensors or None (default: the case's), ``tf``: float64 tensor (ww, wl, intensityAlpha, gamma) (default: the case's).
    ``record``: also return the per-step records the closed form needs."""
    p, ext = case["params"], case["ext"]
    X, Y, Z = case["dims"]
    en = [int(v) for v in p["volEnabled"]]
    if vols is None:
        vols = [None if v is None else torch.from_numpy(v.astype(np.float64)) for v in data["vols"]]
    if tf is None:
        tf = torch.tensor([float(F(p[k])) for k in ("ww", "wl", "intensityAlpha", "gamma")], dtype=torch.float64)
    ww, wl, ia, gamma = tf[0], tf[1], tf[2], tf[3]
    wt = [float(F(v)) for v in p["volWeight"]]
    wsum = F(0.0)
    for m in range(4):
        if en[m]:
            wsum = wsum + F(p["volWeight"][m])                     # fp32, slot order: the host's a.wsum
    wsum = float(wsum)
    step = F(p["stepSize"])
    dt = float(step)
    ert = float(F(ext.get("ertThreshold", 0.01)))
    lut = np.asarray(p["lutColorAlpha"], np.float32).reshape(8, 4)
    o, d, t0, t1, live, bmin, vs = _rays(p, ext)
    n = o[0].size
    C = torch.tensor(np.asarray(p["bgColor"], np.float32).astype(np.float64)).repeat(n, 1)
    T = torch.ones(n, dtype=torch.float64)
    t = t0.copy()
    idx = np.nonzero(live)[0]
    steps = []
    while idx.size:
        go = (t[idx] < t1[idx]) & (T.detach().numpy()[idx] > ert)
        margin_T = np.abs(T.detach().numpy()[idx] - ert)
        idx = idx[go]
        if not idx.size:
            break
        tt = t[idx]
        q = [((o[k][idx] + tt * d[k][idx]) - bmin[k]) / vs[k] for k in range(3)]
        (ix, fx), (iy, fy), (iz, fz) = _cell(q[0], X), _cell(q[1], Y), _cell(q[2], Z)
        base = ix + iy * X + iz * X * Y
        offs = [0, 1, X, X + 1, X * Y, X * Y + 1, X * Y + X, X * Y + X + 1]
        fx64, fy64, fz64 = (torch.from_numpy(a.astype(np.float64)) for a in (fx, fy, fz))
        cw = [(fx64 if b & 1 else 1 - fx64) * (fy64 if b & 2 else 1 - fy64) * (fz64 if b & 4 else 1 - fz64) for b in range(8)]
        v = torch.zeros(idx.size, dtype=torch.float64)
        for m in range(4):
            if en[m]:
                s = sum(cw[b] * vols[m][torch.from_numpy(base + offs[b])] for b in range(8))
                v = v + s * wt[m]
        if wsum > 0:
            v = v / wsum
        u = (v - (wl - ww * 0.5)) / ww
        inside = (u > 0) & (u < 1)
        us = torch.where(inside, u, torch.full_like(u, 0.5))
        val = torch.where(inside, torch.exp(gamma * torch.log(us)), (u >= 1).to(torch.float64))
        pos = val > 0
        alpha = 1 - torch.exp(-val * ia * dt)
        Tc, Cc = T[idx], C[idx]
        Cc = torch.where(pos[:, None], Cc + (alpha * Tc * val)[:, None], Cc)
        Tb = Tc
        Tc = torch.where(pos, Tc * (1 - alpha), Tc)
        C_after = Cc
        for show, buf, mul in ((int(p["showSeg"]), data["labels"], None), (int(p["showPred"]), data["preds"], F(1.5))):
            if show:
                l = onp._sample_label(buf, q[0], q[1], q[2], X, Y, Z).astype(np.int64)
                okl = (l > 0) & (l < 8)
                col = lut[np.where(okl, l, 0)]
                arg = -col[:, 3] * step
                if mul is not None:
                    arg = arg * mul
                al = torch.from_numpy(np.where(okl, (onp._ONE - onp._exp(arg)), F(0.0)).astype(np.float64))   # the host-made fp32 opacity
                Cc = Cc + (al * Tc)[:, None] * torch.from_numpy(col[:, :3].astype(np.float64))
                Tc = Tc * (1 - al)
        C = C.index_put((torch.from_numpy(idx),), Cc)
        T = T.index_put((torch.from_numpy(idx),), Tc)
        t[idx] = tt + step
        if record:
            steps.append(SimpleNamespace(idx=idx, base=base, offs=offs, cw=np.stack([w.numpy() for w in cw], 1), ix=ix, iy=iy, iz=iz,
                                         fx=fx, fy=fy, fz=fz, v=v.detach().numpy(), u=u.detach().numpy(), val=val.detach().numpy(),
                                         alpha=alpha.detach().numpy(), T=Tb.detach().numpy(), C_after=C_after.detach().numpy(),
                                         margin_T=margin_T[go]))
    if record:
        return C, SimpleNamespace(steps=steps, wsum=wsum, wt=wt, en=en, dt=dt, C_final=C.detach().numpy(), n=n)
    return C


def loss(C, G):
    g = torch.from_numpy(np.asarray(G, np.float64).reshape(-1, 4)[:, :3])
    return (C * g).sum()


def autograd(case, data):
    """(grad_vols [4 x (X*Y*Z) float64 | None], grad_tf float64 [4], frame (H*W, 3) float64) by torch autograd."""
    vols = [None if v is None else torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for v in data["vols"]]
    p = case["params"]
    tf = torch.tensor([float(F(p[k])) for k in ("ww", "wl", "intensityAlpha", "gamma")], dtype=torch.float64, requires_grad=True)
    C = forward(case, data, vols, tf)
    L = loss(C, data["G"])
    if L.requires_grad:
        L.backward()
    gv = [None if v is None else (np.zeros(v.numel()) if v.grad is None else v.grad.numpy().copy()) for v in vols]
    return gv, (np.zeros(4) if tf.grad is None else tf.grad.numpy().copy()), C.detach().numpy()


def closed_form(case, data, dtype=np.float64, shuffle=None):
    """The formulas of include/mrirt.h evaluated per sample on the forward's records.  Returns a namespace with grad_vols, A_vols
    (per voxel), grad_tf, A_tf (4 each), plus `samples` (what tests/native/brats_grad_harness.hip replays).  ``dtype=float32,
    shuffle=seed``: every quantity rounded to fp32, fp32 arithmetic, and the per-voxel (and per-scalar) terms summed one by one in
    fp32 in a shuffled order — the reference's own fp32 error, which sets the GPU tolerance."""
    D = dtype
    p = case["params"]
    _, rec = forward(case, data, record=True)
    nvox = int(np.prod(case["dims"]))
    G = np.asarray(data["G"], np.float64).reshape(-1, 4)[:, :3].astype(D)
    ww, wl, ia, gam = (D(F(p[k])) for k in ("ww", "wl", "intensityAlpha", "gamma"))
    dt, wsum = D(rec.dt), D(rec.wsum)
    Cf = rec.C_final.astype(D)
    vox_idx = [[] for _ in range(4)]
    vox_val = [[] for _ in range(4)]
    tf_terms = [[] for _ in range(4)]
    samples = []
    for s in rec.steps:
        v, T = s.v.astype(D), s.T.astype(D)
        g = G[s.idx]
        g1 = (g[:, 0] + g[:, 1]) + g[:, 2]
        Rc = Cf[s.idx] - s.C_after.astype(D)
        gR = (g[:, 0] * Rc[:, 0] + g[:, 1] * Rc[:, 1]) + g[:, 2] * Rc[:, 2]
        if D is np.float64:
            u, val, alpha = s.u, s.val, s.alpha
        else:
            u = (v - (wl - ww * D(0.5))) / ww
            ins = (u > 0) & (u < 1)
            val = np.where(ins, np.exp(gam * np.log(np.where(ins, u, D(0.5)))), (u >= 1).astype(D)).astype(D)
            alpha = (D(1) - np.exp(-val * ia * dt)).astype(D)
        pos = val > 0
        ins = (u > 0) & (u < 1)
        om = D(1) - alpha
        ad = ia * dt
        dval = T * g1 * (alpha + val * ad * om) - ad * gR
        da = np.where(pos, (T * val * g1 * om - gR) * val * dt, D(0))
        us = np.where(ins, u, D(0.5))
        du = np.where(ins, dval * gam * val / us, D(0))
        dgam = np.where(ins, dval * val * np.log(us), D(0))
        dv = du / ww
        dwl = -du / ww
        dww = -du * (v - wl) / (ww * ww)
        for k, term in enumerate((dww, dwl, da, dgam)):
            tf_terms[k].append(term.astype(D))
        nz = dv != 0
        cw = s.cw.astype(D)
        for m in range(4):
            if rec.en[m]:
                ds = dv * D(rec.wt[m]) / wsum if rec.wsum > 0 else dv * D(rec.wt[m])
                for b in range(8):
                    vox_idx[m].append((s.base + s.offs[b])[nz])
                    vox_val[m].append((ds * cw[:, b])[nz].astype(D))
        samples.append(np.stack([s.ix, s.iy, s.iz, s.fx, s.fy, s.fz, s.v, s.T, g1, gR], 1).astype(np.float64))
    rng = np.random.default_rng(shuffle) if shuffle is not None else None

    def total(idx, val, size):
        out, A = np.zeros(size, D), np.zeros(size, np.float64)
        if idx:
            i, x = np.concatenate(idx), np.concatenate(val)
            if rng is not None:
                perm = rng.permutation(i.size)
                i, x = i[perm], x[perm]
            np.add.at(out, i, x)                                   # one add at a time, in this order, in dtype D
            np.add.at(A, i, np.abs(x.astype(np.float64)))
        return out, A
    gv, Av = [], []
    for m in range(4):
        if rec.en[m]:
            o_, a_ = total(vox_idx[m], vox_val[m], nvox)
            gv.append(o_); Av.append(a_)
        else:
            gv.append(None); Av.append(None)
    gtf, Atf = np.zeros(4, D), np.zeros(4)
    for k in range(4):
        terms = [x for x in tf_terms[k]]
        o_, a_ = total([np.zeros(x.size, np.int64) for x in terms], terms, 1)
        gtf[k], Atf[k] = o_[0], a_[0]
    return SimpleNamespace(grad_vols=gv, A_vols=Av, grad_tf=gtf, A_tf=Atf, rec=rec,
                           samples=np.concatenate(samples) if samples else np.zeros((0, 10)))
