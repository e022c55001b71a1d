"""NumPy restatement of the K1 march with an RGBA transfer-function table (mrirt_render_brats_tf).
TEST INFRASTRUCTURE ONLY.

It is the march of ``oracle_np.brats_main`` — the same helpers, imported, in the same order — with the intensity event replaced:

    u = val * float(N-1);  i = min(uint(floor(u)), N-2);  f = u - float(i)
    e[k] = lerp(tf[i][k], tf[i+1][k], f);  sigma = e[3];  the sample counts as live
    if sigma > 0:  alpha = 1 - exp(-(sigma * intensityAlpha) * stepSize)
                   C[k] += (alpha * T) * (e[k] * shade)      (unshaded: (alpha * T) * e[k]);   T *= 1 - alpha

``dtype=np.float64`` evaluates the same loop in double precision from the sample position on (ray set-up, the running t and the
loop test's t stay fp32, so both evaluations take the same samples unless T crosses the early-termination threshold
differently): the yardstick of the FAST tolerance in tf_cases.py.
"""
import numpy as np

from oracle.oracle_np import (DEFAULT_EXT, _exp, _lattice_gradient, _lerp, _pow, _sample_label, _sample_linear, _sat, make_ortho,
                              make_primary)

F = np.float32


def _vec3(v):
    a = np.asarray(v, dtype=np.float32).reshape(-1)
    return F(a[0]), F(a[1]), F(a[2])


def march(params, vols, labels, preds, ext, table, dtype=np.float32):
    """-> dict(frame (H, W, 4), live, shaded (ints), T (H, W), nsteps (H, W), seen: which table events occurred)."""
    D = dtype
    strict = D == np.float32
    exp = _exp if strict else (lambda x: np.exp(np.asarray(x, dtype=np.float64)))
    pw = _pow if strict else (lambda x, y: np.power(np.asarray(x, dtype=np.float64), np.float64(y)))
    tf = np.asarray(table, dtype=np.float32)
    assert tf.ndim == 2 and tf.shape[1] == 4 and 2 <= tf.shape[0] <= 1024
    N = tf.shape[0]
    tfD = tf.astype(D)
    e = dict(DEFAULT_EXT)
    e.update(ext or {})
    Wd, Hd = int(params["imageSize"][0]), int(params["imageSize"][1])
    X, Y, Z = (int(v) for v in params["dims"])
    bminx, bminy, bminz = _vec3(params["volMin"])
    vsx, vsy, vsz = _vec3(params["voxelSize"])
    bmaxx, bmaxy, bmaxz = bminx + vsx * F(X), bminy + vsy * F(Y), bminz + vsz * F(Z)
    step = F(params["stepSize"])
    nearT, farT = F(params["nearT"]), F(params["farT"])
    bg = np.asarray(params["bgColor"], np.float32).reshape(3)
    en = [int(v) for v in params["volEnabled"]]
    wt = [F(v) for v in params["volWeight"]]
    ww, wl, ia = F(params["ww"]), F(params["wl"]), F(params["intensityAlpha"])
    gamma = F(params["gamma"])
    showSeg, showPred = int(params["showSeg"]), int(params["showPred"])
    lut = np.asarray(params["lutColorAlpha"], np.float32).reshape(8, 4)
    ert = F(e["ertThreshold"])
    shade_on = int(e["shadeMode"]) != 0
    if int(e["cameraMode"]) == 0:
        (ox, oy, oz), (dx, dy, dz) = make_primary(Wd, Hd, params["fovY"], params["eye"], params["U"], params["V"], params["W"])
        ox, oy, oz = (np.full((Hd, Wd), o, np.float32) for o in (ox, oy, oz))
    else:
        (ox, oy, oz), (dx, dy, dz) = make_ortho(Wd, Hd, e["orthoHalfHeight"], params["eye"], params["U"], params["V"], params["W"])
    ox, oy, oz, dx, dy, dz = (np.asarray(a, np.float32).reshape(-1) for a in (ox, oy, oz, dx, dy, dz))
    n = ox.size
    eps = F(1e-6)
    ddx, ddy, ddz = (np.where(np.abs(d) < eps, eps, d) for d in (dx, dy, dz))
    rx, ry, rz = F(1.0) / ddx, F(1.0) / ddy, F(1.0) / ddz
    t0x, t1x = (bminx - ox) * rx, (bmaxx - ox) * rx
    t0y, t1y = (bminy - oy) * ry, (bmaxy - oy) * ry
    t0z, t1z = (bminz - oz) * rz, (bmaxz - oz) * rz
    tmin = np.maximum(np.maximum(np.minimum(t0x, t1x), np.minimum(t0y, t1y)), np.minimum(t0z, t1z))
    tmax = np.minimum(np.minimum(np.maximum(t0x, t1x), np.maximum(t0y, t1y)), np.maximum(t0z, t1z))
    hit = tmax >= np.maximum(tmin, F(0.0))
    t0 = np.maximum(tmin, max(F(0.0), nearT))
    t1 = np.minimum(tmax, farT) if farT > 0 else tmax
    live = hit & ~(t1 <= t0)

    volsD = [None if v is None else np.asarray(v, np.float32).astype(D) for v in vols]
    C = np.empty((n, 3), dtype=D)
    C[:] = bg
    T = np.ones(n, dtype=D)
    t = t0.astype(np.float32).copy()
    nsteps = np.zeros(n, dtype=np.int64)
    nshaded = np.zeros(n, dtype=np.int64)
    seen = dict(i_first=False, i_last=False, u_top=False, sigma_nonpos=False, sigma_above_one=False)
    one = D(1.0)
    idx = np.nonzero(live)[0]
    while idx.size:
        go = (t[idx] < t1[idx]) & (T[idx] > ert)
        idx = idx[go]
        if not idx.size:
            break
        tt = t[idx]
        ddx_, ddy_, ddz_ = dx[idx].astype(D), dy[idx].astype(D), dz[idx].astype(D)
        ttD = tt.astype(D)
        qx = ((ox[idx].astype(D) + ttD * ddx_) - D(bminx)) / D(vsx)
        qy = ((oy[idx].astype(D) + ttD * ddy_) - D(bminy)) / D(vsy)
        qz = ((oz[idx].astype(D) + ttD * ddz_) - D(bminz)) / D(vsz)
        v = np.zeros(idx.size, dtype=D)
        wsum = F(0.0)
        g = [np.zeros(idx.size, dtype=D) for _ in range(3)] if shade_on else None
        for m in range(4):
            if en[m] != 0:
                s, (ix, iy, iz, fx, fy, fz) = _sample_linear(volsD[m], qx, qy, qz, X, Y, Z)
                v = v + s * D(wt[m])
                wsum = wsum + wt[m]
                if shade_on:
                    gm = _lattice_gradient(volsD[m], ix, iy, iz, fx, fy, fz, X, Y, Z)
                    for a in range(3):
                        g[a] = g[a] + gm[a] * D(wt[m])
        if wsum > 0:
            v = v / D(wsum)
        val = _sat((v - D(wl - ww * F(0.5))) / D(ww)).astype(D)
        val = pw(val, gamma).astype(D)

        # ---- the table event ----
        u = val * D(N - 1)
        i = np.minimum(np.floor(u).astype(np.int64), N - 2)
        f = u - i.astype(D)
        ek = [_lerp(tfD[i, k], tfD[i + 1, k], f) for k in range(4)]
        sigma = ek[3]
        seen["i_first"] |= bool(np.any(i == 0))
        seen["i_last"] |= bool(np.any(i == N - 2))
        seen["u_top"] |= bool(np.any(u == D(N - 1)))
        seen["sigma_nonpos"] |= bool(np.any(sigma <= 0))
        seen["sigma_above_one"] |= bool(np.any(sigma > 1))
        Tc, Cc = T[idx], C[idx]
        pos = sigma > 0
        alpha = one - exp(-(sigma * D(ia)) * D(step)).astype(D)
        at = alpha * Tc
        if shade_on:
            gx, gy, gz = g[0] * D(F(0.5) / vsx), g[1] * D(F(0.5) / vsy), g[2] * D(F(0.5) / vsz)
            glen = np.sqrt((gx * gx + gy * gy) + gz * gz)
            ok = glen > D(F(e["gradEps"]))
            safe = np.where(ok, glen, one)
            ndl = np.fmin(np.abs((gx * ddx_ + gy * ddy_) + gz * ddz_) / safe, one)
            spec = ndl
            for _ in range(int(e["specPow2"])):
                spec = spec * spec
            shade = np.where(ok, (D(F(e["ka"])) + D(F(e["kd"])) * ndl) + D(F(e["ks"])) * spec, D(F(e["ka"]) + F(e["kd"])))
            contrib = np.stack([at * (ek[k] * shade) for k in range(3)], axis=1)
            nshaded[idx] += pos.astype(np.int64)
        else:
            contrib = np.stack([at * ek[k] for k in range(3)], axis=1)
        Cc = np.where(pos[:, None], Cc + contrib, Cc)
        Tc = np.where(pos, Tc * (one - alpha), Tc)

        # ---- label overlays: oracle_np.brats_main's ----
        for show, buf, mul in ((showSeg, labels, None), (showPred, preds, F(1.5))):
            if show != 0:
                l = _sample_label(buf, qx.astype(np.float32) if strict else qx, qy.astype(np.float32) if strict else qy,
                                  qz.astype(np.float32) if strict else qz, X, Y, Z).astype(np.int64)
                okl = (l > 0) & (l < 8)
                col = lut[np.where(okl, l, 0)]
                arg = -col[:, 3] * step
                if mul is not None:
                    arg = arg * mul
                al = (F(1.0) - _exp(arg)).astype(D)           # host-made per-label constants (prepare()): fp32 in both modes
                atl = al * Tc
                Cn = Cc + atl[:, None] * col[:, :3].astype(D)
                Cc = np.where(okl[:, None], Cn, Cc)
                Tc = np.where(okl, Tc * (one - al), Tc)
        C[idx], T[idx] = Cc, Tc
        t[idx] = tt + step
        nsteps[idx] += 1

    frame = np.empty((Hd, Wd, 4), dtype=D)
    frame[..., :3] = C.reshape(Hd, Wd, 3)
    frame[..., 3] = 1.0
    return dict(frame=frame, live=int(nsteps.sum()), shaded=int(nshaded.sum()), T=T.reshape(Hd, Wd), nsteps=nsteps.reshape(Hd, Wd), seen=seen)


def compare(got_frame, got_live, got_shaded, ref):
    """A list of what differs between a render and a reference march (empty: equal bit for bit, counters included)."""
    out = []
    a, b = np.asarray(got_frame), np.asarray(ref["frame"])
    if a.shape != b.shape or a.dtype != b.dtype:
        return [f"frame is {a.shape} {a.dtype}, the reference {b.shape} {b.dtype}"]
    if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
        bad = (a.view(np.uint32) != b.view(np.uint32)).any(axis=-1)
        out.append(f"frame differs in {int(bad.sum())} pixels, max abs {float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))):.3e}")
    if int(got_live) != ref["live"]:
        out.append(f"live samples {int(got_live)} != {ref['live']}")
    if int(got_shaded) != ref["shaded"]:
        out.append(f"shaded samples {int(got_shaded)} != {ref['shaded']}")
    return out
