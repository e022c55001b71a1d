"""NumPy restatement of K4 `compute_main` (scripts/mesh_rt/mesh_rt.slang:26-164), written from the shader.

Vectorised over rays: every ray keeps its own stack and pops one node per iteration while it has any.  All arithmetic is fp32
in the shader's written order (NumPy's fp32 + - * / sqrt are correctly rounded, as the kernel's); HLSL min / max are fmin /
fmax (a NaN operand yields the other one).  The camera is the library's: tan(fovY / 2) correctly rounded on the host, aspect
W / H, the orthographic extension as csrc/mrirt_device.h primary_ray.

render(...) -> (rgba f32 [H, W, 4] or [P, 4], pops int64 [...], tests int64 [...])
"""
from __future__ import annotations

import math
from typing import Mapping, Optional, Tuple

import numpy as np

f32 = np.float32


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _normalize(x, y, z):
    n = np.sqrt(_dot(x, y, z, x, y, z))
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / n, y / n, z / n


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def primary_rays(params: Mapping, px: np.ndarray, py: np.ndarray, camera_mode: int = 0, ortho_half_height: float = 1.1):
    W, H = int(params["imageSize"][0]), int(params["imageSize"][1])
    eye, U, V, Wv = (np.asarray(params[k], dtype=f32).reshape(3) for k in ("eye", "U", "V", "W"))
    th = f32(math.tan(float(f32(0.5) * f32(params["fovY"]))))
    inv = f32(1.0) / th
    aspect = f32(W) / f32(H)
    uvx = ((px.astype(f32) + f32(0.5)) / f32(W)) * f32(2.0) - f32(1.0)
    uvy = ((py.astype(f32) + f32(0.5)) / f32(H)) * f32(2.0) - f32(1.0)
    if camera_mode == 0:
        cx, cy, cz = uvx * aspect / inv, -uvy / inv, np.ones_like(uvx)
        cx, cy, cz = _normalize(cx, cy, cz)
        d = [(cx * U[k] + cy * V[k]) + cz * Wv[k] for k in range(3)]
        d = list(_normalize(*d))
        o = [np.full_like(uvx, eye[k]) for k in range(3)]
    else:
        ohh = f32(ortho_half_height)
        sx, sy = uvx * ohh * aspect, -uvy * ohh
        o = [(eye[k] + U[k] * sx) + V[k] * sy for k in range(3)]
        d = [np.full_like(uvx, Wv[k]) for k in range(3)]
    return o, d


def _aabb(o, rcp, a, b):
    bmin = (a[:, 0], a[:, 1], a[:, 2])
    bmax = (a[:, 3], b[:, 0], b[:, 1])
    tsm, tbg = [], []
    for k in range(3):
        t0 = (bmin[k] - o[k]) * rcp[k]
        t1 = (bmax[k] - o[k]) * rcp[k]
        tsm.append(np.fmin(t0, t1))
        tbg.append(np.fmax(t0, t1))
    tN = np.fmax(np.fmax(tsm[0], tsm[1]), tsm[2])
    tF = np.fmin(np.fmin(tbg[0], tbg[1]), tbg[2])
    return tF >= np.fmax(tN, f32(0.0)), tN


def _tri_hit(o, d, A, B, Cv):
    ab = [B[:, k] - A[:, k] for k in range(3)]
    ac = [Cv[:, k] - A[:, k] for k in range(3)]
    p = _cross(d, ac)
    det = _dot(*ab, *p)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        fail = np.abs(det) < f32(1e-8)
        inv = f32(1.0) / det
        s = [o[k] - A[:, k] for k in range(3)]
        u = _dot(*s, *p) * inv
        fail |= (u < 0) | (u > 1)
        q = _cross(s, ab)
        v = _dot(*d, *q) * inv
        fail |= (v < 0) | (u + v > 1)
        th = _dot(*ac, *q) * inv
        fail |= th <= f32(1e-5)
    return ~fail, th


def trace(o, d, nodes, tris, verts):
    """bvhTrace over rays: (hit t, winning triangle index or -1, pops, tests)."""
    nodes = np.asarray(nodes, dtype=f32).reshape(-1, 8)
    R = len(o[0])
    rcp = []
    for k in range(3):
        dd = d[k].copy()
        small = np.abs(dd) < f32(1e-8)
        dd[small] = np.where(dd[small] >= 0, f32(1e-8), f32(-1e-8))
        with np.errstate(divide="ignore"):
            rcp.append(f32(1.0) / dd)
    stack = np.zeros((R, 66), dtype=np.int64)
    sp = np.ones(R, dtype=np.int64)
    hit_t = np.full(R, f32(1e30), dtype=f32)
    hit_tri = np.full(R, -1, dtype=np.int64)
    pops = np.zeros(R, dtype=np.int64)
    tests = np.zeros(R, dtype=np.int64)
    lf_all = np.trunc(nodes[:, 6] + f32(0.5)).astype(np.int64)
    w = nodes[:, 7]
    cr_all = np.trunc(w + np.where(w >= 0, f32(0.5), f32(-0.5)).astype(f32)).astype(np.int64)
    while True:
        act = np.nonzero(sp > 0)[0]
        if len(act) == 0:
            break
        sp[act] -= 1
        ni = stack[act, sp[act]]
        pops[act] += 1
        oa = [o[k][act] for k in range(3)]
        ra = [rcp[k][act] for k in range(3)]
        hit, tmin = _aabb(oa, ra, nodes[ni, 0:4], nodes[ni, 4:8])
        keep = hit & ~(tmin > hit_t[act])
        act, ni = act[keep], ni[keep]
        oa = [x[keep] for x in oa]
        ra = [x[keep] for x in ra]
        lf, cr = lf_all[ni], cr_all[ni]
        leaf = cr > 0
        # leaves: triangles in order, the hit replaced on a strict t < hit.t
        if leaf.any():
            la, llf, lcr = act[leaf], lf[leaf], cr[leaf]
            lo = [x[leaf] for x in oa]
            ld = [d[k][la] for k in range(3)]
            for i in range(int(lcr.max())):
                m = i < lcr
                ti = llf[m] + i
                rays = la[m]
                tests[rays] += 1
                idx = tris[ti, :3].astype(np.int64)
                ok, t = _tri_hit([x[m] for x in lo], [x[m] for x in ld], verts[idx[:, 0], :3], verts[idx[:, 1], :3],
                                 verts[idx[:, 2], :3])
                upd = ok & (t < hit_t[rays])
                hit_t[rays[upd]] = t[upd]
                hit_tri[rays[upd]] = ti[upd]
        inn = ~leaf
        if inn.any():
            ia = act[inn]
            l, r = lf[inn], -cr[inn] - 1
            io = [x[inn] for x in oa]
            ir = [x[inn] for x in ra]
            hl, tl = _aabb(io, ir, nodes[l, 0:4], nodes[l, 4:8])
            hr, tr = _aabb(io, ir, nodes[r, 0:4], nodes[r, 4:8])
            both = hl & hr
            near_left = tl < tr
            first = np.where(both, np.where(near_left, r, l), np.where(hl, l, r))
            second = np.where(near_left, l, r)
            n = hl.astype(np.int64) + hr.astype(np.int64)
            s = sp[ia]
            m1 = n >= 1
            stack[ia[m1], s[m1]] = first[m1]
            m2 = n == 2
            stack[ia[m2], s[m2] + 1] = second[m2]
            sp[ia] += n
    return hit_t, hit_tri, pops, tests


def shade(o, d, hit_t, hit_tri, tris, verts):
    R = len(hit_t)
    rgb = np.zeros((R, 3), dtype=f32)
    h = hit_t < f32(1e29)
    if h.any():
        idx = tris[hit_tri[h], :3].astype(np.int64)
        A, B, Cv = verts[idx[:, 0], :3], verts[idx[:, 1], :3], verts[idx[:, 2], :3]
        ab = [B[:, k] - A[:, k] for k in range(3)]
        ac = [Cv[:, k] - A[:, k] for k in range(3)]
        n = _normalize(*_normalize(*_cross(ab, ac)))
        dh = [d[k][h] for k in range(3)]
        flip = _dot(*n, *dh) > 0
        n = [np.where(flip, -x, x) for x in n]
        lx, ly, lz = _normalize(f32(0.3), f32(0.8), f32(0.5))
        ndotl = np.fmax(f32(0.0), _dot(*n, lx, ly, lz))
        s = f32(1.0) - f32(0.05) * hit_t[h]
        sat = np.where(np.isnan(s), f32(0.0), np.clip(s, f32(0.0), f32(1.0))).astype(f32)
        ao = f32(0.3) + f32(0.7) * sat
        k = (f32(0.15) + ndotl) * ao
        rgb[h] = np.stack([k * f32(0.8), k * f32(0.7), k * f32(0.6)], axis=1)
    m = ~h
    if m.any():
        _, y, _ = _normalize(d[0][m], d[1][m], d[2][m])
        tbg = f32(0.5) * (y + f32(1.0))
        for c, (a, b) in enumerate(((0.05, 0.2), (0.06, 0.25), (0.08, 0.3))):
            rgb[m, c] = f32(a) + tbg * (f32(b) - f32(a))
    return rgb


def render(params: Mapping, nodes: np.ndarray, tris: np.ndarray, verts: np.ndarray, camera_mode: int = 0,
           ortho_half_height: float = 1.1, pixels: Optional[Tuple[np.ndarray, np.ndarray]] = None):
    """The frame (or the pixels (px, py)) compute_main draws, with per-ray pop and triangle-test counts."""
    W, H = int(params["imageSize"][0]), int(params["imageSize"][1])
    if pixels is None:
        py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        px, py = px.reshape(-1), py.reshape(-1)
    else:
        px, py = np.asarray(pixels[0]).reshape(-1), np.asarray(pixels[1]).reshape(-1)
    tris = np.asarray(tris).reshape(len(tris), -1)
    verts = np.asarray(verts, dtype=f32).reshape(len(verts), -1)
    o, d = primary_rays(params, px, py, camera_mode, ortho_half_height)
    hit_t, hit_tri, pops, tests = trace(o, d, nodes, tris, verts)
    rgba = np.ones((len(px), 4), dtype=f32)
    rgba[:, :3] = shade(o, d, hit_t, hit_tri, tris, verts)
    if pixels is None:
        return rgba.reshape(H, W, 4), pops.reshape(H, W), tests.reshape(H, W)
    return rgba, pops, tests


def brute_force(params: Mapping, tris: np.ndarray, verts: np.ndarray, camera_mode: int = 0, ortho_half_height: float = 1.1):
    """Closest hit over ALL triangles, no BVH: (hit mask [H*W], t [H*W])."""
    W, H = int(params["imageSize"][0]), int(params["imageSize"][1])
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    o, d = primary_rays(params, px.reshape(-1), py.reshape(-1), camera_mode, ortho_half_height)
    tris = np.asarray(tris).reshape(len(tris), -1)
    verts = np.asarray(verts, dtype=f32).reshape(len(verts), -1)
    best = np.full(len(o[0]), f32(1e30), dtype=f32)
    for i in range(len(tris)):
        A, B, Cv = (np.broadcast_to(verts[int(tris[i, j]), :3], (len(best), 3)) for j in range(3))
        ok, t = _tri_hit(o, d, A, B, Cv)
        upd = ok & (t < best)
        best[upd] = t[upd]
    return best < f32(1e29), best
