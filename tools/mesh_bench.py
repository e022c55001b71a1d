"""K4 measurement: ms/frame, Grays/s and per-ray work of mrirt_render_mesh on seeded procedural meshes.

Meshes: noise-displaced icospheres of 20 480, 1 310 720 and 5 242 880 triangles (subdivisions 5, 8 and 9), normalised as
app.py does and built with the reference's median-split BVH.  Frames: 1280x720 (the app's window) and 1024^2, from an
outside camera and a close-up.  Timing: device events around single launches after warm-up, several alternating rounds;
median and min.  Pops and triangle tests per ray come from one extra launch with the stats counters (not timed).

    python tools/mesh_bench.py [--meshes 5,8,9] [--reps 20] [--rounds 3] [--json out.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_bench.py --reps 5 --rounds 1
"""
from __future__ import annotations

import argparse
import json
import pathlib
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import mrirt  # noqa: E402
from mrirt import mesh  # noqa: E402


def camera(kind: str):
    eye = np.array((1.7, 1.0, 2.2) if kind == "outside" else (0.35, 0.25, 0.95), np.float64)
    w = -eye                                            # both look at the centre of the mesh
    w /= np.linalg.norm(w)
    u = np.cross(w, (0.0, 1.0, 0.0))
    u /= np.linalg.norm(u)
    v = np.cross(u, w)
    return [x.astype(np.float32) for x in (eye, u, v, w)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="5,8,9")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for sub in [int(s) for s in a.meshes.split(",")]:
        t0 = time.time()
        v, t = mesh.icosphere(sub, noise=0.12, seed=7)
        b = mesh.build_bvh(mesh.normalize_mesh(v).astype(np.float32), t)
        dm = mesh.upload_mesh(b)
        build_s = time.time() - t0
        nbytes = dm.nodes.numel() * 4 + dm.tris.numel() * 4 + dm.verts.numel() * 4
        print(f"mesh sub={sub}: {len(t)} triangles, {dm.node_count} nodes, depth {dm.depth}, {nbytes / 1e6:.1f} MB, "
              f"built in {build_s:.1f} s", flush=True)
        cases = [(w, h, cam) for (w, h) in ((1280, 720), (1024, 1024)) for cam in ("outside", "closeup")]
        outs = {}
        for (w, h, cam) in cases:
            eye, U, V, W = camera(cam)
            p = {"imageSize": (w, h), "fovY": np.float32(np.radians(45.0)), "maxBounces": 1, "eye": eye, "U": U, "V": V, "W": W}
            outs[(w, h, cam)] = (p, torch.empty((h, w, 4), dtype=torch.float32, device="cuda"))
            for _ in range(3):
                mrirt.render_mesh(p, dm, out=outs[(w, h, cam)][1])
        torch.cuda.synchronize()
        times = {k: [] for k in outs}
        for _ in range(a.rounds):                           # alternate the cases round by round
            for k, (p, o) in outs.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * a.reps)]
                for r in range(a.reps):
                    ev[2 * r].record()
                    mrirt.render_mesh(p, dm, out=o)
                    ev[2 * r + 1].record()
                torch.cuda.synchronize()
                times[k] += [ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(a.reps)]
        for k, (p, o) in outs.items():
            _, st = mrirt.render_mesh(p, dm, out=o, stats=True)
            w, h, cam = k
            rays = w * h
            med, mn = float(np.median(times[k])), float(np.min(times[k]))
            row = dict(triangles=len(t), nodes=dm.node_count, depth=dm.depth, width=w, height=h, camera=cam,
                       ms_median=med, ms_min=mn, grays_per_s=rays / (med * 1e-3) / 1e9,
                       pops_per_ray=st["pops"] / rays, tests_per_ray=st["tests"] / rays)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        pathlib.Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
