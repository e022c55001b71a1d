"""Generate the K4 fixtures: tests/golden/mesh_*.npz and mesh_*.ply.

Run once, by hand, with MESH_RT_DIR naming the reference checkout's scripts/mesh_rt: the fixtures record what the reference's own bvh.build_bvh and ply_loader.load_ply_ascii return.
No test imports the reference; the tests compare against these files.

    MESH_RT_DIR=/path/to/MRI-RayTracer/scripts/mesh_rt python tests/golden/make_mesh_goldens.py
"""
from __future__ import annotations

import os
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
if "MESH_RT_DIR" not in os.environ:
    sys.exit("set MESH_RT_DIR to the reference's scripts/mesh_rt directory")
sys.path.insert(0, os.environ["MESH_RT_DIR"])

import bvh as ref_bvh                # noqa: E402  (the reference)
import ply_loader as ref_ply         # noqa: E402  (the reference)
from mrirt import mesh               # noqa: E402


def cube():
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32)
    t = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.uint32)
    return v, t


def degenerate():
    """Zero-area triangles (a repeated vertex, three collinear vertices), a triangle listed twice, two coplanar overlapping
    triangles, and a few ordinary ones around them."""
    v = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [0, 0, 0], [0.5, 0, 0],
                  [-1, -1, 0.5], [1, -1, 0.5], [0, 1, 0.5], [-0.5, -0.5, -0.5], [0.5, -0.5, -0.5], [0, 0.5, -0.5]],
                 dtype=np.float32)
    t = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 2], [4, 4, 5], [0, 4, 2], [0, 5, 4], [6, 7, 8], [6, 7, 8], [6, 8, 7],
                  [9, 10, 11], [9, 11, 10], [1, 2, 4], [0, 1, 1]], dtype=np.uint32)
    return v, t


def meshes():
    yield "cube", cube()
    yield "ico3", mesh.icosphere(3)
    yield "ico4", mesh.icosphere(4, noise=0.1, seed=4)
    yield "torus", mesh.torus(24, 12)
    yield "degenerate", degenerate()
    yield "one", (np.array([[-0.5, -0.5, 0.0], [0.5, -0.4, 0.1], [0.0, 0.6, -0.1]], np.float32), np.array([[0, 1, 2]], np.uint32))


ASCII_PLY = """ply
format ascii 1.0
comment made by make_mesh_goldens.py: extra vertex properties, a quad, a short face line
element vertex 6
property float x
property float y
property float z
property float nx
property float ny
property float nz
property uchar red
element face 6
property list uchar int vertex_indices
end_header
0 0 0 0 0 1 255
1 0 0 0 0 1 255
1 1 0 0 0 1 255
0 1 0 0 0 1 255
0.5 0.5 1.25 0 0 1 12
0.1 0.2 0.3 0 0 1 7
3 0 1 2
4 0 1 2 3
3 0 2 3
3 0 1 4
3 1 2 4
3 2 3 4 5
"""


def main():
    for name, (v, t) in meshes():
        vn = mesh.normalize_mesh(v).astype(np.float32)
        b = ref_bvh.build_bvh(vn, t, max_leaf_tris=4)
        np.savez_compressed(HERE / f"mesh_{name}.npz", verts=vn, tris=t, nodes=b.nodes, bvh_tris=b.tris, bvh_verts=b.vert_pos)
        print(name, len(t), "triangles", len(b.nodes), "nodes")
    p = HERE / "mesh_ascii.ply"
    p.write_text(ASCII_PLY)
    out = {}
    for mf in (None, 2, 3):
        v, t = ref_ply.load_ply_ascii(p, max_faces=mf)
        key = "all" if mf is None else f"max{mf}"
        out[f"verts_{key}"], out[f"tris_{key}"] = v, t
    v, t = cube()
    cp = HERE / "mesh_cube.ply"
    cp.write_text("ply\nformat ascii 1.0\ncomment the 12-triangle cube\nelement vertex 8\nproperty float x\nproperty float y\n"
                  "property float z\nelement face 12\nproperty list uchar int vertex_indices\nend_header\n"
                  + "".join(f"{x:g} {y:g} {z:g}\n" for x, y, z in v) + "".join(f"3 {a} {b} {c}\n" for a, b, c in t))
    out["verts_cube"], out["tris_cube"] = ref_ply.load_ply_ascii(cp)
    np.savez_compressed(HERE / "mesh_ply.npz", **out)
    print("ply fixtures:", sorted(out))


if __name__ == "__main__":
    main()
