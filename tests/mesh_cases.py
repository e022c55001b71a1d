"""Shared K4 test inputs: the fixture meshes (tests/golden/mesh_*.npz, the reference's build_bvh output) and cameras."""
from __future__ import annotations

import pathlib

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
MESHES = ("cube", "ico3", "ico4", "torus", "degenerate", "one")


def fixture(name: str):
    return dict(np.load(GOLDEN / f"mesh_{name}.npz"))


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    eye, target, up = (np.asarray(x, dtype=np.float64) for x in (eye, target, up))
    w = target - eye
    w /= np.linalg.norm(w)
    u = np.cross(w, up)
    u /= np.linalg.norm(u)
    v = np.cross(u, w)
    return [np.asarray(x, dtype=np.float32) for x in (eye, u, v, w)]


# name -> (eye, U, V, W)
CAMERAS = {
    "outside": look_at((1.1, 0.9, 1.6), (0.0, 0.0, 0.0)),
    "inside": look_at((0.05, 0.03, 0.02), (1.0, 0.2, -0.3)),
    # exactly axis-aligned directions: the centre pixel of an odd-sized image (and every orthographic ray) has two zero
    # components, which meet the shader's 1e-8 clamp before 1 / d
    "axis": [np.array(x, np.float32) for x in ((0.0, 0.0, 2.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0))],
    # nearly in the plane z = 0 of the flat fixtures, and along a face of the cube
    "grazing": look_at((2.0, 0.05, 0.0008), (-1.0, -0.02, 0.0)),
}


def params(camera: str, width: int, height: int, fov_deg: float = 45.0):
    eye, U, V, W = CAMERAS[camera]
    return {"imageSize": (width, height), "fovY": np.float32(np.radians(fov_deg)), "maxBounces": 1,
            "eye": eye, "U": U, "V": V, "W": W}
