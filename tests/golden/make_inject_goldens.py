"""Pins the coordinate-injection INR tests to the reference notebook's own functions and to SciPy's distance transform.

inject.npz: ``apply_fourier_features``, ``apply_coord_injection_mlp`` and ``predict_full_volume`` are read out of the
reference's notebooks/improved.ipynb at generation time (the text of each function), executed under a NumPy stand-in for
``jnp`` / ``jax.nn`` with ``training=False``, and called on a 12 x 10 x 8 case of four modalities with a Glorot net of the
notebook's shape (FOURIER_DIM 128, HIDDEN_DIMS 64 / 64 / 64, four classes).  Stored: the net, the modalities, the logits of the two
``apply_`` functions on the fp32 coordinate grid of the library's definition with the stand-in in float32 and in float64, and
the ``pred`` volume ``predict_full_volume`` returns with the stand-in in float32.  The seed is the first whose smallest fp64
top-two gap exceeds twice the tolerance of tests/test_gpu_inject.py, so that no voxel has to be left out of the comparison.

boundary.npz: the loop of the notebook's cell 5 (``distance_transform_edt`` per tumour class, ``1 / (1 + dist)``, running
maximum), read out of the notebook likewise, on small label volumes; the float32 map per volume.

Only data is stored.  Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_inject_goldens.py   (SciPy + the reference checkout)
"""
import json
import pathlib
import sys
import textwrap
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import make_goldens  # noqa: E402
import inject_ref as ref  # noqa: E402

HWD, M, F, WIDTHS = (12, 10, 8), 4, 128, (64, 64, 64, 4)
COORD_LAYERS, MOD_LAYERS = [1, 2, 3], [2]


def _cells():
    nb = json.loads((make_goldens.REF / "notebooks" / "improved.ipynb").read_text())
    return ["".join(c["source"]) for c in nb["cells"] if c["cell_type"] == "code"]


def _function_text(cells, name):
    for src in cells:
        at = src.find(f"def {name}(")
        if at >= 0:
            lines = src[at:].splitlines(keepends=True)
            end = next((i for i, ln in enumerate(lines[1:], 1) if ln.strip() and not ln[0].isspace()), len(lines))
            return "".join(lines[:end])
    raise RuntimeError(f"{name} not found in notebooks/improved.ipynb")


def _stand_in(dtype):
    """What the three functions use of jnp / jax.nn, on NumPy arrays of one dtype."""
    jnp = types.SimpleNamespace(pi=np.pi, dot=np.dot, concatenate=np.concatenate, sin=np.sin, cos=np.cos, where=np.where,
                                argmax=np.argmax, array=lambda x: np.asarray(x, dtype))
    jax = types.SimpleNamespace(nn=types.SimpleNamespace(relu=lambda x: np.maximum(x, 0)))
    return jnp, jax


def notebook_functions(dtype):
    cells = _cells()
    jnp, jax = _stand_in(dtype)
    ns = {"np": np, "jnp": jnp, "jax": jax, "COORD_INJECTION_LAYERS": COORD_LAYERS, "MODALITY_INJECTION_LAYERS": MOD_LAYERS}
    for name in ("apply_fourier_features", "apply_coord_injection_mlp", "predict_full_volume"):
        exec(compile(_function_text(cells, name), f"improved.ipynb:{name}", "exec"), ns)
    return ns


def _as(params, dtype):
    return {"fourier": {"B": params["fourier"]["B"].astype(dtype)}, "mlp": [{k: v.astype(dtype) for k, v in p.items()} for p in params["mlp"]]}


def notebook_logits(params, coords, mods_flat, dtype):
    ns = notebook_functions(dtype)
    p = _as(params, dtype)
    feats = ns["apply_fourier_features"](p["fourier"], coords.astype(dtype))
    return ns["apply_coord_injection_mlp"](p["mlp"], coords.astype(dtype), mods_flat.astype(dtype), feats, training=False)


def inject_fixture():
    coords = ref.grid_coords(HWD)
    for seed in range(100):
        rng = np.random.default_rng(2300 + seed)
        params = ref.glorot_net(rng, F, M, WIDTHS, COORD_LAYERS, MOD_LAYERS)
        mods = rng.normal(0, 1, (M, *HWD)).astype(np.float32)
        flat = ref.volume_mods(mods)
        z32 = ref.forward32(params, coords, flat, COORD_LAYERS, MOD_LAYERS)
        z64 = ref.forward64(params, coords, flat, COORD_LAYERS, MOD_LAYERS)
        tau = 8.0 * np.abs(z32.astype(np.float64) - z64).max()
        top = np.sort(z64, 1)
        gap = (top[:, -1] - top[:, -2]).min()
        if gap > 2 * tau:
            break
    else:
        raise RuntimeError("no seed with a top-two gap above twice the tolerance")
    nb32 = notebook_logits(params, coords, flat, np.float32)
    nb64 = notebook_logits(params, coords, flat, np.float64)
    assert nb32.dtype == np.float32 and nb64.dtype == np.float64
    ns = notebook_functions(np.float32)
    pred, seg = ns["predict_full_volume"](_as(params, np.float32), {"mods": mods, "seg": np.zeros(HWD, np.int16)}, chunk_size=300)
    assert pred.dtype == np.int16 and pred.shape == HWD
    out = {"hwd": np.int64(HWD), "mods": mods, "fourier_B": params["fourier"]["B"], "logits32": nb32, "logits64": nb64, "pred": pred,
           "coord_layers": np.int64(COORD_LAYERS), "mod_layers": np.int64(MOD_LAYERS)}
    for i, p in enumerate(params["mlp"]):                   # the notebook's own checkpoint keys (cell 14)
        out[f"mlp_W_{i}"], out[f"mlp_b_{i}"] = p["W"], p["b"]
    print(f"inject fixture: seed {2300 + seed}, smallest fp64 top-two gap {gap:.3e}, 2 tau {2 * tau:.3e}, "
          f"|notebook64 - restatement64| {np.abs(nb64 - z64).max():.3e}")
    return out


def boundary_volumes():
    rng = np.random.default_rng(5)
    vols = {}
    a = np.zeros((9, 8, 7), np.int16); a[2:5, 2:6, 1:4] = 1; a[3:5, 3:5, 2:4] = 2; a[6, 6, 5] = 3
    vols["three_classes"] = a
    b = a.copy(); b[b == 2] = 0
    vols["class_absent"] = b
    c = np.zeros((6, 5, 4), np.int16); c[0, 4, 3] = 3
    vols["one_voxel_class"] = c
    vols["no_tumour"] = np.zeros((4, 3, 5), np.int16)
    d = np.zeros((21, 3, 6), np.int16); d[1:4, 1, 2:5] = 1; d[17:, :, 0] = 2; d[10, 0, 5] = 3
    vols["anisotropic"] = d
    vols["random"] = rng.integers(0, 4, (7, 6, 5)).astype(np.int16) * (rng.random((7, 6, 5)) < 0.2)
    vols["random"] = vols["random"].astype(np.int16)
    e = np.ones((5, 4, 3), np.int16) * 2
    vols["all_one_class"] = e
    return vols


def boundary_fixture():
    from scipy.ndimage import distance_transform_edt
    text = next(src for src in _cells() if "boundary_dist = np.zeros_like(seg" in src)
    lines = text.splitlines(keepends=True)
    first = next(i for i, ln in enumerate(lines) if "boundary_dist = np.zeros_like(seg" in ln)
    last = next(i for i, ln in enumerate(lines) if "np.maximum(boundary_dist" in ln)
    loop = compile(textwrap.dedent("".join(lines[first:last + 1])), "improved.ipynb:boundary_dist", "exec")
    out = {}
    for name, seg in boundary_volumes().items():
        ns = {"np": np, "seg": seg, "NUM_CLASSES": 4, "distance_transform_edt": distance_transform_edt}
        exec(loop, ns)
        out[name + "_seg"] = seg
        out[name + "_w"] = np.asarray(ns["boundary_dist"]).astype(np.float32)
        assert ref.same_bits(out[name + "_w"], ref.boundary_weights(seg, 4)), name
    return out


def main():
    np.savez_compressed(HERE / "inject.npz", **inject_fixture())
    np.savez_compressed(HERE / "boundary.npz", **boundary_fixture())
    print("inject goldens:", (HERE / "inject.npz").stat().st_size, "and", (HERE / "boundary.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
