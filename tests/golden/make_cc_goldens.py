"""Pins the connected-component tests to scipy.ndimage.label and to the reference's own ``compute_multi_metrics``.

cc_scipy.npz: for every small case of tests/cc_cases.py and each of the three structures
``generate_binary_structure(3, connectivity)`` the int32 array ``scipy.ndimage.label`` returns and its count; for the two
larger cases (connectivity 1 and 3) the count and the SHA-256 of the int32 array's bytes.

cc_metrics.json: ``compute_multi_metrics`` is read out of the reference's notebooks/improved.ipynb at generation time (the
text of the function, from its ``def`` to the end of its cell), executed with ``np`` and the notebook's own
``from scipy.ndimage import label as connected_components_3d``, and called on the prediction / truth pairs of
cc_cases.metric_pairs().  Only the dictionaries it returns are stored.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cc_goldens.py          (needs SciPy and the reference checkout)
"""
import hashlib
import json
import pathlib
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import make_goldens  # noqa: E402
import cc_cases  # noqa: E402
import cc_ref  # noqa: E402


def _notebook_function():
    from scipy.ndimage import label as connected_components_3d
    nb = json.loads((make_goldens.REF / "notebooks" / "improved.ipynb").read_text())
    for cell in nb["cells"]:
        src = "".join(cell["source"])
        at = src.find("def compute_multi_metrics(")
        if cell["cell_type"] == "code" and at >= 0:
            ns = {"np": np, "connected_components_3d": connected_components_3d}
            exec(compile(src[at:], "improved.ipynb:compute_multi_metrics", "exec"), ns)
            return ns["compute_multi_metrics"]
    raise RuntimeError("compute_multi_metrics not found in notebooks/improved.ipynb")


def main():
    from scipy import ndimage
    out = {}
    for name, lab, mask, _ in cc_cases.small_cases():
        for conn in (1, 2, 3):
            arr, n = ndimage.label(cc_ref.inside(lab, mask), ndimage.generate_binary_structure(3, conn))
            assert arr.dtype == np.int32
            out[f"{name}_c{conn}"] = arr
            out[f"{name}_c{conn}_n"] = np.int64(n)
    for name, lab, mask in cc_cases.large_cases():
        for conn in (1, 3):
            arr, n = ndimage.label(cc_ref.inside(lab, mask), ndimage.generate_binary_structure(3, conn))
            assert arr.dtype == np.int32
            out[f"{name}_c{conn}_n"] = np.int64(n)
            out[f"{name}_c{conn}_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest())
    np.savez_compressed(HERE / "cc_scipy.npz", **out)

    fn = _notebook_function()
    metrics = {}
    for name, pred, truth in cc_cases.metric_pairs():
        metrics[name] = {k: (int(v) if isinstance(v, (int, np.integer)) else float(v)) for k, v in fn(pred, truth).items()}
    (HERE / "cc_metrics.json").write_text(json.dumps(metrics, indent=1, sort_keys=True) + "\n")
    print("connected-component goldens:", len(cc_cases.small_cases()), "small cases,", len(cc_cases.large_cases()), "large,",
          len(metrics), "metric pairs;", (HERE / "cc_scipy.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
