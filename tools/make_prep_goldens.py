#!/usr/bin/env python3
"""Writes tests/golden/prep_gauss.npz: inputs, scipy.ndimage.gaussian_filter's outputs and the weights used, so the Gaussian
pre-filter (csrc/prep.hip, tests/prep_ref.py) can be checked against SciPy where SciPy is not installed.

    python tools/make_prep_goldens.py          # needs scipy; the file is committed

Keys: ``in_<shape>`` (fp32), ``w_<sigma>`` (fp64, SciPy's own kernel), ``out_<shape>_<sigma>`` (fp32), shape as 9x8x7."""
import pathlib

import numpy as np

SHAPES = [(1, 1, 1), (2, 3, 1), (5, 1, 7), (9, 8, 7), (33, 17, 20)]
SIGMAS = [0.5, 2.3]
OUT = pathlib.Path(__file__).resolve().parent.parent / "tests" / "golden" / "prep_gauss.npz"


def tag(shape):
    return "x".join(str(v) for v in shape)


def main():
    from scipy import ndimage
    from scipy.ndimage import _filters
    rng = np.random.default_rng(20)
    data = {}
    for sigma in SIGMAS:
        data[f"w_{sigma}"] = np.asarray(_filters._gaussian_kernel1d(sigma, 0, int(4.0 * sigma + 0.5)), dtype=np.float64)
    for shape in SHAPES:
        # MRI-like: a zero background, intensities of a few thousand with a fraction, some negative values
        a = (rng.integers(-200, 4096, size=shape) * (rng.random(shape) < 0.7) + rng.random(shape)).astype(np.float32)
        data[f"in_{tag(shape)}"] = a
        for sigma in SIGMAS:
            out = ndimage.gaussian_filter(a, sigma)
            assert out.dtype == np.float32
            data[f"out_{tag(shape)}_{sigma}"] = out
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({OUT.stat().st_size} B)")


if __name__ == "__main__":
    main()
