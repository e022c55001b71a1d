"""Pins the loss of the training tests to the reference's own ``loss_fn`` (inr/inr/model.py:64-88).

model.py is imported through the NumPy-backed ``jax`` stub of make_goldens.py, extended here by the few names its loss uses
(one_hot, log_softmax, softmax, value_and_grad as the identity: only the forward value is taken).  Two small cases are run in
fp64 and only the numbers are stored: inputs, network, and the loss / aux the reference returns.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_inr_train_goldens.py
"""
import pathlib
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import make_goldens  # noqa: E402
import inr_ref  # noqa: E402


def _log_softmax(x, axis=-1):
    s = x - x.max(axis=axis, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=axis, keepdims=True))


def main():
    model = make_goldens._import_reference_model()
    jax = model.jax
    jax.nn.one_hot = lambda labels, n: (np.asarray(labels)[..., None] == np.arange(n)).astype(np.float64)
    jax.nn.log_softmax = _log_softmax
    jax.nn.softmax = lambda x, axis=-1: np.exp(_log_softmax(x, axis))
    jax.value_and_grad = lambda f, **k: f
    out = {}
    # (K, M, hidden, hidden layers, classes, n, dice weight); the second has a class that never occurs and dice_weight 0
    for i, (K, M, hid, nh, nc, n, dw) in enumerate([(2, 1, 32, 2, 4, 40, 0.5), (1, 2, 32, 1, 3, 17, 0.0)]):
        rng = np.random.default_rng(8800 + i)
        dims = [3 + 6 * K + M] + [hid] * nh + [nc]
        layers = [{k: v.astype(np.float64) for k, v in p.items()} for p in inr_ref.fourier_params(rng, dims)]
        coords = rng.random((n, 3)) * 2 - 1
        feats = rng.standard_normal((n, M))
        labels = rng.integers(0, nc - 1 if i == 1 else nc, n)
        cw = 0.5 + rng.random(nc) * 2
        loss, aux = model.make_loss_and_grad(nc, cw, dw, K)(layers, coords, feats, labels)
        out[f"c{i}_meta"] = np.array([K, M, nc, len(layers)], np.int64)
        out[f"c{i}_dw"] = np.float64(dw)
        for l, p in enumerate(layers):
            out[f"c{i}_W{l}"], out[f"c{i}_b{l}"] = p["W"], p["b"]
        out[f"c{i}_coords"], out[f"c{i}_feats"], out[f"c{i}_labels"], out[f"c{i}_cw"] = coords, feats, labels.astype(np.int64), cw
        out[f"c{i}_loss"] = np.float64(loss)
        out[f"c{i}_ce_per_class"] = np.asarray(aux["ce_per_class"], np.float64)
        out[f"c{i}_dice_per_class"] = np.asarray(aux["dice_per_class"], np.float64)
    out["n"] = np.int64(2)
    np.savez_compressed(HERE / "inr_train_loss.npz", **out)
    print("inr training loss goldens: 2 cases")


if __name__ == "__main__":
    main()
