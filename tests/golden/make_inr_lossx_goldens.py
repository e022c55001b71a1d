"""Pins the extended loss of the training tests to the reference's own ``loss_fn`` (scripts/jax_inr_brats.py:205-257).

jax_inr_brats.py is imported through the NumPy-backed ``jax`` stub of make_goldens.py, the way make_inr_train_goldens.py
imports model.py, extended by the names its loss uses (one_hot, log_softmax, softmax, softplus), by a stub of
``optax.softmax_cross_entropy`` and by empty ``nibabel`` / ``scipy.ndimage`` modules (its loaders are not called).  ``loss_fn``
takes a network and inputs, not logits: it is given K = 0, zero coordinates, the logits as the four "intensities" and one
linear layer W = [0 (3 x 4); I (4 x 4)], b = 0, so that its logits are the given numbers exactly.  Evaluated in fp64 with
C = 4 (the script's NUM_CLASSES); only numbers are stored: logits, labels, options and the value ``loss_fn`` returns.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_inr_lossx_goldens.py
"""
import pathlib
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import make_goldens  # noqa: E402

C = 4
# name: (loss_fn keywords, labels: "all" | "no_edema" | "edema_only")
CASES = {
    "focal": (dict(focal_gamma=2.0), "all"),
    "focal_alpha": (dict(focal_gamma=1.0, focal_alpha=np.array([0.25, 1.0, 0.5, 2.0])), "all"),
    "smoothing": (dict(label_smoothing=0.05, dice_weight=0.5, per_class_dice=True), "all"),
    "dice_prevalence": (dict(dice_weight=0.5, per_class_dice=False), "all"),
    "dice_per_class": (dict(dice_weight=0.5, per_class_dice=True), "all"),
    "edema_fp": (dict(edema_fp_weight=0.3), "all"),
    "tversky": (dict(tversky_weight=0.4, tversky_alpha=0.8, tversky_beta=0.2), "all"),
    "logit_reg": (dict(edema_logit_reg=0.2), "all"),
    "all": (dict(focal_gamma=2.0, focal_alpha=np.array([0.25, 1.0, 0.5, 2.0]), label_smoothing=0.05, dice_weight=0.5, per_class_dice=False,
                 edema_fp_weight=0.3, tversky_weight=0.4, tversky_alpha=0.7, tversky_beta=0.3, edema_logit_reg=0.2), "all"),
    "all_no_edema": (dict(focal_gamma=2.0, label_smoothing=0.05, dice_weight=0.5, per_class_dice=False, edema_fp_weight=0.3,
                          tversky_weight=0.4, edema_logit_reg=0.2), "no_edema"),
    "all_edema_only": (dict(focal_gamma=2.0, label_smoothing=0.05, dice_weight=0.5, per_class_dice=False, edema_fp_weight=0.3,
                            tversky_weight=0.4, edema_logit_reg=0.2), "edema_only"),
}
N = 37


def _log_softmax(x, axis=-1):
    s = x - x.max(axis=axis, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=axis, keepdims=True))


def _import_reference_script():
    optax = types.ModuleType("optax")
    optax.softmax_cross_entropy = lambda logits, labels: -(labels * _log_softmax(logits)).sum(-1)
    nib = types.ModuleType("nibabel")
    scipy, ndimage = types.ModuleType("scipy"), types.ModuleType("scipy.ndimage")
    ndimage.gaussian_filter = None
    scipy.ndimage = ndimage
    extra = {"optax": optax, "nibabel": nib, "scipy": scipy, "scipy.ndimage": ndimage}
    saved = {k: sys.modules.get(k) for k in extra}
    real_load = make_goldens._load
    sys.modules.update(extra)
    make_goldens._load = lambda path, name: real_load(make_goldens.REF / "scripts/jax_inr_brats.py", "ref_jax_inr_brats")
    try:
        mod = make_goldens._import_reference_model()      # installs the jax stub around the load
    finally:
        make_goldens._load = real_load
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    jax = mod.jax
    jax.nn.one_hot = lambda labels, n: (np.asarray(labels)[..., None] == np.arange(n)).astype(np.float64)
    jax.nn.log_softmax = _log_softmax
    jax.nn.softmax = lambda x, axis=-1: np.exp(_log_softmax(x, axis))
    jax.nn.softplus = lambda x: np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    return mod


def main():
    script = _import_reference_script()
    assert script.NUM_CLASSES == C
    params = [{"W": np.concatenate([np.zeros((3, C)), np.eye(C)]), "b": np.zeros(C)}]
    out = {"names": np.array(sorted(CASES))}
    for i, name in enumerate(sorted(CASES)):
        kw, which = CASES[name]
        rng = np.random.default_rng(9100 + i)
        logits = rng.uniform(-4, 4, (N, C))
        labels = {"all": rng.integers(0, C, N), "no_edema": rng.choice([0, 1, 3], N), "edema_only": np.full(N, 2)}[which].astype(np.int64)
        cw = 0.5 + rng.random(C) * 2
        loss = script.loss_fn(params, np.zeros((N, 3)), logits, labels, 0, None, None, class_weights=cw, **kw)
        out[f"{name}_logits"], out[f"{name}_labels"], out[f"{name}_cw"], out[f"{name}_loss"] = logits, labels, cw, np.float64(loss)
        for k, v in kw.items():
            out[f"{name}_opt_{k}"] = np.asarray(v, np.float64)
    np.savez_compressed(HERE / "inr_lossx.npz", **out)
    print("inr extended loss goldens:", len(CASES), "cases")


if __name__ == "__main__":
    main()
