"""Pins the unified-loss tests to the reference notebook's own loss.

unified_loss.npz: ``unified_focal_loss``, ``dice_loss``, ``compute_tv_loss`` and the lines of ``loss_fn`` that follow its forward
pass (the four terms, their combination, the aux dict) are read out of the reference's notebooks/improved.ipynb at generation
time, executed under a NumPy stand-in for ``jnp`` / ``jax.nn`` in float64, and called on the configurations of
tests/unified_loss_cases.py (GOLDEN_CASES: C in {1, 3, 4}, an absent class, labels outside the range, logits beyond +-10,
saturated probabilities, both TV weights, gamma 0.25 / 0.5 / 1, lambda 0 / 0.5 / 1, no boundary weights).  Stored per case: the
inputs (logits, labels, boundary weights), the configuration, and the fp64 values of ``loss`` and of every aux entry in the ABI's
order.  For C == 1 the notebook's mean over no tumour class is NaN; the library defines 0 there and 0 is stored.

Only numbers are stored, no text of the functions.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_unified_loss_goldens.py   (needs the reference checkout)
"""
import pathlib
import sys
import textwrap
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import make_inject_goldens as mig  # noqa: E402
import unified_loss_cases as uc  # noqa: E402
import unified_loss_ref as ref  # noqa: E402


def _softmax(x, axis=-1):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def _one_hot(labels, num_classes):
    labels = np.asarray(labels)
    return (labels[:, None] == np.arange(num_classes)[None, :]).astype(np.float64)      # all 0 for a label outside the range


def _stand_in():
    """What the four pieces use of jnp / jax, on NumPy fp64 arrays."""
    jnp = types.SimpleNamespace(clip=np.clip, power=np.power, stack=np.stack, sum=np.sum, log=np.log, ones=np.ones, var=np.var,
                                argmax=np.argmax, abs=np.abs, mean=np.mean, array=lambda x: np.asarray(x, np.float64))
    jax = types.SimpleNamespace(jit=lambda f: f, nn=types.SimpleNamespace(softmax=_softmax, one_hot=_one_hot))
    return jnp, jax


def _combining_lines(cells):
    """loss_fn from the line that calls unified_focal_loss to the end of its aux dict, dedented."""
    text = mig._function_text(cells, "loss_fn")
    lines = text.splitlines(keepends=True)
    first = next(i for i, ln in enumerate(lines) if "unified_focal_loss(logits, labels)" in ln)
    start = next(i for i, ln in enumerate(lines) if ln.strip().startswith("aux = {"))
    last = next(i for i in range(start, len(lines)) if lines[i].strip() == "}")
    return textwrap.dedent("".join(lines[first:last + 1]))


def notebook_loss(z, labels, bw, cfg):
    """(loss, aux dict) of the notebook's functions in fp64."""
    cells = mig._cells()
    jnp, jax = _stand_in()
    C = z.shape[1]
    ns = {"np": np, "jnp": jnp, "jax": jax, "NUM_CLASSES": C, "UNIFIED_FOCAL_GAMMA": cfg["gamma"], "UNIFIED_FOCAL_DELTA": 0.6,
          "UNIFIED_FOCAL_LAMBDA": cfg["lam"], "CLASS_WEIGHTS": list(cfg["cw"]), "BOUNDARY_WEIGHT": cfg["bd_w"]}
    for name in ("unified_focal_loss", "dice_loss", "compute_tv_loss"):
        exec(compile(mig._function_text(cells, name), f"improved.ipynb:{name}", "exec"), ns)
    ns.update(logits=z.astype(np.float64), labels=labels.astype(np.int64), coords=None, tv_weight=cfg["tv_w"],
              boundary_weights=np.zeros(len(z)) if bw is None else bw.astype(np.float64))
    with np.errstate(invalid="ignore"), __import__("warnings").catch_warnings():
        __import__("warnings").simplefilter("ignore")
        exec(compile(_combining_lines(cells), "improved.ipynb:loss_fn", "exec"), ns)
    return float(ns["loss"]), ns["aux"]


def main():
    out = {"names": np.array([c[0] for c in uc.GOLDEN_CASES])}
    for case in uc.GOLDEN_CASES:
        name = case[0]
        z, labels, bw, cfg = uc.golden_case(case)
        assert cfg["alpha"] == 0.3 and cfg["beta"] == 0.7 and cfg["ufl_w"] == 0.5 and cfg["dice_w"] == 0.5      # what cell 8 hard-codes
        loss, aux = notebook_loss(z, labels, bw, cfg)
        aux = {k: np.asarray(v, np.float64) for k, v in aux.items()}
        if z.shape[1] == 1:
            assert np.isnan(aux["dice_mean_tumor"])
            aux["dice_mean_tumor"] = np.float64(0.0)
        vec = np.concatenate([[float(aux[k]) for k in ref.AUX_KEYS], aux["dice_per_class"]])
        assert np.isfinite(loss) and np.isfinite(vec).all(), name
        out[name + "_logits"], out[name + "_labels"] = z, labels
        if bw is not None:
            out[name + "_bw"] = bw
        out[name + "_cfg"] = np.float64([cfg["gamma"], cfg["lam"], cfg["tv_w"], cfg["bd_w"], *cfg["cw"]])
        out[name + "_loss"], out[name + "_aux"] = np.float64(loss), vec
        l64, a64, _, _ = ref.forward(z, labels, bw, cfg, want_grad=False)
        print(f"{name}: loss {loss:.12f}  restatement - notebook {l64 - loss:+.2e}, aux {np.abs(ref.aux_vector(a64) - vec).max():.2e}")
    np.savez_compressed(HERE / "unified_loss.npz", **out)
    print("unified_loss.npz:", (HERE / "unified_loss.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
