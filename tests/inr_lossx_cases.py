"""The cases of the extended-loss and tumour-sampler tests, built on the CPU; shared by the host, reference and GPU tests.  No GPU.

Loss cases (LOSS): random logits within +-zmax, labels by ``mode``, per-class weights and focal alphas from the case's seed.
Each option of scripts/jax_inr_brats.py's loss alone and all together; n on both sides of a 256-point block and past the
256 x 256 points the partial sums reach without striding (tc.LOSS_FIRST_STRIDED); C in {1, 3, 4, 16}; gamma in {1, 2, 5};
smoothing 0 and 0.05; alpha on and off; both Dice forms; a class that never occurs under the prevalence-weighted form; a batch
without edema (TP = FN = 0) and one of edema only (FP = 0); labels outside the range.

Tolerances (rule of DESIGN.md section 13, as inr_train_cases.py applies it): ``LOSS_TOL[name]`` is 8 x the worst deviation of
the same formula (inr_lossx_ref.loss_terms) evaluated in fp32 on the CPU (torch) with the batch in five random orders, from
its fp64 value: loss relative to |loss|; aux, terms and dlogits relative to their largest fp64 magnitude.  Measured by
``python tests/inr_lossx_cases.py`` on 2026-10-19 (torch CPU); never taken from the kernel; applied as recorded.  A tolerance
may not exceed 5e-3; where the measurement was exactly 0 it is ZERO_MIN = 2^-24 (tc.tol).  STEP_TOL likewise for the whole
step (forward, extended loss, backward) on one ReLU and one SIREN network.
"""
import functools

import numpy as np

import inr_lossx_ref as lx
import inr_siren_cases as sc
import inr_siren_ref as sr
import inr_train_cases as tc

ALL = dict(focal_gamma=2.0, alpha=True, label_smoothing=0.05, dice_weight=0.5, per_class_dice=False, edema_fp_weight=0.3,
           tversky_weight=0.4, tversky_alpha=0.7, tversky_beta=0.3, edema_logit_reg=0.2)
BIG = 65836                        # 300 points past tc.LOSS_FIRST_STRIDED

# name: (n, classes, largest |logit|, label mode, options; "alpha": True draws focal_alpha from the seed)
LOSS = {
    "focal_g2_n255_c4": (255, 4, 4.0, "all", dict(focal_gamma=2.0)),
    "focal_g1_alpha_n257_c4": (257, 4, 4.0, "all", dict(focal_gamma=1.0, alpha=True)),
    "focal_g5_dice_n257_c16": (257, 16, 4.0, "all", dict(focal_gamma=5.0, dice_weight=0.5)),
    "smooth_n255_c3": (255, 3, 4.0, "all", dict(label_smoothing=0.05, dice_weight=0.5)),
    "dice_prev_absent_n257_c4": (257, 4, 4.0, "absent_last", dict(dice_weight=0.5, per_class_dice=False)),
    "dice_prev_smooth_n255_c16": (255, 16, 4.0, "absent_last", dict(dice_weight=1.0, per_class_dice=False, label_smoothing=0.05)),
    "edema_fp_n255_c4": (255, 4, 4.0, "all", dict(edema_fp_weight=0.3)),
    "tversky_n257_c4": (257, 4, 4.0, "all", dict(tversky_weight=0.4)),
    "logit_reg_n255_c3": (255, 3, 30.0, "all", dict(edema_logit_reg=0.2)),
    "all_n257_c4": (257, 4, 4.0, "all", ALL),
    "all_no_edema_n255_c4": (255, 4, 4.0, "no_edema", ALL),
    "all_edema_only_n255_c4": (255, 4, 4.0, "edema_only", ALL),
    "all_outside_n257_c4": (257, 4, 4.0, "outside", ALL),
    "all_n1_c4": (1, 4, 4.0, "all", ALL),
    "focal_smooth_dice_n1_c1": (1, 1, 4.0, "all", dict(focal_gamma=2.0, label_smoothing=0.05, dice_weight=0.5)),
    "focal_smooth_alpha_n255_c1": (255, 1, 4.0, "all", dict(focal_gamma=1.0, alpha=True, label_smoothing=0.05, dice_weight=0.5)),
    "all_big_c4": (BIG, 4, 4.0, "all", ALL),
    "focal_alpha_prev_big_c16": (BIG, 16, 30.0, "absent_last", dict(focal_gamma=2.0, alpha=True, dice_weight=0.5, per_class_dice=False,
                                                                      edema_fp_weight=0.3, tversky_weight=0.4, edema_logit_reg=0.2)),
}
LOSS_SEED = 9300                   # case i (in the order above) uses LOSS_SEED + i + LOSS_RESEED.get(name, 0)
# With its first seed the fp32 CPU loss of the Tversky case landed within 4.4e-9 of the fp64 value by chance (8 x = 3.5e-8):
# no tolerance an fp32 result can be held to, whose own rounding is up to 2^-24 = 6e-8.  A criterion on the CPU figures alone.
# (One class with the prevalence-weighted Dice is left out for a like reason: its fp64 loss is ~1e-9, fp32 gives 0.)
LOSS_RESEED = {"tversky_n257_c4": 100}

# 8 x the worst fp32-CPU deviation over five batch orders, as `python tests/inr_lossx_cases.py` prints (2026-10-19)
LOSS_TOL = {
    "focal_g2_n255_c4": dict(loss=2.22e-06, aux=1.07e-06, terms=2.22e-06, dlogits=2.67e-06),
    "focal_g1_alpha_n257_c4": dict(loss=1.81e-06, aux=6.42e-07, terms=1.81e-06, dlogits=1.8e-06),
    "focal_g5_dice_n257_c16": dict(loss=1.18e-06, aux=9.98e-07, terms=1.02e-06, dlogits=2.5e-06),
    "smooth_n255_c3": dict(loss=8.79e-07, aux=4.74e-07, terms=4.5e-07, dlogits=1.21e-06),
    "dice_prev_absent_n257_c4": dict(loss=6.88e-07, aux=7.01e-07, terms=5.68e-07, dlogits=1.11e-06),
    "dice_prev_smooth_n255_c16": dict(loss=9.89e-08, aux=8.06e-07, terms=6.83e-07, dlogits=2.1e-06),
    "edema_fp_n255_c4": dict(loss=7.55e-07, aux=1.22e-06, terms=9.87e-07, dlogits=7.88e-07),
    "tversky_n257_c4": dict(loss=1.43e-07, aux=1.32e-06, terms=1.69e-07, dlogits=1.05e-06),
    "logit_reg_n255_c3": dict(loss=8.76e-07, aux=4.44e-07, terms=1.02e-06, dlogits=9.96e-07),
    "all_n257_c4": dict(loss=1.02e-06, aux=8.03e-07, terms=1.53e-06, dlogits=1.86e-06),
    "all_no_edema_n255_c4": dict(loss=8.39e-07, aux=9.75e-07, terms=1.49e-06, dlogits=3.2e-06),
    "all_edema_only_n255_c4": dict(loss=1.67e-06, aux=7.36e-07, terms=1.84e-06, dlogits=3.22e-06),
    "all_outside_n257_c4": dict(loss=1.57e-06, aux=1.19e-06, terms=1.17e-06, dlogits=1.98e-06),
    "all_n1_c4": dict(loss=1.7e-06, aux=6.19e-07, terms=1.16e-06, dlogits=2.49e-06),
    "focal_smooth_dice_n1_c1": dict(loss=0, aux=0, terms=0, dlogits=0),
    "focal_smooth_alpha_n255_c1": dict(loss=0, aux=0, terms=0, dlogits=0),
    "all_big_c4": dict(loss=1.14e-06, aux=1.27e-06, terms=1.85e-06, dlogits=3.11e-06),
    "focal_alpha_prev_big_c16": dict(loss=3.37e-07, aux=9.23e-07, terms=5.65e-07, dlogits=4.14e-06),
}
STEP_TOL = {
    "relu": dict(grads=5.17e-06, loss=1.1e-07, aux=8.57e-07, dlogits=2.78e-06, logits=2.65e-06),
    "siren": dict(grads=1.99e-06, loss=8.2e-07, aux=8.11e-07, dlogits=1.75e-06, logits=2.01e-06),
}

STEP_OPT = ALL
STEP_RELU, STEP_SIREN_DIMS, STEP_SIREN_N, STEP_SIREN_SEED = "k2_m1_2x32_n777", [7, 32, 32, 4], 600, 9500


def _labels(rng, mode, n, nc):
    if mode == "all":
        return rng.integers(0, nc, n).astype(np.int32)
    if mode == "absent_last":
        return rng.integers(0, max(nc - 1, 1), n).astype(np.int32)
    if mode == "no_edema":
        return rng.choice(np.array([k for k in range(nc) if k != 2], np.int32), n)
    if mode == "edema_only":
        return np.full(n, 2, np.int32)
    if mode == "outside":
        lab = rng.integers(0, nc, n).astype(np.int32)
        lab[::7] = -1
        lab[3::11] = nc
        lab[5::13] = 2 ** 31 - 1
        return lab
    raise KeyError(mode)


def options_of(spec, rng, nc):
    spec = dict(spec)
    alpha = (0.25 + rng.random(nc) * 1.75).astype(np.float32) if spec.pop("alpha", False) else None
    return lx.options(focal_alpha=alpha, **spec)


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """dict(logits, labels, cw, opt, classes, n, ref = the fp64 loss_alone)."""
    n, nc, zmax, mode, spec = LOSS[name]
    rng = np.random.default_rng(LOSS_SEED + list(LOSS).index(name) + LOSS_RESEED.get(name, 0))
    logits = (rng.uniform(-1, 1, (n, nc)) * zmax).astype(np.float32)
    labels = _labels(rng, mode, n, nc)
    cw = (0.5 + rng.random(nc) * 2).astype(np.float32)
    opt = options_of(spec, rng, nc)
    return dict(logits=logits, labels=labels, cw=cw, opt=opt, classes=nc, n=n, ref=lx.loss_alone(logits, labels, cw, opt))


def loss_fp32_deviation(name, orders=5, seed=9):
    import torch
    c = loss_case(name)
    ref = c["ref"]
    rng = np.random.default_rng(seed)
    worst = dict(loss=0.0, aux=0.0, terms=0.0, dlogits=0.0)
    for _ in range(orders):
        got = lx.loss_alone(c["logits"], c["labels"], c["cw"], c["opt"], torch.float32, rng.permutation(c["n"]))
        worst["loss"] = max(worst["loss"], abs(got["loss"] - ref["loss"]) / max(abs(ref["loss"]), 1e-300))
        for k in ("aux", "terms", "dlogits"):
            worst[k] = max(worst[k], tc.rel_max(got[k], ref[k]))
    return worst


def tol(recorded):
    return tc.tol(recorded)


# ---- the whole step with the extended loss ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_opt(nc=4):
    return options_of(STEP_OPT, np.random.default_rng(9400), nc)


@functools.lru_cache(maxsize=None)
def relu_step_case():
    """tc.e2e_case(STEP_RELU) with ref = the fp64 step under the extended loss."""
    c = dict(tc.e2e_case(STEP_RELU))
    c["ref"] = tc.tr.step(c["layers"], c["x64"], lx.ext_loss(c["labels"], tc.CLASS_WEIGHTS, step_opt()))
    return c


def relu_step_fp32_deviation():
    c = relu_step_case()
    return tc.fp32_deviation(c, lambda perm: lx.ext_loss(c["labels"], tc.CLASS_WEIGHTS, step_opt(), perm), c["ref"])


@functools.lru_cache(maxsize=None)
def siren_step_case():
    """A 7 -> 2 x 32 -> 4 SIREN at n = 600, built like sc.e2e_case, with ref = the fp64 step under the extended loss."""
    rng = np.random.default_rng(STEP_SIREN_SEED)
    dims, n = STEP_SIREN_DIMS, STEP_SIREN_N
    layers = sr.siren_layers(rng, dims, sc.W0)
    coords = (rng.random((n, 3)) * 2 - 1).astype(np.float32)
    feats = rng.standard_normal((n, dims[0] - 3)).astype(np.float32)
    x = sr.input_matrix(coords, feats)
    labels = rng.integers(0, dims[-1], n).astype(np.int32)
    cw = (0.5 + rng.random(dims[-1]) * 1.5).astype(np.float32)
    ref = sr.step(layers, x.astype(np.float64), sc.W0, lx.ext_loss(labels, cw, step_opt()))
    return dict(layers=layers, dims=dims, coords=coords, feats=feats, x=x, labels=labels, cw=cw, classes=dims[-1], n=n, ref=ref)


def siren_step_fp32_deviation(orders=5, seed=9):
    import torch
    c = siren_step_case()
    ref = c["ref"]
    rng = np.random.default_rng(seed)
    worst = dict(grads=0.0, loss=0.0, aux=0.0, dlogits=0.0, logits=0.0)
    for _ in range(orders):
        perm = rng.permutation(c["n"])
        got = sr.step(c["layers"], c["x"], sc.W0, lx.ext_loss(c["labels"], c["cw"], step_opt(), perm), torch.float32, perm)
        worst["grads"] = max(worst["grads"], tc.tr.deviation(ref, got))
        worst["loss"] = max(worst["loss"], abs(got["loss"] - ref["loss"]) / abs(ref["loss"]))
        for k in ("logits", "dlogits", "aux"):
            worst[k] = max(worst[k], tc.rel_max(got[k], ref[k]))
    return worst


# ---- tumour index and mixed sampler -------------------------------------------------------------------------------------------------
# volumes whose size is no multiple of the 4096-voxel chunk; case 0 empty, case 1 full, case 2 with the last voxel only, case 3 random
MIX_SHAPES = [(5, 7, 9), (17, 16, 17), (67, 66, 65)]          # 315, 4624 and 287 430 voxels
MIX_MODS = 2
MIX_NS = (1, 255, 1000)
MIX_SEED = 0xC0FFEE0000004D


@functools.lru_cache(maxsize=None)
def mix_cases(shape_index):
    hwd = MIX_SHAPES[shape_index]
    rng = np.random.default_rng(9600 + shape_index)
    segs = [np.zeros(hwd, np.int16), rng.integers(1, 4, hwd).astype(np.int16), np.zeros(hwd, np.int16),
            np.where(rng.random(hwd) < 0.1, rng.integers(1, 4, hwd), 0).astype(np.int16)]
    segs[2][-1, -1, -1] = 3
    segs[3][0, 0, 0] = -2                                 # a negative label is no tumour voxel
    return [{"mods": rng.standard_normal((MIX_MODS, *hwd)).astype(np.float32), "seg": s} for s in segs]


def mix_n_tumours(n):
    return sorted({0, 1, n // 2, n} & set(range(n + 1)))


if __name__ == "__main__":                               # the measurement behind LOSS_TOL and STEP_TOL
    for name in LOSS:
        print('    "%s": dict(%s),' % (name, ", ".join("%s=%.3g" % (k, 8 * v) for k, v in loss_fp32_deviation(name).items())))
    for name, d in (("relu", relu_step_fp32_deviation()), ("siren", siren_step_fp32_deviation())):
        print('    "%s": dict(%s),' % (name, ", ".join("%s=%.3g" % (k, 8 * v) for k, v in d.items())))
