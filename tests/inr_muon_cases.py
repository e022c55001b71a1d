"""The cases of the Muon tests, built on the CPU; shared by the reference, host and GPU tests.  No GPU.

Exact cases (EXACT): whole networks whose every weight matrix is a scaled selection matrix — at most one non-zero per row and
per column, each +-2^e with two or three different e per matrix (distinct singular values).  Every sum of every Newton-Schulz
product then has at most one non-zero term, so the fp32 MFMA result must EQUAL the fp32 NumPy restatement;
test_inr_muon_ref.py proves that precondition (and that no intermediate is denormal or overflows) from the restatement's own
trace.  The shapes pair every hidden width with in in {1, 7, 17, 65, 128}, out in {1, 4, 16} and 2 / 3 / 8 layers: in < out,
in > out (the transposed path), in = out, and both sides of the 64-wide tile edges.

Tolerances (rule of DESIGN.md sections 13 / 14): 8 x the worst deviation of the fp32 CPU restatement from the fp64 one,
relative to the largest fp64 magnitude of that matrix.  Measured by ``python tests/inr_muon_cases.py`` on the CPU (NumPy) on
2026-10-19 and recorded below; never taken from the kernel.  The same script prints the factor by which the fp64 CPU Muon loop
lowers the loss of the two end-to-end cases (E2E_FALL: the GPU run must fall by at least that / 1.5).
"""
import functools

import numpy as np

import inr_loop_cases as lc
import inr_muon_ref as mr
import inr_siren_cases as sc

# ---- orthogonalize, exact -------------------------------------------------------------------------------------------------------
# dims, seed; "zero": index of a layer that is all zero; "holes": layers with all-zero rows (fewer entries than min(in, out))
EXACT = [
    dict(dims=[1, 32, 1], seed=1),
    dict(dims=[7, 64, 64, 4], seed=2, holes=(0, 1)),
    dict(dims=[17, 128, 128, 16], seed=3, zero=1),
    dict(dims=[65, 256, 256, 1], seed=4, holes=(1,)),
    dict(dims=[128, 32, 32, 16], seed=5),
    dict(dims=[128, 256, 4], seed=6),
    dict(dims=[65, 64] + [64] * 6 + [16], seed=7, holes=(3,), zero=5),        # 8 layers
    dict(dims=[17, 32, 4], seed=8),
]
EXACT_NS_STEPS = (1, 5)
GUARD_CASE = 3                      # this case also runs on a scratch of exactly the stated size between two guard blocks
NAN_CASE, NAN_LAYER = 1, 1
EXPONENTS = (0, -1, -3)


def exact_id(c):
    return "x".join(str(d) for d in c["dims"])


@functools.lru_cache(maxsize=None)
def exact_case(i):
    """The flat fp32 matrices of EXACT[i]."""
    c = EXACT[i]
    rng = np.random.default_rng(8800 + c["seed"])
    mats = []
    for l, (a, b) in enumerate(zip(c["dims"][:-1], c["dims"][1:])):
        M = np.zeros((a, b), np.float32)
        r = min(a, b)
        k = 0 if l == c.get("zero") else (max(1, r // 2) if l in c.get("holes", ()) else r)
        rows, cols = rng.permutation(a)[:k], rng.permutation(b)[:k]
        exps = rng.choice(EXPONENTS[:2 if k < 3 else 3], k)
        if k >= 2:
            exps[:2] = EXPONENTS[:2]                     # at least two different magnitudes
        M[rows, cols] = rng.choice([-1.0, 1.0], k) * np.exp2(exps)
        mats.append(M)
    return np.concatenate([M.reshape(-1) for M in mats])


# ---- orthogonalize and step, tolerance ------------------------------------------------------------------------------------------
TOL_NETS = {"7x256x256x256x4": [7, 256, 256, 256, 4], "103x64x64x4": [103, 64, 64, 4], "65x32x32x32x16": [65, 32, 32, 32, 16]}
TOL_SCALES = (1e-6, 1.0, 1e3)
# 8 x these is the bound: worst |fp32 CPU - fp64| / max |fp64| over the net's layers and the three scales (2026-10-19, NumPy)
NS_DEVIATION = {"7x256x256x256x4": 4.15e-06, "103x64x64x4": 2.65e-06, "65x32x32x32x16": 2.08e-06}
# the whole step (W and mu_w per layer) on STEP_NET, the same rule
STEP_NET = [17, 64, 64, 4]
STEP_DEVIATION = dict(w=4.06e-08, mu_w=6.93e-08)


@functools.lru_cache(maxsize=None)
def tol_case(name, scale):
    dims = TOL_NETS[name]
    rng = np.random.default_rng(8900 + sorted(TOL_NETS).index(name))
    nw = sum(a * b for a, b in zip(dims[:-1], dims[1:]))
    return (rng.standard_normal(nw) * scale).astype(np.float32)


def layer_deviation(got, want64, dims):
    """Per layer: worst |got - want| / max |want|."""
    return [float(np.abs(np.asarray(g, np.float64) - w).max() / max(np.abs(w).max(), 1e-300))
            for g, w in zip(mr.split(np.asarray(got).reshape(-1), dims), mr.split(np.asarray(want64).reshape(-1), dims))]


@functools.lru_cache(maxsize=None)
def step_case(seed=0):
    """Weights, biases, first moments (second moment of the biases >= 0) and float gradients of STEP_NET."""
    dims = STEP_NET
    rng = np.random.default_rng(9100 + seed)
    nw, nb = sum(a * b for a, b in zip(dims[:-1], dims[1:])), sum(dims[1:])
    f = lambda n, s: (rng.standard_normal(n) * s).astype(np.float32)
    return dict(dims=dims, w=f(nw, 0.2), b=f(nb, 0.05), gw=f(nw, 0.3), gb=f(nb, 0.3), mu_w=f(nw, 0.1), mu_b=f(nb, 0.1),
                nu_b=(rng.random(nb) * 0.01).astype(np.float32))


# Nesterov on / off, clipping active / inactive (as a multiple of the raw norm; 0 = off), t, weight decay
STEP_VARIANTS = [
    dict(nesterov=True, clip=0.5, t=0, wd=0.0),
    dict(nesterov=False, clip=4.0, t=0, wd=0.0),
    dict(nesterov=True, clip=0.0, t=999, wd=0.01),
    dict(nesterov=False, clip=0.5, t=12345678, wd=0.01),
]
STEP_LR, STEP_GSCALE = 2e-4, 0.5


# ---- run and end to end ----------------------------------------------------------------------------------------------------------
# train_inr / train_siren with OPTIMIZER_CHOICE = "muon" on inr_loop_cases' two 16^3 cases
E2E_RELU = dict(lc.E2E_CONFIG, OPTIMIZER_CHOICE="muon", LR=1e-2, MIN_LR=1e-3)
E2E_SIREN = dict(sc.E2E_CONFIG, OPTIMIZER_CHOICE="muon", LR=3e-3, MIN_LR=3e-4)
# first-5 / last-5 mean loss of the fp64 CPU Muon loop on the same batches (2026-10-19); the GPU run must fall by that / 1.5
E2E_FALL = dict(relu=1.502, siren=1.642)
E2E_FALL_MEANS = dict(relu=(0.9031, 0.6011), siren=(0.8690, 0.5291))


def e2e_loop_case(family):
    c = E2E_RELU if family == "relu" else E2E_SIREN
    base = lc.e2e_case() if family == "relu" else sc.e2e_loop_case()
    cfg = dict(base["cfg"], peak=c["LR"], end=c["MIN_LR"])
    return dict(layers=base["layers"], cases=base["cases"], cfg=cfg, steps=c["TRAIN_STEPS"])


def measure_ns():
    out = {}
    for name, dims in TOL_NETS.items():
        worst = 0.0
        for scale in TOL_SCALES:
            m = tol_case(name, scale)
            dev = layer_deviation(mr.ns_flat(m, dims, None, np.float32), mr.ns_flat(m, dims, None, np.float64), dims)
            worst = max(worst, max(dev))
        out[name] = worst
    return out


def step_reference(variant, dtype):
    c = step_case()
    import inr_loop_ref as lr_ref
    norm = lr_ref.gnorm(c["gw"], c["gb"], STEP_GSCALE)
    clip = float(np.float32(variant["clip"] * norm))
    s = lr_ref.clip_factor(norm, clip, dtype)
    h = mr.hp(nesterov=variant["nesterov"], weight_decay=variant["wd"])
    return mr.step(c["w"], c["b"], c["gw"], c["gb"], c["mu_w"], c["mu_b"], c["nu_b"], c["dims"], s, STEP_LR, variant["t"], STEP_GSCALE, h, dtype), clip


def measure_step():
    worst = dict(w=0.0, mu_w=0.0)
    for v in STEP_VARIANTS:
        r32, r64 = step_reference(v, np.float32)[0], step_reference(v, np.float64)[0]
        for key in worst:
            worst[key] = max(worst[key], max(layer_deviation(r32[key], r64[key], STEP_NET)))
    return worst


if __name__ == "__main__":                               # the measurements recorded above
    import pathlib
    import sys
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
    print("NS_DEVIATION =", {k: float("%.3g" % v) for k, v in measure_ns().items()})
    print("STEP_DEVIATION =", {k: float("%.3g" % v) for k, v in measure_step().items()})
    for family in ("relu", "siren"):
        e = e2e_loop_case(family)
        per_step = mr.train(e["layers"], e["cases"], e["cfg"], e["steps"], "float64")["losses"].mean(1)
        print("%s: fp64 Muon loop, mean of the first 5 losses %.4f, of the last 5 %.4f, factor %.3f" %
              (family, per_step[:5].mean(), per_step[-5:].mean(), per_step[:5].mean() / per_step[-5:].mean()))
