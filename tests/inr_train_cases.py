"""The cases of the INR training tests, built on the CPU; shared by the host, reference and GPU tests.  No GPU.

Exact cases (EXACT, the shape sweep SWEEP, the batch sweep BATCH, FEATURE0): integer ReLU nets (tests/inr_ref.py's
construction) of the raw kind (FEATURE0: the Fourier kind with K = 0, see its section below) with integer inputs and
integer dlogits in -2..2; every case also plants a dead unit (a first-layer bias below anything the inputs can reach).
Every case must keep every sum of |terms| of the step below 2^24 (inr_train_ref.int_step): tests/test_inr_train_ref.py
checks that for each.

End-to-end cases: Fourier nets with Glorot weights and small biases.  The points that bring any hidden pre-activation (fp64)
within 2e-5 x rms of the ReLU kink are removed when the case is built — a condition on the inputs — and at most 5 % may go.

Tolerances (rule of DESIGN.md section 13): ``E2E_TOL[name]`` is 8 x the worst deviation |g32 - g64| / A of the same step
evaluated in fp32 on the CPU (torch) with the batch in five random orders; likewise for loss, aux and dlogits relative to
their largest fp64 magnitude.  Measured by ``python tests/inr_train_cases.py`` on 2026-10-18 (torch CPU; the cases added
with the shape and batch sweep on 2026-10-19, when the script reproduced every earlier figure); never taken from the kernel.
The recorded values are applied as they are.  A tolerance may not exceed 5e-3 (a missing term shows as O(1) x A).
Only where the fp32 evaluation hit the fp64 value exactly (a recorded 0: the one-class cases, whose loss and dlogits are 0
and whose Dice is 1 in any arithmetic) the tolerance is ZERO_MIN = 2^-24, half a unit in the last place of the fp32 result.
"""
import functools

import numpy as np

import inr_ref
import inr_train_ref as tr

ZERO_MIN = 2.0 ** -24
CAP = 5e-3
KINK_MARGIN = 2e-5

# (in, hidden, layers, out, n, accumulate)
EXACT = [
    (1, 32, 2, 1, 1, False),
    (7, 64, 3, 4, 63, False),
    (31, 128, 5, 16, 64, False),
    (103, 256, 8, 4, 65, False),
    (128, 32, 2, 16, 257, False),
    (7, 256, 2, 4, 1000, False),
    (128, 64, 3, 1, 1000, True),
    (31, 128, 3, 4, 257, False),
    (103, 64, 8, 16, 1, False),
    (1, 256, 5, 1, 63, False),
]
EXACT_SEED = 4100


def exact_id(c):
    return "in%d_h%d_L%d_o%d_n%d%s" % (*c[:5], "_acc" if c[5] else "")


def _exact(shape, seed):
    ind, hid, depth, out, n, acc = shape
    rng = np.random.default_rng(seed)
    dims = [ind] + [hid] * (depth - 1) + [out]
    layers = inr_ref.integer_relu_net(rng, dims)
    layers[0]["b"][0] = -(2.0 * np.abs(layers[0]["W"][:, 0]).sum() + 1.0)          # inputs are in -2..2: unit 0 is dead
    x = inr_ref.integer_inputs(rng, n, ind)
    dl = rng.integers(-2, 3, (n, out)).astype(np.float32)
    nw = sum(a * b for a, b in zip(dims[:-1], dims[1:]))
    init_w = rng.integers(-3, 4, nw).astype(np.float32) if acc else None
    init_b = rng.integers(-3, 4, sum(dims[1:])).astype(np.float32) if acc else None
    return dict(layers=layers, x=x, dlogits=dl, init_w=init_w, init_b=init_b, dims=dims, ref=tr.int_step(layers, x, dl))


@functools.lru_cache(maxsize=None)
def exact_case(i):
    """dict(layers, x, dlogits, init_w, init_b (accumulate cases, else None), ref = int_step)."""
    return _exact(EXACT[i], EXACT_SEED + i)


# ---- shape sweep ----------------------------------------------------------------------------------------
SWEEP_N = 321                      # five 64-row blocks + 1 row; two slabs, the second of 65 points = four k tiles + 1 point
SWEEP_INS, SWEEP_DEPTHS, SWEEP_OUTS = (1, 15, 16, 17, 63, 64, 65, 127, 128), (2, 3, 8), (1, 2, 3, 5, 15, 16)


def _sweep_nets():
    """(in, hidden, layers, out, n, accumulate): every (hidden, in), (hidden, layers) and (hidden, out) pair of
    {32,64,128,256} x SWEEP_INS / SWEEP_DEPTHS / SWEEP_OUTS, built like inr_ref._exact_nets; the offsets rotate the pairing
    per width.  in 16 / 17 / 64 / 65: a k extent on a multiple of kTrBK and one above; in 63 / 64: the slab product's
    in + 1 rows on a 64-row block and one past it; out 2 / 3 / 5 / 15: k tails of the masked product, column tails of the
    16-wide tile.  A quarter accumulates into non-zero gradients."""
    nets = []
    for hi, hid in enumerate((32, 64, 128, 256)):
        for ii, ind in enumerate(SWEEP_INS):
            nets.append((ind, hid, SWEEP_DEPTHS[(ii + hi) % 3], SWEEP_OUTS[(ii + 2 * hi) % 6], SWEEP_N, (ii + hi) % 4 == 0))
    return nets


SWEEP = _sweep_nets()
SWEEP_SEED = 4300                  # net i uses SWEEP_SEED + i; SWEEP_RESEED[i] instead where that draw misses a precondition
SWEEP_RESEED = {}                  # none needed: the script below prints bounds of 2^8.9 .. 2^14.5, >= 1445 zero units per net (2026-10-19)


@functools.lru_cache(maxsize=None)
def sweep_case(i):
    return _exact(SWEEP[i], SWEEP_RESEED.get(i, SWEEP_SEED + i))


# ---- batch sweep: two narrow nets on both sides of every doubling of the slab length up to 4096 ----------------------------------
# n      16383      16384     16385          32768     32769           65536      65537                          131073
# slabs  64 x 256   64 x 256  33 x 512 (1)   64 x 512  33 x 1024 (1)   64 x 1024  33 x 2048 (1)                  33 x 4096 (1)
# (k): the last slab holds k points.  loss blocks: 256 is reached at n = 65281; the stride loop starts at n = 65537.
BATCH_NS = (16383, 16384, 16385, 32768, 32769, 65536, 65537, 131073)
BATCH = [(7, 32, 2, 4, n, n == 65537) for n in BATCH_NS] + [(31, 64, 3, 4, n, False) for n in BATCH_NS if n <= 32769]
BATCH_SEED = 4500                  # printed bounds: 2^14.9 (n = 16383) .. 2^17.9 (n = 131073) for 7 -> 32 -> 4, 2^16.3 .. 2^17.3 for the wider net
BATCH_REPEAT = (7, 32, 2, 4, 131073, False)         # this case runs its step twice: the same bytes
GUARD_NS = (16384, 16385, 65537)                    # the raw-ABI cases: net 7 -> 32 -> 4 of BATCH at these n


@functools.lru_cache(maxsize=None)
def batch_case(i):
    return _exact(BATCH[i], BATCH_SEED + i)


def batch_index(ind, n):
    return next(i for i, c in enumerate(BATCH) if c[0] == ind and c[4] == n)


# ---- the feature builder without a sine: FOURIER_RELU with K = 0, x = (coords, modalities) ---------------------------------------
# (M, hidden, layers, out); n = SWEEP_N.  Coordinates in {-1, -0.5, 0, 0.5, 1}, integer modalities and dlogits: every value
# of the step is a multiple of 1/2.  The int64 reference runs on 2 x (x, every bias): ReLU is positively homogeneous, so its
# logits and dW are 2 x the network's and its db (sums of dz, which only see the unchanged signs) is the network's own.
FEATURE0 = [(0, 32, 2, 4), (5, 64, 3, 16), (8, 128, 3, 3)]
FEATURE0_SEED = 4700               # printed bounds of the doubled nets: 2^10.0, 2^11.9, 2^11.8


def feature0_id(c):
    return "m%d_h%d_L%d_o%d" % c


@functools.lru_cache(maxsize=None)
def feature0_case(i):
    """dict(layers, coords, feats or None, dlogits, dims, M, ref = int_step of the doubled net: logits x 2, dW x 2, db x 1)."""
    M, hid, depth, out = FEATURE0[i]
    rng = np.random.default_rng(FEATURE0_SEED + i)
    dims = [3 + M] + [hid] * (depth - 1) + [out]
    layers = inr_ref.integer_relu_net(rng, dims)
    layers[0]["b"][0] = -(2.0 * np.abs(layers[0]["W"][:, 0]).sum() + 1.0)
    coords = rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0], np.float32), (SWEEP_N, 3))
    feats = inr_ref.integer_inputs(rng, SWEEP_N, M) if M else None
    dl = rng.integers(-2, 3, (SWEEP_N, out)).astype(np.float32)
    x = coords if feats is None else np.concatenate([coords, feats], 1)
    doubled = [{"W": p["W"], "b": 2.0 * p["b"]} for p in layers]
    return dict(layers=layers, coords=coords, feats=feats, dlogits=dl, dims=dims, M=M, x=x, ref=tr.int_step(doubled, 2.0 * x, dl))


# name: (K, M, hidden, hidden layers, classes, n)
E2E = {
    "k4_m4_4x64_n1024": (4, 4, 64, 4, 4, 1024),
    "k16_m4_4x256_n2048": (16, 4, 256, 4, 4, 2048),
    "k2_m1_2x32_n777": (2, 1, 32, 2, 4, 777),
    "k1_m0_2x32_n600": (1, 0, 32, 2, 4, 600),            # no modality: feats is None down to mrirt_inr_forward_f32
    "k1_m8_2x32_n600": (1, 8, 32, 2, 4, 600),            # the most modalities the descriptor takes
}
E2E_SEED = {"k16_m4_4x256_n2048": 5200, "k2_m1_2x32_n777": 5201, "k4_m4_4x64_n1024": 5202, "k1_m0_2x32_n600": 5203, "k1_m8_2x32_n600": 5204}
CLASS_WEIGHTS = [0.5, 1.0, 2.0, 1.5]
DICE_WEIGHT = 0.5

# 8 x the worst fp32-CPU deviation over five batch orders (see the module docstring), as `python tests/inr_train_cases.py` prints
E2E_TOL = {
    "k4_m4_4x64_n1024": dict(grads=4.06e-4, loss=2.23e-7, aux=8.12e-7, dlogits=1.41e-6, logits=2.6e-6),      # 4 points removed
    "k16_m4_4x256_n2048": dict(grads=4.12e-3, loss=4.9e-7, aux=8.89e-7, dlogits=1.62e-6, logits=1.23e-5),   # 26 points removed
    "k2_m1_2x32_n777": dict(grads=5.33e-6, loss=4.82e-7, aux=3.87e-7, dlogits=1.08e-6, logits=2.65e-6),     # none removed
    "k1_m0_2x32_n600": dict(grads=2.14e-5, loss=7.98e-7, aux=5.91e-7, dlogits=8.38e-7, logits=1.55e-6),     # none removed (2026-10-19)
    "k1_m8_2x32_n600": dict(grads=2.25e-6, loss=1.46e-7, aux=1.02e-6, dlogits=1.3e-6, logits=1.21e-6),      # none removed (2026-10-19)
}
MSE_TOL = dict(grads=4.06e-4, loss=7.77e-7, dlogits=8.6e-7, logits=2.6e-6)      # mlp_autograd with an MSE loss on the first shape


@functools.lru_cache(maxsize=None)
def e2e_case(name):
    """dict(layers, coords, feats, labels, K, classes, removed, ref = the fp64 step) after the kink filter."""
    K, M, hid, nh, nc, n = E2E[name]
    rng = np.random.default_rng(E2E_SEED[name])
    dims = [3 + 6 * K + M] + [hid] * nh + [nc]
    layers = inr_ref.fourier_params(rng, dims)
    coords = (rng.random((n, 3)) * 2 - 1).astype(np.float32)
    feats = rng.standard_normal((n, M)).astype(np.float32) if M else None
    labels = rng.integers(0, nc, n).astype(np.int32)
    import torch
    x64 = tr.build_input(coords, feats, K, torch.float64).numpy()
    keep = tr.kink_free(layers, x64, KINK_MARGIN)
    removed = int((~keep).sum())
    if removed > 0.05 * n:
        raise ValueError(f"{name}: the kink filter removes {removed} of {n} points (more than 5 %)")
    coords, feats, labels, x64 = coords[keep], None if feats is None else feats[keep], labels[keep], x64[keep]
    ref = tr.step(layers, x64, tr.model_loss(labels, CLASS_WEIGHTS, DICE_WEIGHT, nc))
    return dict(layers=layers, coords=coords, feats=feats, labels=labels, K=K, M=M, classes=nc, dims=dims, removed=removed, n=int(keep.sum()),
                x64=x64, ref=ref)


def mse_target(case):
    rng = np.random.default_rng(77)
    return rng.standard_normal((case["n"], case["classes"])).astype(np.float32)


def mse_loss(target, perm=None):
    import torch

    def f(logits):
        t = torch.as_tensor(target if perm is None else target[np.asarray(perm)], dtype=logits.dtype)
        return ((logits - t) ** 2).mean(), None
    return f


def rel_max(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def fp32_deviation(case, loss_factory, ref, orders=5, seed=9):
    """Worst deviation of the step in fp32 on the CPU from the fp64 ``ref`` over ``orders`` random batch orders."""
    import torch
    rng = np.random.default_rng(seed)
    worst = dict(grads=0.0, loss=0.0, aux=0.0, dlogits=0.0, logits=0.0)
    for _ in range(orders):
        perm = rng.permutation(case["n"])
        x32 = tr.build_input(case["coords"], case["feats"], case["K"], torch.float32).numpy()
        got = tr.step(case["layers"], x32, loss_factory(perm), torch.float32, perm)
        worst["grads"] = max(worst["grads"], tr.deviation(ref, got))
        worst["loss"] = max(worst["loss"], abs(got["loss"] - ref["loss"]) / abs(ref["loss"]))
        worst["logits"] = max(worst["logits"], rel_max(got["logits"], ref["logits"]))
        worst["dlogits"] = max(worst["dlogits"], rel_max(got["dlogits"], ref["dlogits"]))
        if ref["aux"] is not None:
            worst["aux"] = max(worst["aux"], rel_max(got["aux"], ref["aux"]))
    return worst


def e2e_fp32_deviation(name):
    c = e2e_case(name)
    return fp32_deviation(c, lambda perm: tr.model_loss(c["labels"], CLASS_WEIGHTS, DICE_WEIGHT, c["classes"], perm), c["ref"])


def mse_ref(case):
    return tr.step(case["layers"], case["x64"], mse_loss(mse_target(case)))


def tol(recorded):
    """A recorded tolerance (8 x a measured deviation) as it is; ZERO_MIN where the measurement was exactly 0 — a value above
    the cap is an error of the case."""
    t = float(recorded) if recorded > 0 else ZERO_MIN
    if t > CAP:
        raise ValueError(f"tolerance {t:.3g} exceeds the cap {CAP}")
    return t


# ---- loss alone ------------------------------------------------------------------------------------------------------------------
# (n, classes, dice weight, largest |logit|); class C-1 never occurs among the labels of the cases with 4 or more classes
LOSS = [(1, 1, 0.0, 3.0), (1, 4, 0.5, 3.0), (5, 4, 1.0, 80.0), (5, 16, 0.0, 3.0), (1000, 1, 0.5, 3.0), (1000, 4, 0.5, 80.0),
        (1000, 16, 1.0, 80.0), (1000, 4, 0.0, 3.0), (5, 1, 1.0, 80.0),
        # beyond the cap of 256 loss blocks: the points from 65536 on (a third) are reached by the grid-stride loop only.
        # Logits within +-3 for both: at +-80 the fp32 CPU loss of the 16-class case lands within 4e-10 of the fp64 value by
        # chance, 8 x which is no tolerance an fp32 result can be held to (half a unit in its last place is 6e-8).
        (100003, 4, 0.5, 3.0), (100003, 16, 0.5, 3.0)]
# 8 x the fp32-CPU deviation of loss_alone (a single order: nothing here depends on the batch order but three sums)
LOSS_TOL = [dict(loss=0.0, aux=0.0, dlogits=0.0), dict(loss=1.96e-7, aux=3.1e-7, dlogits=2.37e-7), dict(loss=6.4e-7, aux=4.51e-7, dlogits=1.15e-6),
            dict(loss=1.64e-7, aux=6e-7, dlogits=3.17e-7), dict(loss=0.0, aux=0.0, dlogits=0.0), dict(loss=3.29e-7, aux=2.22e-7, dlogits=1.47e-6),
            dict(loss=1.12e-7, aux=8.63e-7, dlogits=4.62e-6), dict(loss=2.16e-7, aux=4.6e-7, dlogits=1.6e-6), dict(loss=0.0, aux=0.0, dlogits=0.0),
            dict(loss=4.01e-7, aux=1.08e-6, dlogits=1.8e-6), dict(loss=5.71e-7, aux=8.93e-7, dlogits=1.13e-6)]      # the two of 2026-10-19


LOSS_FIRST_STRIDED = 256 * 256      # kLossMaxBlocks x kLossThreads: the first point the partial sums reach by striding


def loss_id(c):
    return "n%d_c%d_dw%g_z%g" % c


@functools.lru_cache(maxsize=None)
def loss_case(i):
    n, nc, dw, zmax = LOSS[i]
    rng = np.random.default_rng(6300 + i)
    logits = (rng.uniform(-1, 1, (n, nc)) * zmax).astype(np.float32)
    labels = rng.integers(0, max(nc - 1, 1) if nc >= 4 else nc, n).astype(np.int32)
    cw = (0.5 + rng.random(nc) * 2).astype(np.float32)
    return dict(logits=logits, labels=labels, cw=cw, dw=dw, classes=nc, ref=tr.loss_alone(logits, labels, cw, dw))


def loss_fp32_deviation(i):
    import torch
    c = loss_case(i)
    got = tr.loss_alone(c["logits"], c["labels"], c["cw"], c["dw"], torch.float32)
    return dict(loss=abs(got["loss"] - c["ref"]["loss"]) / max(abs(c["ref"]["loss"]), 1e-300), aux=rel_max(got["aux"], c["ref"]["aux"]),
                dlogits=rel_max(got["dlogits"], c["ref"]["dlogits"]))


if __name__ == "__main__":                               # the measurement behind E2E_TOL, MSE_TOL and LOSS_TOL
    for what, lst, case in (("exact", EXACT, exact_case), ("sweep", SWEEP, sweep_case), ("batch", BATCH, batch_case)):
        for i, c in enumerate(lst):
            r = case(i)["ref"]
            print(what, exact_id(c), "bound 2^%.1f" % np.log2(max(r["bound"], 1)), "zero", r["zero_units"], "dead", r["dead_units"])
    for i, c in enumerate(FEATURE0):
        r = feature0_case(i)["ref"]
        print("feature0", feature0_id(c), "bound (doubled net) 2^%.1f" % np.log2(max(r["bound"], 1)), "zero", r["zero_units"], "dead", r["dead_units"])
    for name in E2E:
        c = e2e_case(name)
        d = e2e_fp32_deviation(name)
        print(name, "removed", c["removed"], "of", E2E[name][5], {k: "%.3g" % (8 * v) for k, v in d.items()})
    c = e2e_case("k4_m4_4x64_n1024")
    d = fp32_deviation(c, lambda perm: mse_loss(mse_target(c), perm), mse_ref(c))
    print("mse", {k: "%.3g" % (8 * v) for k, v in d.items()})
    for i, c in enumerate(LOSS):
        print(loss_id(c), {k: "%.3g" % (8 * v) for k, v in loss_fp32_deviation(i).items()})
