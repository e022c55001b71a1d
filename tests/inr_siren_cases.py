"""The cases of the SIREN training tests, built on the CPU; shared by the host, reference and GPU tests.  No GPU.

Exact cases (EXACT): selection nets (inr_siren_ref.selection_net) at n = 321.  Every dot product of the step has one non-zero
term, so the fp32 NumPy restatement (inr_siren_ref.np_step) is what a k-ordered fma chain gives, bit for bit;
tests/test_inr_siren_ref.py proves the single term, the absence of denormal sines and the domain for each case.  dlogits is
non-zero in one row p* (the block and slab edges of n = 321); a quarter of the cases accumulate into non-zero gradients.

Further exact tiers, all selection nets against the same restatement: HEAD_COVER (n = 65; per width the heads lie over every
hidden unit once), BEYOND_NET (rows beyond the sine's domain and at +-3e38, p* on one of them; the same net with a NaN and an
inf input, forward only) and BATCH (inr_train_cases.BATCH_NS = 16383 .. 131073 points; dlogits non-zero in one row PER SLAB, so
the fixed-order sum over the slabs adds up to 64 non-zero partials: the reference is inr_siren_ref.np_step_slabs).

Tolerance cases (E2E): random siren_init nets.  ``E2E_TOL[name]`` is 8 x the worst deviation of the same step evaluated in fp32
on the CPU (torch, the restated sine) from the fp64 step over five batch orders — |g32 - g64| / A for the gradients, relative
to the largest fp64 magnitude for logits, loss, aux and dlogits (rule of DESIGN.md sections 13 / 14).  No point is removed: the
sine has no kink.  Measured by ``python tests/inr_siren_cases.py`` on 2026-10-19 (torch CPU); never taken from the kernel.

Loop: RUN (mrirt_siren_train_run against the separate calls) and the train_siren run, with the fall of the fp64 CPU loop on
the same batches (E2E_FALL, measured by the same script).
"""
import functools

import numpy as np

import inr_loop_cases as lc
import inr_siren_ref as sr
import inr_train_cases as tc

KIND_SIREN, KIND_RAW_SIREN = 1, 3
N = 321                            # five 64-row blocks + 1 row; two slabs, the second of 65 points
P_STARS = (0, 63, 64, 255, 256, 320)
HIDDENS, INS, DEPTHS, OUTS = (32, 64, 128, 256), (1, 7, 17, 65, 128), (2, 3, 8), (1, 4, 16)
EXACT_SEED = 8100


def _exact_nets():
    """dicts(ind, hidden, layers, out, kind, w0, pstar, acc, span, shift): every (hidden, in) and (hidden, depth) pair, the
    other values rotating; the in = 7 nets but the last are the coords + modalities kind (it needs in = 3 + M), every other net
    is the raw kind; w0
    alternates between 1 and 30; net 3 takes inputs spanning +-2^20 (w0 = 1)."""
    shapes = []
    for hi, hid in enumerate(HIDDENS):
        for ii, ind in enumerate(INS):
            shapes.append((ind, hid, DEPTHS[(ii + hi) % 3], OUTS[(ii + 2 * hi) % 3]))
        for di, depth in enumerate(DEPTHS):
            shapes.append((INS[(di + hi + 1) % 5], hid, depth, OUTS[(di + hi) % 3]))
    nets, used = [], {}
    for i, (ind, hid, depth, out) in enumerate(shapes):
        span = i == 3
        shift = used.get(hid, 0) % hid                    # the heads of one width select consecutive runs of hidden units
        used[hid] = used.get(hid, 0) + out
        nets.append(dict(ind=ind, hidden=hid, layers=depth, out=out, kind=KIND_SIREN if ind == 7 and i % 4 == 1 else KIND_RAW_SIREN,
                         w0=1.0 if span or i % 2 else 30.0, pstar=P_STARS[i % 6], acc=i % 4 == 0, span=span, shift=shift))
    return nets


EXACT = _exact_nets()
GUARD_CASE = 6                     # this case also runs on a scratch of exactly the stated size between two guard blocks


def exact_id(c):
    return "%s_in%d_h%d_L%d_o%d_w%g_p%d%s%s" % ("siren" if c["kind"] == KIND_SIREN else "raw", c["ind"], c["hidden"], c["layers"], c["out"],
                                               c["w0"], c["pstar"], "_acc" if c["acc"] else "", "_span" if c["span"] else "")


def _selection_case(c, seed, n, make_x=None):
    """A selection net of the dict ``c`` (ind, hidden, layers, out, kind, w0, pstar, acc, span, shift) on n points."""
    rng = np.random.default_rng(seed)
    dims = [c["ind"]] + [c["hidden"]] * (c["layers"] - 1) + [c["out"]]
    layers = sr.selection_net(rng, dims, c["shift"])
    lim = 2.0 ** 20 - 16.0 if c["span"] else 2.0
    x = rng.uniform(-lim, lim, (n, c["ind"])).astype(np.float32) if make_x is None else make_x(rng)
    dl = np.zeros((n, c["out"]), np.float32)
    dl[c["pstar"]] = rng.standard_normal(c["out"]).astype(np.float32) + np.float32(3.0)          # no zero among them
    nw, nb = sum(a * b for a, b in zip(dims[:-1], dims[1:])), sum(dims[1:])
    init_w = rng.standard_normal(nw).astype(np.float32) if c["acc"] else None
    init_b = rng.standard_normal(nb).astype(np.float32) if c["acc"] else None
    raw = c["kind"] == KIND_RAW_SIREN
    return dict(net=c, layers=layers, dims=dims, x=x, coords=None if raw else np.ascontiguousarray(x[:, :3]),
                feats=x if raw else np.ascontiguousarray(x[:, 3:]), dlogits=dl, init_w=init_w, init_b=init_b,
                ref=sr.np_step(layers, x, c["w0"], dl, init_w, init_b))


@functools.lru_cache(maxsize=None)
def exact_case(i):
    """dict(net, layers, dims, x, coords, feats (as the kind takes them), dlogits, init_w, init_b, ref = np_step)."""
    return _selection_case(EXACT[i], EXACT_SEED + i, N)


# ---- every hidden unit under a head: per width, out = 16 and the head's shift in steps of 16 -------------------------------------
HEAD_N = 65                        # one 64-row block + 1 row, one slab
HEAD_SEED = 8200


def _head_cover_nets():
    nets = []
    for hid in HIDDENS:
        for shift in range(0, hid, 16):
            i = len(nets)
            nets.append(dict(ind=17, hidden=hid, layers=3, out=16, kind=KIND_RAW_SIREN, w0=1.0 if i % 2 == 0 else 30.0, pstar=(0, 63, 64)[i % 3],
                             acc=False, span=False, shift=shift))
    return nets


HEAD_COVER = _head_cover_nets()


@functools.lru_cache(maxsize=None)
def head_cover_case(i):
    return _selection_case(HEAD_COVER[i], HEAD_SEED + i, HEAD_N)


# ---- beyond the sine's domain: a third of the rows inside +-2^20, a third in +-(2^20, 2^24], a third at +-3e38 ---------------------
BEYOND_NET = dict(ind=17, hidden=64, layers=3, out=4, kind=KIND_RAW_SIREN, w0=1.0, pstar=256, acc=False, span=False, shift=0)
BEYOND_SEED = 8300
BEYOND_NAN_AT, BEYOND_INF_AT = (10, 3), (200, 5)         # (row, input) of the NaN and of the +inf of the forward-only case


def beyond_class(n=N):
    """Row p's class: 0 inside the domain, 1 beyond it within +-(2^20, 2^24], 2 at +-3e38."""
    return np.arange(n) % 3


def _beyond_x(rng):
    ind = BEYOND_NET["ind"]
    sign = rng.choice(np.array([-1.0, 1.0]), (N, ind))
    inside = rng.uniform(-(2.0 ** 20 - 16.0), 2.0 ** 20 - 16.0, (N, ind))
    beyond = sign * rng.uniform(2.0 ** 20 + 16.0, 2.0 ** 24, (N, ind))            # a bias moves it by less than 16
    cls = beyond_class()[:, None]
    return np.where(cls == 0, inside, np.where(cls == 1, beyond, sign * 3e38)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def beyond_case():
    """The exact case whose p* lies on a row beyond the domain (class 1): sin = +0, cos = 1 there, the gradient passes through."""
    assert beyond_class()[BEYOND_NET["pstar"]] == 1
    return _selection_case(BEYOND_NET, BEYOND_SEED, N, _beyond_x)


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """The forward of beyond_case's net with one NaN and one +inf input element in two rows: dict(x, rows, logits, ins, cos)."""
    e = beyond_case()
    x = e["x"].copy()
    x[BEYOND_NAN_AT], x[BEYOND_INF_AT] = np.nan, np.inf
    logits, ins, cs = sr.np_forward(e["layers"], x, BEYOND_NET["w0"])
    return dict(x=x, rows=(BEYOND_NAN_AT[0], BEYOND_INF_AT[0]), logits=logits, ins=ins, cos=cs)


# ---- batch sweep: selection nets on both sides of every doubling of the slab length (inr_train_cases.BATCH_NS) ---------------------
# (kind, in, hidden, layers, out, w0, n, accumulate).  dlogits has ONE non-zero row per slab -- the slab's first, last or middle
# point for z mod 3 = 0, 1, 2 -- so every slab's partial has one non-zero term and the fixed-order sum over the slabs adds up to
# 64 non-zero partials: inr_siren_ref.np_step_slabs is what the kernels must give bit for bit.
BATCH = ([(KIND_SIREN, 7, 32, 2, 4, 30.0, n, n == 65537) for n in tc.BATCH_NS] +
         [(KIND_RAW_SIREN, 31, 64, 3, 4, 1.0, n, False) for n in tc.BATCH_NS if n <= 32769] +
         [(KIND_SIREN, 7, 256, 3, 4, 30.0, 65537, False)])
BATCH_SEED = 8400
BATCH_REPEAT = (KIND_SIREN, 7, 32, 2, 4, 30.0, 131073, False)      # this case runs its step twice: the same bytes
GUARD_NS = (16385, 65537)                                         # the raw-ABI cases: net 7 -> 32 -> 4 of BATCH at these n
RUN_LONG_MICRO = lc.RUN_LONG_MICRO


def batch_id(c):
    return "%s_in%d_h%d_L%d_o%d_w%g_n%d%s" % ("siren" if c[0] == KIND_SIREN else "raw", *c[1:7], "_acc" if c[7] else "")


def batch_index(ind, hidden, n):
    return next(i for i, c in enumerate(BATCH) if c[1] == ind and c[2] == hidden and c[6] == n)


def slab_rows(n):
    """The one row per slab that carries a non-zero dlogits."""
    rows = []
    for z, (k0, k1) in enumerate(sr.slab_ranges(n)):
        rows.append((k0, k1 - 1, k0 + (k1 - k0) // 2)[z % 3])
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def batch_case(i):
    """dict(net tuple, layers, dims, x, coords, feats, dlogits, rows, init_w, init_b, w0, ref = np_step_slabs)."""
    kind, ind, hid, depth, out, w0, n, acc = BATCH[i]
    rng = np.random.default_rng(BATCH_SEED + i)
    dims = [ind] + [hid] * (depth - 1) + [out]
    layers = sr.selection_net(rng, dims)
    x = rng.uniform(-2.0, 2.0, (n, ind)).astype(np.float32)
    rows = slab_rows(n)
    dl = np.zeros((n, out), np.float32)
    dl[rows] = rng.standard_normal((rows.size, out)).astype(np.float32) + np.float32(3.0)
    nw, nb = sum(a * b for a, b in zip(dims[:-1], dims[1:])), sum(dims[1:])
    init_w = rng.standard_normal(nw).astype(np.float32) if acc else None
    init_b = rng.standard_normal(nb).astype(np.float32) if acc else None
    raw = kind == KIND_RAW_SIREN
    return dict(net=BATCH[i], layers=layers, dims=dims, x=x, coords=None if raw else np.ascontiguousarray(x[:, :3]),
                feats=x if raw else np.ascontiguousarray(x[:, 3:]), dlogits=dl, rows=rows, init_w=init_w, init_b=init_b, w0=w0, n=n, kind=kind,
                ref=sr.np_step_slabs(layers, x, w0, dl, sr.slab_len(n), init_w, init_b))


# ---- tolerance tier ---------------------------------------------------------------------------------------------------------------
# name: (kind, in, hidden, hidden layers, out, n)
E2E = {
    "siren_7_2x32_4_n321": (KIND_SIREN, 7, 32, 2, 4, 321),
    "siren_7_3x256_4_n130": (KIND_SIREN, 7, 256, 3, 4, 130),
    "raw_65_3x64_16_n600": (KIND_RAW_SIREN, 65, 64, 3, 16, 600),
    "siren_11_7x128_3_n257": (KIND_SIREN, 11, 128, 7, 3, 257),
}
E2E_SEED = {name: 8500 + i for i, name in enumerate(E2E)}
W0 = 30.0
DICE_WEIGHT = 0.5
CAP = tc.CAP

# 8 x the worst fp32-CPU deviation over five batch orders, as `python tests/inr_siren_cases.py` prints (2026-10-19)
E2E_TOL = {
    "siren_7_2x32_4_n321": dict(grads=3.03e-6, loss=4.79e-7, aux=1.05e-6, dlogits=1.43e-6, logits=1.63e-6),
    "siren_7_3x256_4_n130": dict(grads=4.05e-6, loss=1.39e-6, aux=1.25e-6, dlogits=2.71e-6, logits=6.13e-6),
    "raw_65_3x64_16_n600": dict(grads=2.46e-6, loss=1.34e-6, aux=7.45e-7, dlogits=1.73e-6, logits=3.6e-6),
    "siren_11_7x128_3_n257": dict(grads=1.26e-5, loss=3.99e-7, aux=1.02e-6, dlogits=4.56e-6, logits=5.65e-6),
}


@functools.lru_cache(maxsize=None)
def e2e_case(name):
    """dict(kind, layers, dims, coords, feats, x, labels, cw, classes, n, ref = the fp64 step)."""
    kind, ind, hid, nh, nc, n = E2E[name]
    rng = np.random.default_rng(E2E_SEED[name])
    dims = [ind] + [hid] * nh + [nc]
    layers = sr.siren_layers(rng, dims, W0)
    coords = (rng.random((n, 3)) * 2 - 1).astype(np.float32)
    feats = rng.standard_normal((n, ind - 3)).astype(np.float32)
    x = sr.input_matrix(coords, feats)
    labels = rng.integers(0, nc, n).astype(np.int32)
    cw = (0.5 + rng.random(nc) * 1.5).astype(np.float32)
    raw = kind == KIND_RAW_SIREN
    ref = sr.step(layers, x.astype(np.float64), W0, tc.tr.model_loss(labels, cw, DICE_WEIGHT, nc))
    return dict(kind=kind, layers=layers, dims=dims, coords=None if raw else coords, feats=x if raw else feats, x=x, labels=labels, cw=cw,
                classes=nc, n=n, M=None if raw else ind - 3, ref=ref)


def e2e_fp32_deviation(name, orders=5, seed=9):
    import torch
    c = e2e_case(name)
    ref = c["ref"]
    rng = np.random.default_rng(seed)
    worst = dict(grads=0.0, loss=0.0, aux=0.0, dlogits=0.0, logits=0.0)
    for _ in range(orders):
        perm = rng.permutation(c["n"])
        got = sr.step(c["layers"], c["x"], W0, tc.tr.model_loss(c["labels"], c["cw"], DICE_WEIGHT, c["classes"], perm), torch.float32, perm)
        worst["grads"] = max(worst["grads"], tc.tr.deviation(ref, got))
        worst["loss"] = max(worst["loss"], abs(got["loss"] - ref["loss"]) / abs(ref["loss"]))
        for k in ("logits", "dlogits", "aux"):
            worst[k] = max(worst[k], tc.rel_max(got[k], ref[k]))
    return worst


def tol(recorded):
    return tc.tol(recorded)


# ---- loop -----------------------------------------------------------------------------------------------------------------------
RUN_NET = dict(M=2, hidden=32, hidden_layers=2, classes=3)         # over inr_loop_cases' "run" cache (two modalities)
RUN_INIT_SEED = 8700


def run_dims():
    return [3 + RUN_NET["M"]] + [RUN_NET["hidden"]] * RUN_NET["hidden_layers"] + [RUN_NET["classes"]]


def run_layers():
    return sr.siren_layers(np.random.default_rng(RUN_INIT_SEED), run_dims(), W0)


def run_cfg(accum, micro=None):
    return dict(lc.run_cfg(accum, micro), w0=W0)


E2E_CONFIG = dict(GLOBAL_BATCH_SIZE=1024, MICRO_BATCH_SIZE=512, HIDDEN_DIMS=[32, 32], LR=3e-3, MIN_LR=1e-4, WARMUP_STEPS=4,
                  TRAIN_STEPS=40, RNG_SEED=7, NUM_CLASSES=4, DICE_WEIGHT=0.5, CLASS_WEIGHTS=[0.5, 1.0, 1.0, 2.0], CLIP_NORM=1.0,
                  CHECKPOINT_EVERY_STEPS=20, W0=30.0)
# first-5 / last-5 mean loss of the fp64 CPU loop on the same batches, and its two means (2026-10-19); the GPU run must fall by
# at least E2E_FALL / 1.5
E2E_FALL = 1.732
E2E_FALL_MEANS = (0.8220, 0.4747)


def e2e_init():
    """siren_init's construction: the list form of siren_init(RNG_SEED, 7, HIDDEN_DIMS, 4, W0)."""
    c = E2E_CONFIG
    rng = np.random.default_rng(c["RNG_SEED"])
    dims = [7] + list(c["HIDDEN_DIMS"]) + [c["NUM_CLASSES"]]
    out = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        lim = np.sqrt(6.0 / a) / (c["W0"] if i == 0 else 1.0)
        out.append({"W": rng.uniform(-lim, lim, (a, b)).astype(np.float32), "b": np.zeros(b, np.float32)})
    return out


def e2e_loop_case():
    c = E2E_CONFIG
    accum = -(-c["GLOBAL_BATCH_SIZE"] // c["MICRO_BATCH_SIZE"])
    cfg = dict(classes=c["NUM_CLASSES"], micro=c["MICRO_BATCH_SIZE"], accum=accum, seed=c["RNG_SEED"], cw=c["CLASS_WEIGHTS"], dw=c["DICE_WEIGHT"],
               peak=c["LR"], end=c["MIN_LR"], warmup=c["WARMUP_STEPS"], decay_steps=max(1, c["TRAIN_STEPS"] - c["WARMUP_STEPS"]),
               clip=c["CLIP_NORM"], w0=c["W0"])
    return dict(layers=e2e_init(), cases=lc.e2e_cases(), cfg=cfg, steps=c["TRAIN_STEPS"])


if __name__ == "__main__":                               # the measurements recorded above
    import pathlib
    import sys
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
    for i, c in enumerate(EXACT):
        e = exact_case(i)
        print("exact", i, exact_id(c), "terms / min |sin| / max |a|:", sr.single_term(e["layers"], e["x"], c["w0"], e["dlogits"]))
    for name in E2E:
        print(name, {k: "%.3g" % (8 * v) for k, v in e2e_fp32_deviation(name).items()})
    e = e2e_loop_case()
    per_step = sr.train(e["layers"], e["cases"], e["cfg"], e["steps"], "float64")["losses"].mean(1)
    print("train_siren case: fp64 mean of the first 5 losses %.4f, of the last 5 %.4f, factor %.3f" %
          (per_step[:5].mean(), per_step[-5:].mean(), per_step[:5].mean() / per_step[-5:].mean()))
