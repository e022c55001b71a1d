"""The cases of the INR training-loop tests, built on the CPU; shared by the reference, host, sanitizer and GPU tests.  No GPU.

Caches (``cache_cases(name)``: a list of {"mods" (M, H, W, D) fp32, "seg" (H, W, D) int16}):
  addr      2 cases of 3 x 5 x 7, M = 2, whose voxels encode their own address: mods[c][m][x][y][z] = (((c 2 + m) 3 + x) 5 + y) 7 + z,
            seg[c][x][y][z] = c 105 + (x 5 + y) 7 + z — a wrong case, modality, axis order or offset is a wrong integer
  m0 / m8   no modality (4 x 3 x 5, one case) and eight (2 cases of 3 x 4 x 5)
  tiny      one case of 2 x 2 x 2, M = 1
  three     3 cases of 17 x 9 x 33, M = 4
  run       the same three-case geometry with M = 2 and labels in 0..2: the cache of the run / trajectory tests, whose network
            takes two modalities

Trajectory tolerance (rule of DESIGN.md section 14): TRAJ_TOL is 8 x the worst deviation of the same 8 steps evaluated in
fp32 on the CPU with every micro-batch in five random orders from the fp64 run, relative to the largest fp64 magnitude per
layer (parameters) and over the 16 losses.  Measured by ``python tests/inr_loop_ref.py`` on 2026-10-18 (torch CPU); never
taken from the kernel.  The same script checks that at most 2 % of the points of the last micro-batch have a hidden
pre-activation within 2e-5 x rms of the ReLU kink, and prints the factor by which the fp64 reference of the
``train_inr`` case lowers the loss (E2E_SPARE; the test asks for any decrease, the reference must show 1.5 x).
"""
import functools

import numpy as np

SAMPLER_CACHES = ["addr", "m0", "m8", "tiny", "three"]
BATCH_SIZES = [1, 63, 64, 65, 4097]
BATCH_INDICES = [0, 1, 2 ** 32 + 5]
SEEDS = [12345, (0xC0FFEE << 32) | 77]              # the second one has a non-zero high word

_SHAPES = {"addr": (2, 2, (3, 5, 7)), "m0": (1, 0, (4, 3, 5)), "m8": (2, 8, (3, 4, 5)), "tiny": (1, 1, (2, 2, 2)),
           "three": (3, 4, (17, 9, 33)), "run": (3, 2, (17, 9, 33))}


def cache_shape(name):
    return _SHAPES[name]


@functools.lru_cache(maxsize=None)
def cache_cases(name):
    n, M, (H, W, D) = _SHAPES[name]
    if name == "addr":
        x, y, z = np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing="ij")
        return [{"mods": np.stack([((((c * 2 + m) * 3 + x) * 5 + y) * 7 + z) for m in range(M)]).astype(np.float32),
                 "seg": (c * 105 + (x * 5 + y) * 7 + z).astype(np.int16)} for c in range(n)]
    rng = np.random.default_rng(8100 + sorted(_SHAPES).index(name))
    hi = 3 if name == "run" else 4
    return [{"mods": rng.standard_normal((M, H, W, D)).astype(np.float32), "seg": rng.integers(0, hi, (H, W, D)).astype(np.int16)}
            for _ in range(n)]


# ---- AdamW ---------------------------------------------------------------------------------------------------------------------
ADAMW_SIZES = [1, 3, 4, 5, 255, 256, 257, 4 * 256 * 64 + 7]      # nw + nb: the float4 tails and the block tails
ADAMW_STEPS = [0, 999]
ADAMW_FLOAT_N = 70000


def adamw_split(n):
    """(nw, nb) with nw + nb = n, nw >= 1: the biases take about a tenth (none when n == 1)."""
    nb = n // 10 if n > 3 else (n - 1)
    return n - nb, nb


@functools.lru_cache(maxsize=None)
def adamw_case(n, integer=True):
    """Parameters, moments (second moments >= 0) and gradients of n elements; integer gradients in -3..3."""
    rng = np.random.default_rng(9000 + n)
    g = rng.integers(-3, 4, n).astype(np.float32) if integer else (rng.standard_normal(n) * 0.3).astype(np.float32)
    if integer and not g.any():
        g[0] = 2.0
    return dict(p=rng.standard_normal(n).astype(np.float32), mu=(rng.standard_normal(n) * 0.1).astype(np.float32),
                nu=(rng.random(n) * 0.01).astype(np.float32), g=g)


# ---- run = composition, trajectory ---------------------------------------------------------------------------------------------
RUN_NET = dict(K=2, M=2, hidden=32, hidden_layers=2, classes=3, micro=300)
RUN_SEED = 4242
RUN_CW = [0.75, 1.0, 1.5]
RUN_DW = 0.5
TRAJ_STEPS = 8
TRAJ_ACCUM = 2
TRAJ_INIT_SEED = 31
# 8 x the worst fp32-CPU deviation over five batch orders, as `python tests/inr_loop_ref.py` prints (2026-10-18)
TRAJ_TOL = dict(params=1.71e-6, losses=8.99e-7)
TRAJ_NEAR_KINK = 0.0        # fraction of the last micro-batch's points near the kink in the fp64 run (bar: 0.02)


RUN_LONG_MICRO = 16385      # the first micro-batch with 512-point slabs (33 of them, the last of one point)


def run_cfg(accum, micro=None):
    """The configuration of the run tests: clipping active (the raw norm is above it at the start), warm-up then cosine."""
    return dict(K=RUN_NET["K"], classes=RUN_NET["classes"], micro=micro or RUN_NET["micro"], accum=accum, seed=RUN_SEED, cw=RUN_CW, dw=RUN_DW,
                peak=5e-3, end=1e-4, warmup=2, decay_steps=12, clip=0.25)


def run_layers(seed=TRAJ_INIT_SEED):
    rng = np.random.default_rng(seed)
    dims = [3 + 6 * RUN_NET["K"] + RUN_NET["M"]] + [RUN_NET["hidden"]] * RUN_NET["hidden_layers"] + [RUN_NET["classes"]]
    out = []
    for a, b in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (a + b))
        out.append({"W": rng.uniform(-lim, lim, (a, b)).astype(np.float32), "b": (rng.standard_normal(b) * 0.05).astype(np.float32)})
    return out


def traj_case():
    return dict(layers=run_layers(), cases=cache_cases("run"), cfg=run_cfg(TRAJ_ACCUM))


# ---- train_inr end to end -------------------------------------------------------------------------------------------------------
E2E_CONFIG = dict(GLOBAL_BATCH_SIZE=1024, MICRO_BATCH_SIZE=512, FOURIER_FREQS=2, HIDDEN_DIMS=[32, 32], LR=1e-2, MIN_LR=1e-4, WARMUP_STEPS=4,
                  TRAIN_STEPS=40, RNG_SEED=7, NUM_CLASSES=4, DICE_WEIGHT=0.5, CLASS_WEIGHTS=[0.5, 1.0, 1.0, 2.0], CLIP_NORM=1.0,
                  CHECKPOINT_EVERY_STEPS=20)
E2E_SPARE = 2.587          # first-5 / last-5 mean loss of the fp64 CPU reference of this run (must be >= 1.5)


@functools.lru_cache(maxsize=None)
def e2e_cases():
    """Two 16^3 synthetic cases (mrirt.synth): four z-scored modalities each and the nested-sphere labels, as (M, H, W, D) /
    (H, W, D) arrays (the grids are x-fastest)."""
    from mrirt import synth
    n, out = 16, []
    for c in range(2):
        mods = np.stack([synth.synth_volume(n, 1234 + 10 * c + m, phase=0.3 * m).reshape(n, n, n).transpose(2, 1, 0) for m in range(4)])
        mods = ((mods - mods.mean((1, 2, 3), keepdims=True)) / mods.std((1, 2, 3), keepdims=True)).astype(np.float32)
        out.append({"mods": np.ascontiguousarray(mods), "seg": np.ascontiguousarray(synth.synth_labels(n).reshape(n, n, n).transpose(2, 1, 0)).astype(np.int16)})
    return out


def e2e_init():
    """init_mlp's construction (Glorot-uniform weights from a NumPy generator seeded with RNG_SEED, zero biases)."""
    c = E2E_CONFIG
    rng = np.random.default_rng(c["RNG_SEED"])
    dims = [3 + 6 * c["FOURIER_FREQS"] + 4] + list(c["HIDDEN_DIMS"]) + [c["NUM_CLASSES"]]
    out = []
    for a, b in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (a + b))
        out.append({"W": rng.uniform(-lim, lim, (a, b)).astype(np.float32), "b": np.zeros(b, np.float32)})
    return out


def e2e_case():
    c = E2E_CONFIG
    accum = -(-c["GLOBAL_BATCH_SIZE"] // c["MICRO_BATCH_SIZE"])
    cfg = dict(K=c["FOURIER_FREQS"], classes=c["NUM_CLASSES"], micro=c["MICRO_BATCH_SIZE"], accum=accum, seed=c["RNG_SEED"], cw=c["CLASS_WEIGHTS"],
               dw=c["DICE_WEIGHT"], peak=c["LR"], end=c["MIN_LR"], warmup=c["WARMUP_STEPS"], decay_steps=max(1, c["TRAIN_STEPS"] - c["WARMUP_STEPS"]),
               clip=c["CLIP_NORM"])
    return dict(layers=e2e_init(), cases=e2e_cases(), cfg=cfg, steps=c["TRAIN_STEPS"])
