#!/usr/bin/env python3
"""tools/inject_fit_unified.py's 48^3 synthetic fit with the notebook's whole training procedure: train_inject with the unified keys
and the hybrid, uncertainty-guided sampler (UNCERTAINTY_RATIO 0.5, 0.75 in stage 2, BALANCED_RATIO 0.3) and the decaying coordinate
noise (COORD_NOISE_SIGMA_INIT / _FINAL), the loss curve and its four terms, and the Dice per class of predict_full_volume against
the labels it was trained on, beside the figures of the same fit on uniform batches (profiles/r24_unified_loss/fit.json): evidence
that the sampler trains the network, not a test bar.

    python tools/inject_fit_hybrid.py [--steps 300] [--out profiles/r25_hybrid/fit.json]
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--sigma-init", type=float, default=0.3)         # the notebook's COORD_NOISE_SIGMA_INIT
    ap.add_argument("--sigma-final", type=float, default=0.1)        # ... and _FINAL
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from mrirt import inr, synth
    if not torch.cuda.is_available():
        raise SystemExit("inject_fit_hybrid.py trains on the GPU; there is none here")
    size, M, nc = args.size, 4, 4
    mods = np.stack([synth.synth_volume(size, 1234 + m, phase=0.3 * m).reshape(size, size, size).transpose(2, 1, 0) for m in range(M)])
    mods = ((mods - mods.mean((1, 2, 3), keepdims=True)) / mods.std((1, 2, 3), keepdims=True)).astype(np.float32)
    seg = synth.synth_labels(size).reshape(size, size, size).transpose(2, 1, 0).astype(np.int16)
    seg = np.ascontiguousarray(np.clip(seg, 0, nc - 1))
    case = {"mods": np.ascontiguousarray(mods), "seg": seg}
    stage1 = (2 * args.steps) // 3
    config = dict(NUM_CLASSES=nc, RNG_SEED=42, FOURIER_DIM=128, HIDDEN_DIMS=[64, 64, 64], COORD_INJECTION_LAYERS=[1, 2, 3], MODALITY_INJECTION_LAYERS=[2],
                  DROPOUT_RATE=0.1, MICRO_BATCH_SIZE=4000, ACCUM_STEPS=2, STAGE1_STEPS=stage1, STAGE2_STEPS=args.steps - stage1, LR_STAGE1=2e-3,
                  LR_STAGE2=5e-4, MIN_LR=1e-5, WARMUP_STEPS=max(1, args.steps // 15), WEIGHT_DECAY=1e-4, CLIP_NORM=1.0,
                  CLASS_WEIGHTS=[0.1, 1.5, 1.0, 2.0], UNIFIED_FOCAL_GAMMA=0.5, UNIFIED_FOCAL_LAMBDA=0.5, TV_WEIGHT_STAGE1=0.02, TV_WEIGHT_STAGE2=0.05,
                  BOUNDARY_WEIGHT=0.1, UNCERTAINTY_RATIO=0.5, UNCERTAINTY_RATIO_STAGE2=0.75, BALANCED_RATIO=0.3, UNIFORM_RATIO=0.2,
                  UNCERTAINTY_MC_SAMPLES=5, COORD_NOISE_SIGMA_INIT=args.sigma_init, COORD_NOISE_SIGMA_FINAL=args.sigma_final)
    curve = []
    every = max(1, args.steps // 10)

    def log(step, m):
        if step == 1 or step % every == 0:
            curve.append({k.split("/")[1]: (round(v, 6) if isinstance(v, float) else v) for k, v in m.items() if k != "train/lr"})

    t0 = time.time()
    params, state = inr.train_inject(config, [case], log=log)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    pred, _ = inr.predict_full_volume(params, case)
    dice = inr.dice_score(pred, seg, nc)
    first = inr.inject_init(42, 128, M, [64, 64, 64], nc)
    dice0 = inr.dice_score(inr.predict_full_volume(first, case)[0], seg, nc)
    h = state["loss_history"]
    res = dict(device=torch.cuda.get_device_name(0), size=size, steps=args.steps, seconds_with_a_log_every_step=seconds, config={k: v for k, v in config.items()},
               class_voxels=[int((seg == c).sum()) for c in range(nc)], loss_first=h[0], loss_last=float(np.mean(h[-10:])), curve=curve,
               dice_per_class={str(k): float(v) for k, v in dice.items()}, dice_per_class_at_init={str(k): float(v) for k, v in dice0.items()},
               B_moved=float(np.abs(params["fourier"]["B"] - first["fourier"]["B"]).max()))
    before = ROOT / "profiles" / "r24_unified_loss" / "fit.json"
    if before.exists():                                  # the same fit on uniform batches, as recorded
        res["dice_per_class_uniform_batches"] = json.loads(before.read_text())["dice_per_class"]
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
