#!/usr/bin/env python3
"""Fit a small Fourier/ReLU INR to the synthetic label volume with the library's own training step — the optimisation demo
(the reference's docs/Goals.md "Differentiability Proof": a gradient from a loss to the MLP's weights, then a fit).

The fit is ``mrirt.inr.train_inr``: every step draws a batch of voxels from the device-resident case (the counter-based
sampler), runs the fp32 forward, the reference's CE + soft Dice loss and the weight gradients (csrc/inr_train.hip) and applies
AdamW (csrc/inr_optim.hip), all enqueued by ``mrirt_inr_train_run`` in chunks of 100 steps — a constant learning rate, no
clipping.  Loss and per-class Dice of the whole volume are printed before and after; the fitted weights then go through
``pack_mlp`` and ``predict_volume``, the bf16 inference path, whose Dice against the labels is the last line.

``--siren`` fits the notebook's SIREN instead (x = (coords, modalities), ``mrirt.inr.train_siren`` / ``mrirt_siren_train_run``,
the exact-sine step of DESIGN.md section 16); the fitted dict goes through ``pack_mlp(params, KIND_SIREN, 0, 4, w0)`` and
``classify``, and the Dice of those classes against the labels is the last line.

The loss and sampling flags of the reference's scripts/jax_inr_brats.py are taken under their own names (--focal-gamma,
--focal-alpha a,b,c,d, --label-smoothing, --per-class-dice / --no-per-class-dice, --edema-fp-weight, --tversky-edema-alpha / -beta /
-weight, --edema-logit-reg, --tumor-ratio): with any of them the fit runs through ``mrirt_inr_train_run_ext`` (DESIGN.md section
18) and the whole-volume loss printed is the extended one; without them nothing changes.

    python tools/inr_fit.py [--size 48] [--steps 300] [--batch 4096] [--hidden 64] [--layers 4] [--freqs 4] [--lr 3e-3]
    python tools/inr_fit.py --siren [--w0 30] [--lr 1e-3] ...
    python tools/inr_fit.py --focal-gamma 2 --tumor-ratio 0.4 --tversky-edema-weight 0.2 --no-per-class-dice
"""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--layers", type=int, default=4, help="hidden layers")
    ap.add_argument("--freqs", type=int, default=4)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--dice-weight", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--siren", action="store_true", help="fit a SIREN (sine activations) instead of the Fourier/ReLU network")
    ap.add_argument("--w0", type=float, default=30.0)
    ap.add_argument("--per-class-dice", action=argparse.BooleanOptionalAction, default=None, help="mean over classes (the default here) or prevalence-weighted Dice")
    ap.add_argument("--focal-gamma", type=float, default=None)
    ap.add_argument("--focal-alpha", type=str, default=None, help="comma-separated per-class alpha")
    ap.add_argument("--label-smoothing", type=float, default=None)
    ap.add_argument("--edema-fp-weight", type=float, default=None)
    ap.add_argument("--tversky-edema-alpha", type=float, default=None)
    ap.add_argument("--tversky-edema-beta", type=float, default=None)
    ap.add_argument("--tversky-edema-weight", type=float, default=None)
    ap.add_argument("--edema-logit-reg", type=float, default=None)
    ap.add_argument("--tumor-ratio", type=float, default=None)
    args = ap.parse_args()
    import torch
    from mrirt import inr, synth
    n, K, nc = args.size, args.freqs, 4
    dev = torch.device("cuda:0")
    # the synthetic case as predict_volume sees one: mods (M, H, W, D), seg (H, W, D); the grids are x-fastest
    mods = np.stack([synth.synth_volume(n, 1234 + m, phase=0.3 * m).reshape(n, n, n).transpose(2, 1, 0) for m in range(4)])
    mods = ((mods - mods.mean((1, 2, 3), keepdims=True)) / mods.std((1, 2, 3), keepdims=True)).astype(np.float32)
    seg = synth.synth_labels(n).reshape(n, n, n).transpose(2, 1, 0).astype(np.int32)
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    coords = torch.from_numpy((grid / (n - 1) * 2.0 - 1.0).astype(np.float32)).to(dev)
    feats = torch.from_numpy(np.ascontiguousarray(mods.transpose(1, 2, 3, 0).reshape(-1, 4))).to(dev)
    labels = torch.from_numpy(seg.reshape(-1)).to(dev)
    counts = np.bincount(seg.reshape(-1), minlength=nc).astype(np.float64)
    cw = (counts.sum() / (nc * np.maximum(counts, 1.0))).astype(np.float32)          # inverse-frequency class weights

    # the extended-loss / sampling keys the user gave, under train_inr's names; none: today's run
    extra = {k.upper(): v for k, v in vars(args).items() if k.upper() in inr.EXT_CONFIG_KEYS and v is not None}
    if "FOCAL_ALPHA" in extra:
        extra["FOCAL_ALPHA"] = [float(v) for v in extra["FOCAL_ALPHA"].split(",")]
    args.extra = extra
    args.ext = inr.loss_ext_of_config(dict(extra, CLASS_WEIGHTS=[float(v) for v in cw], DICE_WEIGHT=args.dice_weight), nc) if extra else None
    if args.siren:
        return fit_siren(args, inr, dev, mods, seg, coords, feats, labels, cw, nc)
    params = [{k: torch.from_numpy(v).to(dev) for k, v in p.items()} for p in inr.init_mlp(args.seed, 3 + 6 * K + 4, [args.hidden] * args.layers, nc)]
    step = inr.make_loss_and_grad(nc, cw, args.dice_weight, K, ext=args.ext)
    config = dict(GLOBAL_BATCH_SIZE=args.batch, MICRO_BATCH_SIZE=args.batch, FOURIER_FREQS=K, HIDDEN_DIMS=[args.hidden] * args.layers, LR=args.lr,
                  MIN_LR=args.lr, WARMUP_STEPS=0, TRAIN_STEPS=args.steps, RNG_SEED=args.seed, NUM_CLASSES=nc, DICE_WEIGHT=args.dice_weight,
                  CLASS_WEIGHTS=[float(v) for v in cw], CLIP_NORM=float("inf"), CHECKPOINT_EVERY_STEPS=100, **args.extra)

    def whole_volume(tag):
        (loss, aux), _ = step(params, coords, feats, labels)
        print(f"{tag}: loss {float(loss):.4f}  soft dice per class {[round(float(v), 4) for v in aux['dice_per_class'].cpu()]}"
              f"  ce per class {[round(float(v), 4) for v in aux['ce_per_class'].cpu()]}")
    whole_volume("before")

    def log(it, m):
        if it % 100 == 0:
            print(f"step {it}: batch loss {m['train/loss']:.4f}")
    host, _ = inr.train_inr(config, [{"mods": mods, "seg": seg}], params=[{k: v.cpu().numpy() for k, v in p.items()} for p in params], log=log)
    params = [{k: torch.from_numpy(v).to(dev) for k, v in p.items()} for p in host]
    whole_volume("after")
    net = inr.pack_mlp(host, inr.KIND_FOURIER_RELU, K, 4)
    pred, _ = inr.predict_volume(host, {"mods": mods, "seg": seg}, K, net=net)
    dice = inr.dice_score(pred, torch.from_numpy(seg).to(dev), nc)
    print("predict_volume (bf16 inference path) dice per class:", {c: round(v, 4) for c, v in dice.items()})


def fit_siren(args, inr, dev, mods, seg, coords, feats, labels, cw, nc):
    import torch
    params = inr.siren_init(args.seed, 7, [args.hidden] * args.layers, nc, args.w0)
    step = inr.make_siren_loss_and_grad(nc, cw, args.dice_weight, args.w0, ext=args.ext)
    config = dict(GLOBAL_BATCH_SIZE=args.batch, MICRO_BATCH_SIZE=args.batch, HIDDEN_DIMS=[args.hidden] * args.layers, LR=args.lr, MIN_LR=args.lr,
                  WARMUP_STEPS=0, TRAIN_STEPS=args.steps, RNG_SEED=args.seed, NUM_CLASSES=nc, DICE_WEIGHT=args.dice_weight,
                  CLASS_WEIGHTS=[float(v) for v in cw], CLIP_NORM=float("inf"), CHECKPOINT_EVERY_STEPS=100, W0=args.w0, **args.extra)

    def whole_volume(tag, p):
        (loss, aux), _ = step(p, coords, feats, labels)
        print(f"{tag}: loss {float(loss):.4f}  soft dice per class {[round(float(v), 4) for v in aux['dice_per_class'].cpu()]}"
              f"  ce per class {[round(float(v), 4) for v in aux['ce_per_class'].cpu()]}")
    whole_volume("before", params)

    def log(it, m):
        if it % 100 == 0:
            print(f"step {it}: batch loss {m['train/loss']:.4f}")
    params, _ = inr.train_siren(config, [{"mods": mods, "seg": seg}], params=params, log=log)
    whole_volume("after", params)
    net = inr.pack_mlp(params, inr.KIND_SIREN, 0, 4, args.w0)
    pred = inr.classify(net, coords, feats).reshape(seg.shape)
    dice = inr.dice_score(pred, torch.from_numpy(seg).to(dev), nc)
    print("classify (bf16 inference path) dice per class:", {c: round(v, 4) for c, v in dice.items()})


if __name__ == "__main__":
    main()
