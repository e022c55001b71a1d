#!/usr/bin/env python3
"""Fit a small Fourier/ReLU INR to the synthetic label volume with the library's own training step — the optimisation demo
(the reference's docs/Goals.md "Differentiability Proof": a gradient from a loss to the MLP's weights, then a fit).

Every step draws a random batch of voxels, runs ``mrirt.inr.make_loss_and_grad`` (fp32 forward, the reference's CE + soft
Dice loss and the weight gradients, all in csrc/inr_train.hip) and hands the gradients to ``torch.optim.AdamW``.  Loss and
per-class Dice of the whole volume are printed before and after; the fitted weights then go through ``pack_mlp`` and
``predict_volume``, the bf16 inference path, whose Dice against the labels is the last line.

    python tools/inr_fit.py [--size 48] [--steps 300] [--batch 4096] [--hidden 64] [--layers 4] [--freqs 4] [--lr 3e-3]
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

    rng = np.random.default_rng(args.seed)
    dims = [3 + 6 * K + 4] + [args.hidden] * args.layers + [nc]
    params = []
    for a, b in zip(dims[:-1], dims[1:]):                # init_mlp of the reference: Glorot weights, zero biases
        lim = np.sqrt(6.0 / (a + b))
        params.append({"W": torch.from_numpy(rng.uniform(-lim, lim, (a, b)).astype(np.float32)).to(dev),
                       "b": torch.zeros(b, dtype=torch.float32, device=dev)})
    flat = [p[k] for p in params for k in ("W", "b")]
    opt = torch.optim.AdamW(flat, lr=args.lr, weight_decay=0.0)
    step = inr.make_loss_and_grad(nc, cw, args.dice_weight, K)

    def whole_volume(tag):
        (loss, aux), _ = step(params, coords, feats, labels)
        print(f"{tag}: loss {float(loss):.4f}  soft dice per class {[round(float(v), 4) for v in aux['dice_per_class'].cpu()]}"
              f"  ce per class {[round(float(v), 4) for v in aux['ce_per_class'].cpu()]}")
    whole_volume("before")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    for it in range(args.steps):
        idx = torch.randint(0, coords.shape[0], (args.batch,), device=dev, generator=gen)
        (loss, _), grads = step(params, coords[idx], feats[idx], labels[idx])
        for p, g in zip(params, grads):
            p["W"].grad, p["b"].grad = g["W"], g["b"]
        opt.step()
        if (it + 1) % 100 == 0:
            print(f"step {it + 1}: batch loss {float(loss):.4f}")
    whole_volume("after")
    host = [{"W": p["W"].cpu().numpy(), "b": p["b"].cpu().numpy()} for p in params]
    net = inr.pack_mlp(host, inr.KIND_FOURIER_RELU, K, 4)
    pred, _ = inr.predict_volume(host, {"mods": mods, "seg": seg}, K, net=net)
    dice = inr.dice_score(pred, torch.from_numpy(seg).to(dev), nc)
    print("predict_volume (bf16 inference path) dice per class:", {c: round(v, 4) for c, v in dice.items()})


if __name__ == "__main__":
    main()
