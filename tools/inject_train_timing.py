#!/usr/bin/env python3
"""Time the coordinate-injection INR's training step -- mrirt_inject_forward_train + mrirt_inr_loss + mrirt_inject_backward --
and a whole train_inject step (sampler, step, clipped AdamW), at the notebook's shape (F 128, M 4, 64/64/64/4, coordinates into
layers 1 and 2, modalities into layer 2) for n = 4000 (the notebook's micro-batch) and n = 65536, beside torch's autograd of the
same function on the same GPU (fp32 eager: sin / cos features, cat, addmm, relu, a fixed dropout mask; the same mrirt_inr_loss
gives both paths their dlogits).

Inputs, weights and scratch are on the device; after `--warmup` untimed rounds the two paths alternate for `--iters` rounds in
one process, each call bracketed by its own pair of events on the launch stream.  Reported: median [min, max] in ms, and the
step's algorithmic matrix FLOPs (2 n in out per product: forward, X^T dZ with the row of ones, dZ W^T over the rows that get a
gradient, g^T c01) over the step time as a share of the 157 TFLOP/s fp32-matrix peak -- a whole-step figure, not a kernel's.

    python tools/inject_train_timing.py [--iters 20] [--warmup 5] [--out profiles/r23_inject_train/timing.json]
"""
import argparse
import json
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

F, M, HIDDEN, NC, CL, ML = 128, 4, (64, 64, 64), 4, (1, 2), (2,)
CW, DW, KEEP = [0.5, 1.0, 2.0, 1.5], 0.3, 0.7
PEAK_FP32_MATRIX = 157e12


def alternate(fns, iters, warmup):
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in ms.items()}


def step_flops(n, ins, outs, splits):
    per_point = sum(i * o + (i + 1) * o + s * o for i, o, s in zip(ins, outs, splits)) + (F // 2) * 3
    return 2 * n * per_point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from mrirt import inr, synth
    if not torch.cuda.is_available():
        raise SystemExit("inject_train_timing.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    size = 32
    mods = np.stack([synth.synth_volume(size, 1234 + m, phase=0.3 * m).reshape(size, size, size).transpose(2, 1, 0) for m in range(M)])
    mods = ((mods - mods.mean((1, 2, 3), keepdims=True)) / mods.std((1, 2, 3), keepdims=True)).astype(np.float32)
    seg = synth.synth_labels(size).reshape(size, size, size).transpose(2, 1, 0).astype(np.int16)
    cache = inr.VoxelCache([{"mods": np.ascontiguousarray(mods), "seg": np.ascontiguousarray(seg)}])
    params = inr.inject_init(1, F, M, HIDDEN, NC, CL, ML)
    desc = inr.inject_desc(params, CL, ML)
    widths = list(HIDDEN) + [NC]
    ins = inr._inject_in_dims(F, M, widths, CL, ML)
    splits = [F] + widths[:-1]
    rows = []
    for n in (4000, 65536):
        rng = np.random.default_rng(n)
        coords = torch.from_numpy((rng.random((n, 3)) * 2 - 1).astype(np.float32)).to(dev)
        feats = torch.from_numpy(rng.standard_normal((n, M)).astype(np.float32)).to(dev)
        labels = torch.from_numpy(rng.integers(0, NC, n).astype(np.int32)).to(dev)
        B, w, b = inr._inject_flat(params, dev)
        scratch = inr.inject_train_scratch(desc, n, dev)
        drop = inr.inject_dropout(7, KEEP, 1, 0, 0)
        gB, gw, gb = torch.empty_like(B), torch.empty_like(w), torch.empty_like(b)

        def ours():
            logits = inr.inject_forward_train(desc, B, w, b, coords, feats, n, scratch, drop)
            _, _, dl = inr.loss_and_dlogits(logits, labels, CW, DW, scratch)
            return inr.inject_backward(desc, B, w, coords, feats, n, dl, scratch, drop, gB, gw, gb)

        tB = B.clone().requires_grad_(True)
        tW = [torch.from_numpy(p["W"]).to(dev).requires_grad_(True) for p in params["mlp"]]
        tb = [torch.from_numpy(p["b"]).to(dev).requires_grad_(True) for p in params["mlp"]]
        masks = [(torch.rand((n, wd), device=dev) < KEEP).to(torch.float32) / KEEP for wd in HIDDEN]
        loss_scratch = torch.empty(max(int(inr._lib.lib().mrirt_inr_loss_scratch_bytes(n)), 16), dtype=torch.uint8, device=dev)

        def torch_step():
            for t in (tB, *tW, *tb):
                t.grad = None
            a = 6.2831855 * (((coords + 1.0) * 0.5) @ tB.T)
            h = torch.cat([torch.sin(a), torch.cos(a), feats], 1)
            for l, (W, bias) in enumerate(zip(tW, tb)):
                if 0 < l < len(tW) - 1:
                    h = torch.cat([h] + ([coords] if l in CL else []) + ([feats] if l in ML else []), 1)
                h = torch.addmm(bias, h, W)
                if l < len(tW) - 1:
                    h = torch.relu(h) * masks[l]
            _, _, dl = inr.loss_and_dlogits(h.detach(), labels, CW, DW, loss_scratch)
            h.backward(dl)

        t = alternate({"mrirt": ours, "torch": torch_step}, args.iters, args.warmup)
        flop = step_flops(n, ins, widths, splits)
        row = dict(n=n, scratch_bytes=scratch.numel(), step_ms=t["mrirt"], torch_step_ms=t["torch"],
                   ratio_torch_over_mrirt=t["torch"]["median"] / t["mrirt"]["median"], step_matrix_flop=flop,
                   step_share_of_fp32_matrix_peak=flop / (t["mrirt"]["median"] * 1e-3) / PEAK_FP32_MATRIX)
        # a whole train_inject step: sampler + step + clipped AdamW, per step of a run without a log (nothing waits in between)
        steps = 10
        config = dict(NUM_CLASSES=NC, RNG_SEED=3, FOURIER_DIM=F, HIDDEN_DIMS=list(HIDDEN), COORD_INJECTION_LAYERS=[1, 2, 3], MODALITY_INJECTION_LAYERS=[2],
                      DROPOUT_RATE=0.3, MICRO_BATCH_SIZE=n, ACCUM_STEPS=1, STAGE1_STEPS=steps, STAGE2_STEPS=0, LR_STAGE1=2e-3, LR_STAGE2=5e-4,
                      MIN_LR=1e-5, WARMUP_STEPS=0, WEIGHT_DECAY=1e-4, CLIP_NORM=1.0, CLASS_WEIGHTS=CW, DICE_WEIGHT=DW)

        def loop():
            inr.train_inject(config, cache, params)
        loop_ms = alternate({"train_inject": loop}, max(3, args.iters // 4), 1)["train_inject"]
        row["train_inject_step_ms"] = {k: v / steps for k, v in loop_ms.items()}
        rows.append(row)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, net=dict(F=F, M=M, widths=widths, coord_layers=CL, mod_layers=ML, keep=KEEP),
               rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
