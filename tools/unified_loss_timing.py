#!/usr/bin/env python3
"""Time mrirt_unified_loss (loss, aux and dlogits: three launches) at n = 4000 (the notebook's micro-batch) and n = 65536, C = 4,
beside torch's autograd of the same function in fp32 on the same GPU (clamp, softmax, the per-class sums, pow / log, var; eager)
and beside mrirt_inr_loss_ext on the same logits and labels (focal CE + per-class Dice: the nearest loss the library had), and a
whole train_inject step with the unified keys, which gives the three launches' share of a step.

Inputs and scratch are on the device; after `--warmup` untimed rounds the paths alternate for `--iters` rounds in one process,
each call bracketed by its own pair of events on the launch stream.  Reported: median [min, max] in ms.

    python tools/unified_loss_timing.py [--iters 20] [--warmup 5] [--out profiles/r24_unified_loss/timing.json]
"""
import argparse
import json
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

NC, CW = 4, [0.1, 1.5, 1.0, 2.0]
F, M, HIDDEN = 128, 4, (64, 64, 64)


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


def torch_loss(z, labels, bw, cw, gamma=0.5, lam=0.5, alpha=0.3, beta=0.7, tv_w=0.02, bd_w=0.1):
    """The loss of include/mrirt.h in eager fp32 torch (torch.clamp's gradient is the closed-interval rule)."""
    import torch
    n, C = z.shape
    pc = torch.softmax(z.clamp(-10.0, 10.0), 1).clamp(1e-7, 1.0 - 1e-7)
    pu = torch.softmax(z, 1)
    t = torch.nn.functional.one_hot(labels.long(), C).to(z.dtype)
    P, A, T = pc.sum(0), (pc * t).sum(0), t.sum(0)
    ti = (A / (A + alpha * (P - A) + beta * (T - A) + 1e-7)).clamp(0.0, 1.0)
    mftl = torch.pow(1.0 - ti + 1e-7, 1.0 / gamma).mean()
    q = (pc * t).sum(1)
    mfl = (torch.pow(1.0 - q + 1e-7, gamma) * -torch.log(q + 1e-10)).mean()
    ufl = (lam * mftl + (1.0 - lam) * mfl).clamp(0.0, 1e6)
    dice = (2.0 * A + 1.0) / (P + T + 1.0)
    dl = (1.0 - (dice * cw).sum() / (cw.sum() + 1e-10)).clamp(0.0, 10.0)
    tv = pu.var(0, unbiased=False).sum()
    bl = (bw * (z.argmax(1) - labels).abs()).mean()
    return 0.5 * ufl + 0.5 * dl + tv_w * tv + bd_w * bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from mrirt import inr, synth
    if not torch.cuda.is_available():
        raise SystemExit("unified_loss_timing.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    size = 32
    mods = np.stack([synth.synth_volume(size, 1234 + m, phase=0.3 * m).reshape(size, size, size).transpose(2, 1, 0) for m in range(M)])
    mods = ((mods - mods.mean((1, 2, 3), keepdims=True)) / mods.std((1, 2, 3), keepdims=True)).astype(np.float32)
    seg = np.clip(synth.synth_labels(size).reshape(size, size, size).transpose(2, 1, 0), 0, NC - 1).astype(np.int16)
    cache = inr.VoxelCache([{"mods": np.ascontiguousarray(mods), "seg": np.ascontiguousarray(seg)}])
    cache.set_boundary()
    params = inr.inject_init(1, F, M, HIDDEN, NC)
    cfg = inr.unified_loss(CW)
    ext = inr.loss_ext(CW, 0.5, per_class_dice=True, focal_gamma=2.0)
    cw_t = torch.tensor(CW, dtype=torch.float32, device=dev)
    rows = []
    for n in (4000, 65536):
        rng = np.random.default_rng(n)
        z = torch.from_numpy(rng.normal(0, 2, (n, NC)).astype(np.float32)).to(dev)
        labels = torch.from_numpy(rng.integers(0, NC, n).astype(np.int32)).to(dev)
        bw = torch.from_numpy(rng.random(n).astype(np.float32)).to(dev)
        scratch = inr.unified_loss_scratch(n, dev)
        zt = z.clone().requires_grad_(True)

        def ours():
            return inr.unified_loss_and_dlogits(z, labels, cfg, bw, scratch)

        def loss_ext():
            return inr.loss_and_dlogits(z, labels, CW, 0.5, ext=ext)

        def torch_step():
            zt.grad = None
            torch_loss(zt, labels, bw, cw_t).backward()

        t = alternate({"mrirt_unified_loss": ours, "torch_autograd": torch_step, "mrirt_inr_loss_ext": loss_ext}, args.iters, args.warmup)
        l_ours, _, g_ours = ours()
        torch_step()
        row = dict(n=n, C=NC, scratch_bytes=scratch.numel(), ms=t, ratio_torch_over_mrirt=t["torch_autograd"]["median"] / t["mrirt_unified_loss"]["median"],
                   loss=float(l_ours), torch_loss=float(torch_loss(z, labels, bw, cw_t)), dlogits_max_abs_diff=float((g_ours - zt.grad).abs().max()))
        steps = 10
        config = dict(NUM_CLASSES=NC, RNG_SEED=3, FOURIER_DIM=F, HIDDEN_DIMS=list(HIDDEN), COORD_INJECTION_LAYERS=[1, 2, 3], MODALITY_INJECTION_LAYERS=[2],
                      DROPOUT_RATE=0.3, MICRO_BATCH_SIZE=n, ACCUM_STEPS=1, STAGE1_STEPS=steps, STAGE2_STEPS=0, LR_STAGE1=2e-3, LR_STAGE2=5e-4,
                      MIN_LR=1e-5, WARMUP_STEPS=0, WEIGHT_DECAY=1e-4, CLIP_NORM=1.0, CLASS_WEIGHTS=CW, UNIFIED_FOCAL_GAMMA=0.5, UNIFIED_FOCAL_LAMBDA=0.5,
                      TV_WEIGHT_STAGE1=0.02, TV_WEIGHT_STAGE2=0.05, BOUNDARY_WEIGHT=0.1)

        def loop():
            inr.train_inject(config, cache, params)
        loop_ms = alternate({"train_inject": loop}, max(3, args.iters // 4), 1)["train_inject"]
        row["train_inject_step_ms"] = {k: v / steps for k, v in loop_ms.items()}
        row["loss_share_of_step"] = t["mrirt_unified_loss"]["median"] / row["train_inject_step_ms"]["median"]
        rows.append(row)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
