#!/usr/bin/env python3
"""Time one optimiser step through mrirt_inr_train_run_ext with a full ext — the extended loss of scripts/jax_inr_brats.py
(focal CE with alpha, label smoothing, prevalence-weighted Dice, the three edema terms) and TUMOR_RATIO 0.4 — beside the same
step with every member of ext NULL / 0 (the launches of mrirt_siren_train_run / mrirt_inr_train_run), in the same process.

Shapes: the SIREN 7 -> 3 x 256 -> 4 and the Fourier/ReLU net 103 -> 4 x 256 -> 4 (K = 16, four modalities), at micro-batches
of 4096 and 65536 points.  Per row: cache, weights and scratch already on the device, `--warmup` untimed calls, then `--iters`
calls of `--run-steps` steps (accum 1, sampler included) each bracketed by its own pair of events on the launch stream; the
figure is the median per step.  Nothing is read back.

    python tools/lossx_timing.py [--iters 20] [--warmup 5] [--out profiles/r14_lossx/timing.json]
"""
import argparse
import json
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

NETS = [dict(family="siren", K=0, hidden=256, hidden_layers=3), dict(family="relu", K=16, hidden=256, hidden_layers=4)]
NS = (4096, 65536)
CW, DW, W0, M, NC, RATIO = [0.5, 1.0, 2.0, 1.5], 0.5, 30.0, 4, 4, 0.4
LOSS = dict(per_class_dice=False, focal_gamma=2.0, focal_alpha=[0.25, 1.0, 0.5, 2.0], label_smoothing=0.05, edema_fp_weight=0.3,
            tversky_edema_alpha=0.8, tversky_edema_beta=0.2, tversky_edema_weight=0.4, edema_logit_reg=0.2, edema_class=2)


def timed(fn, iters, warmup, per=1):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / per)
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--run-steps", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctypes as C
    import torch
    import inr_ref
    from mrirt import _lib, inr, synth
    dev = torch.device("cuda:0")
    size = 32
    mods = np.stack([synth.synth_volume(size, 1234 + m, phase=0.3 * m).reshape(size, size, size).transpose(2, 1, 0) for m in range(M)])
    mods = ((mods - mods.mean((1, 2, 3), keepdims=True)) / mods.std((1, 2, 3), keepdims=True)).astype(np.float32)
    seg = synth.synth_labels(size).reshape(size, size, size).transpose(2, 1, 0).astype(np.int16)
    cache = inr.VoxelCache([{"mods": np.ascontiguousarray(mods), "seg": np.ascontiguousarray(seg)}])
    cache.tumour_index()                                 # load time: not part of a step
    tumour_fraction = float((seg > 0).mean())
    rows = []
    for net in NETS:
        for n in NS:
            rng = np.random.default_rng(1)
            dims = [3 + 6 * net["K"] + M] + [net["hidden"]] * net["hidden_layers"] + [NC]
            if net["family"] == "siren":
                layers, desc = inr_ref.siren_params(rng, dims), inr.siren_train_desc(dims, M, W0)
            else:
                layers, desc = inr_ref.fourier_params(rng, dims), inr.train_desc(dims, net["K"], M)
            cfg = inr.train_cfg(n, 1, 3, CW, DW, 1e-4, 1e-5, 2, 1000, 1.0)
            row = dict(family=net["family"], dims=dims, n=n, n_tumour=inr.n_tumour_of(n, RATIO))
            exts = dict(plain=inr.train_ext(), full=inr.train_ext(cache, inr.loss_ext(CW, DW, **LOSS), None, row["n_tumour"]))
            for name, ext in exts.items():
                st = inr.AdamWState.from_params(layers)
                nbytes = int(_lib.lib().mrirt_inr_train_run_ext_scratch_bytes(C.byref(desc), C.byref(cache.desc), C.byref(cfg), C.byref(ext)))
                scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # one buffer for every timed call

                def run():
                    return inr.train_run(desc, cache, cfg, st, args.run_steps, scratch, ext=ext)
                row[name] = dict(scratch_bytes=nbytes, optimiser_step_ms=timed(run, args.iters, max(1, args.warmup // 2), per=args.run_steps))
            row["ratio_full_over_plain"] = row["full"]["optimiser_step_ms"]["median"] / row["plain"]["optimiser_step_ms"]["median"]
            rows.append(row)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, run_steps=args.run_steps, tumor_ratio=RATIO,
               cache_tumour_fraction=tumour_fraction, loss=LOSS, rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
