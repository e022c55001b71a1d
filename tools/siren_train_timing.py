#!/usr/bin/env python3
"""Time the SIREN training step — mrirt_siren_forward_f32 + mrirt_inr_loss + mrirt_siren_backward — and one optimiser step
through mrirt_siren_train_run, beside the ReLU step and loop of the same layer widths on the same GPU (the Fourier kind with
K = 0: the same 7 inputs, the same matrix products, no sine), and report the ratios.

Per shape: inputs, weights and scratch already on the device, `--warmup` untimed calls, then `--iters` calls each bracketed by
its own pair of events on the launch stream (device time of the whole pipeline of launches; nothing is read back).  The
optimiser step is timed as one mrirt_*_train_run call of `--run-steps` steps (accum 1, sampler included) divided by the count.

    python tools/siren_train_timing.py [--iters 20] [--warmup 5] [--out profiles/r11_siren_train/timing.json]
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

SHAPES = [dict(hidden=256, hidden_layers=hl, classes=4, n=n) for hl in (3, 4) for n in (4096, 65536)]      # the notebook's net, C5's
CW, DW, W0, M = [0.5, 1.0, 2.0, 1.5], 0.5, 30.0, 4


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
    rows = []
    for s in SHAPES:
        rng = np.random.default_rng(1)
        dims = [3 + M] + [s["hidden"]] * s["hidden_layers"] + [s["classes"]]
        n = s["n"]
        coords = torch.from_numpy((rng.random((n, 3)) * 2 - 1).astype(np.float32)).to(dev)
        feats = torch.from_numpy(rng.standard_normal((n, M)).astype(np.float32)).to(dev)
        labels = torch.from_numpy(rng.integers(0, s["classes"], n).astype(np.int32)).to(dev)
        row = dict(shape=s, dims=dims)
        for family in ("siren", "relu"):
            if family == "siren":
                layers = inr_ref.siren_params(rng, dims)
                desc = inr.siren_train_desc(dims, M, W0)
                scratch = inr.siren_train_scratch(desc, n, dev)
                fwd, bwd = inr.siren_forward_f32, inr.siren_backward_f32
            else:
                layers = inr_ref.fourier_params(rng, dims)
                desc = inr.train_desc(dims, 0, M)
                scratch = inr.train_scratch(desc, n, dev)
                fwd, bwd = inr.forward_f32, inr.backward_f32
            st = inr.AdamWState.from_params(layers)
            w_flat, b_flat = st.w.clone(), st.b.clone()

            def forward():
                return fwd(desc, w_flat, b_flat, coords, feats, n, scratch)

            def step():
                logits = forward()
                _, _, dl = inr.loss_and_dlogits(logits, labels, CW, DW, scratch)
                return bwd(desc, w_flat, n, dl, scratch)

            cfg = inr.train_cfg(n, 1, 3, CW, DW, 1e-4, 1e-5, 2, 1000, 1.0)
            nbytes = int(getattr(_lib.lib(), f"mrirt_{'siren' if family == 'siren' else 'inr'}_train_run_scratch_bytes")(
                C.byref(desc), C.byref(cache.desc), C.byref(cfg)))
            run_scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # one buffer for every timed call

            def run():
                return inr.train_run(desc, cache, cfg, st, args.run_steps, run_scratch)
            row[family] = dict(scratch_bytes=scratch.numel(), forward_ms=timed(forward, args.iters, args.warmup),
                               step_ms=timed(step, args.iters, args.warmup),
                               optimiser_step_ms=timed(run, args.iters, max(1, args.warmup // 2), per=args.run_steps))
        flop = 3 * 2 * n * sum(a * b for a, b in zip(dims[:-1], dims[1:]))
        row["siren_matrix_tflops"] = flop / (row["siren"]["step_ms"]["median"] * 1e-3) / 1e12
        row["ratio_forward"] = row["siren"]["forward_ms"]["median"] / row["relu"]["forward_ms"]["median"]
        row["ratio_step"] = row["siren"]["step_ms"]["median"] / row["relu"]["step_ms"]["median"]
        row["ratio_optimiser_step"] = row["siren"]["optimiser_step_ms"]["median"] / row["relu"]["optimiser_step_ms"]["median"]
        rows.append(row)
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, run_steps=args.run_steps, w0=W0, rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
