#!/usr/bin/env python3
"""Steps per second of the INR training loop: mrirt_inr_train_run (sampler + step + clipped AdamW enqueued by one C call)
against the loop a caller had to write before it — a ``torch.randint`` gather from one pre-flattened case,
``inr.make_loss_and_grad`` and ``torch.optim.AdamW``, one Python iteration per step (tools/inr_fit.py as it was) — on the same
GPU, at two shapes with accum = 1.

Per shape and loop: ``--warmup`` untimed chunks, then ``--chunks`` chunks of ``--steps`` optimiser steps, each chunk bracketed
by a pair of events on the launch stream; the median chunk gives steps per second.  The split of one step into sampler /
forward + loss + backward / optimiser is timed the same way on the separate entry points (median of ``--chunks`` x ``--steps``
calls each).  Nothing is read back inside a timed region.

    python tools/inr_loop_timing.py [--chunks 20] [--steps 50] [--warmup 3] [--out profiles/r10_inr_loop/timing.json]
"""
import argparse
import json
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = [dict(K=4, M=4, hidden=64, hidden_layers=4, classes=4, micro=4096), dict(K=16, M=4, hidden=256, hidden_layers=4, classes=4, micro=65536)]
CW, DW, SIZE = [0.5, 1.0, 2.0, 1.5], 0.5, 64


def timed_chunks(fn, chunks, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(chunks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from mrirt import inr
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    cases = [{"mods": rng.standard_normal((4, SIZE, SIZE, SIZE)).astype(np.float32), "seg": rng.integers(0, 4, (SIZE, SIZE, SIZE)).astype(np.int16)}
             for _ in range(2)]
    cache = inr.VoxelCache(cases)
    rows = []
    for s in SHAPES:
        n, K, steps = s["micro"], s["K"], args.steps
        dims = [3 + 6 * K + s["M"]] + [s["hidden"]] * s["hidden_layers"] + [s["classes"]]
        desc = inr.train_desc(dims, K, s["M"])
        cfg = inr.train_cfg(n, 1, 0, CW, DW, 1e-3, 1e-5, 10, 10 ** 6, 1.0)
        st = inr.AdamWState.from_params(inr.init_mlp(0, dims[0], dims[1:-1], dims[-1]))
        nbytes = int(inr._lib.lib().mrirt_inr_train_run_scratch_bytes(inr.C.byref(desc), inr.C.byref(cache.desc), inr.C.byref(cfg)))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        run = timed_chunks(lambda: inr.train_run(desc, cache, cfg, st, steps, scratch), args.chunks, args.warmup)

        # the loop before this entry point: pre-flattened case, torch.randint gather, make_loss_and_grad, torch.optim.AdamW
        grid = np.stack(np.meshgrid(*[np.arange(SIZE)] * 3, indexing="ij"), -1).reshape(-1, 3)
        coords = torch.from_numpy((grid / (SIZE - 1) * 2.0 - 1.0).astype(np.float32)).to(dev)
        feats = torch.from_numpy(np.ascontiguousarray(cases[0]["mods"].transpose(1, 2, 3, 0).reshape(-1, 4))).to(dev)
        labels = torch.from_numpy(cases[0]["seg"].reshape(-1).astype(np.int32)).to(dev)
        params = [{"W": torch.from_numpy(p["W"]).to(dev), "b": torch.from_numpy(p["b"]).to(dev)} for p in inr.init_mlp(0, dims[0], dims[1:-1], dims[-1])]
        opt = torch.optim.AdamW([p[k] for p in params for k in ("W", "b")], lr=1e-3, weight_decay=1e-4)
        step_fn = inr.make_loss_and_grad(s["classes"], CW, DW, K)
        gen = torch.Generator(device=dev).manual_seed(0)

        def old_loop():
            for _ in range(steps):
                idx = torch.randint(0, coords.shape[0], (n,), device=dev, generator=gen)
                (_, _), grads = step_fn(params, coords[idx], feats[idx], labels[idx])
                for p, g in zip(params, grads):
                    p["W"].grad, p["b"].grad = g["W"], g["b"]
                opt.step()
        old = timed_chunks(old_loop, args.chunks, args.warmup)

        # the split of one step, on the separate entry points
        tr = inr.train_scratch(desc, n, dev)
        gw, gb = torch.empty_like(st.w), torch.empty_like(st.b)
        c, f, lab = cache.sample(0, 0, n)

        def many(fn):
            def run_many():
                for _ in range(steps):
                    fn()
            return run_many

        def fwd_bwd():
            logits = inr.forward_f32(desc, st.w, st.b, c, f, n, tr)
            _, _, dl = inr.loss_and_dlogits(logits, lab, CW, DW, tr)
            inr.backward_f32(desc, st.w, n, dl, tr, gw, gb)
        split = {name: timed_chunks(many(fn), args.chunks, args.warmup)["median"] / steps for name, fn in (
            ("sampler_ms", lambda: cache.sample(0, 1, n)), ("step_ms", fwd_bwd), ("optimiser_ms", lambda: inr.adamw_step(st, gw, gb, 1e-4, clip_norm=1.0)))}
        rows.append(dict(shape=s, dims=dims, params=int(st.w.numel() + st.b.numel()), scratch_bytes=nbytes, train_run_chunk_ms=run, parent_loop_chunk_ms=old,
                         train_run_steps_per_s=steps / (run["median"] * 1e-3), parent_loop_steps_per_s=steps / (old["median"] * 1e-3),
                         speedup=old["median"] / run["median"], split_python_calls=split))
    res = dict(device=torch.cuda.get_device_name(0), chunks=args.chunks, steps=args.steps, warmup=args.warmup, rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
