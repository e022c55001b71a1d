#!/usr/bin/env python3
"""Time one INR training step — mrirt_inr_forward_f32 + mrirt_inr_loss + mrirt_inr_backward — at two shapes, and torch's own
autograd of the same function (fp32 matmuls, log_softmax, the same loss) on the same GPU as a point of comparison.

Per shape: inputs, weights and scratch already on the device, `--warmup` untimed steps, then `--iters` steps each bracketed by
its own pair of events on the launch stream (device time of the whole pipeline of launches; nothing is read back).  Reported:
median, min, max in ms, and the fp32 FLOP rate of the matrix products (2 n sum_l in_l out_l forward, twice that backward).

    python tools/inr_train_timing.py [--iters 20] [--warmup 5] [--out profiles/r09_inr_train/timing.json]
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

SHAPES = [dict(K=4, M=4, hidden=64, hidden_layers=4, classes=4, n=4096), dict(K=16, M=4, hidden=256, hidden_layers=4, classes=4, n=65536)]
CW, DW = [0.5, 1.0, 2.0, 1.5], 0.5


def timed(fn, iters, warmup):
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
        ms.append(e0.elapsed_time(e1))
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import inr_ref
    from mrirt import inr
    dev = torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32 = False
    rows = []
    for s in SHAPES:
        rng = np.random.default_rng(1)
        dims = [3 + 6 * s["K"] + s["M"]] + [s["hidden"]] * s["hidden_layers"] + [s["classes"]]
        layers = inr_ref.fourier_params(rng, dims)
        n = s["n"]
        coords = torch.from_numpy((rng.random((n, 3)) * 2 - 1).astype(np.float32)).to(dev)
        feats = torch.from_numpy(rng.standard_normal((n, s["M"])).astype(np.float32)).to(dev)
        labels = torch.from_numpy(rng.integers(0, s["classes"], n).astype(np.int32)).to(dev)
        Ws = [torch.from_numpy(p["W"]).to(dev) for p in layers]
        bs = [torch.from_numpy(p["b"]).to(dev) for p in layers]
        desc = inr.train_desc(dims, s["K"], s["M"])
        w_flat, b_flat = torch.cat([W.reshape(-1) for W in Ws]), torch.cat(bs)
        scratch = inr.train_scratch(desc, n, dev)

        def ours():
            logits = inr.forward_f32(desc, w_flat, b_flat, coords, feats, n, scratch)
            _, _, dl = inr.loss_and_dlogits(logits, labels, CW, DW, scratch)
            return inr.backward_f32(desc, w_flat, n, dl, scratch)

        tW = [W.clone().requires_grad_(True) for W in Ws]
        tb = [b.clone().requires_grad_(True) for b in bs]
        cw, lab64 = torch.tensor(CW, device=dev), labels.to(torch.int64)

        def torch_autograd():
            h = inr.build_input(coords, feats, s["K"])
            for i, (W, b) in enumerate(zip(tW, tb)):
                h = h @ W + b
                if i + 1 < len(tW):
                    h = torch.relu(h)
            y = torch.nn.functional.one_hot(lab64, s["classes"]).to(torch.float32)
            ce = (-(y * torch.log_softmax(h, -1)).sum(-1) * cw[lab64]).mean()
            p = torch.softmax(h, -1)
            dice = (2 * (p * y).sum(0) + 1e-6) / (p.sum(0) + y.sum(0) + 1e-6)
            loss = (1 - DW) * ce + DW * (1 - dice.mean())
            return torch.autograd.grad(loss, tW + tb)

        flop = 3 * 2 * n * sum(a * b for a, b in zip(dims[:-1], dims[1:]))
        a, t = timed(ours, args.iters, args.warmup), timed(torch_autograd, args.iters, args.warmup)
        rows.append(dict(shape=s, dims=dims, scratch_bytes=scratch.numel(), step_ms=a, torch_autograd_ms=t,
                         matrix_tflops=flop / (a["median"] * 1e-3) / 1e12))
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
